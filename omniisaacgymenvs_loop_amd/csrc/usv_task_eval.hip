// Fixed-horizon success-rate evaluation of the kinds without obstacles (GoToXY, KeepXY, GoToPose,
// TrackXYVelocity, TrackXYOVelocity) for MI355X (gfx950): the reference's omniisaacgymenvs/utils/eval_metrics.py
// (build_distance_dataframe :16-35, check_stay :38-54, the time-under shares of get_GoToPose_success_rate_new
// :83-91), which works on a [T][n][obs] host copy of every observation, restated as a streaming function of the
// per-step error with O(1) state per env, kept on the device next to the step kernel.
//
// One thread per env, struct-of-arrays table: every table row is a coalesced wave access; the observation row is
// read directly (5 of its 33 floats, a 132-byte lane stride).  No atomics, no cross-env communication.  The
// errors are formed as numpy forms them on the float32 observation: float32 products and a float32 sum without
// contraction (__fmul_rn / __fadd_rn), the correctly rounded sqrtf of this build (usv_eval.hip's header explains
// why not __fsqrt_rn), the heading through the library's own usv_atan2.  Every comparison is float32 against the
// float32-rounded level; thr / 2 and thr * 7.5 are formed in double and then rounded.  A NaN compares false.
#include "usv_device.h"
#include "usv_tev_fold.h"

#include <cmath>

namespace {

constexpr int kTevBlock = 256;    // usv_eval.hip's block shape

__host__ __device__ __forceinline__ int tev_channels(int kind) {
  switch (kind) {
    case USV_TASK_GO_TO_XY:
    case USV_TASK_KEEP_XY:
    case USV_TASK_TRACK_XY: return 1;
    case USV_TASK_GO_TO_POSE:
    case USV_TASK_TRACK_XYO: return 2;
    default: return 0;
  }
}

__global__ void __launch_bounds__(kTevBlock) k_teval_begin(double *__restrict__ table, int n) {
  const int e = blockIdx.x * kTevBlock + threadIdx.x;
  if (e >= n) return;
  const size_t N = (size_t)n;
#pragma unroll 1
  for (int r = 0; r < USV_TEV_ROWS; ++r) table[(size_t)r * N + e] = 0.0;
#pragma unroll
  for (int c = 0; c < USV_TEV_CH; ++c) {
    double *ch = table + (size_t)(USV_TEV_CH_STRIDE * c) * N + e;
    ch[USV_TEV_FIRST_THR * N] = -1.0;
    ch[USV_TEV_FIRST_THR2 * N] = -1.0;
    ch[USV_TEV_STAY * N] = 1.0;
  }
}

// kind is wave-uniform (one task per launch): the branches below do not diverge
__global__ void __launch_bounds__(kTevBlock) k_teval_step(int kind, int n, const float *__restrict__ obs,
                                                          const float *__restrict__ rew,
                                                          const int32_t *__restrict__ reset_buf, usv_teval_t tv) {
  const int e = blockIdx.x * kTevBlock + threadIdx.x;
  if (e >= n) return;
  const size_t N = (size_t)n;
  double *col = tv.table + e;
  const double t = col[USV_TEV_STEPS * N];   // the trace index
  col[USV_TEV_STEPS * N] = t + 1.0;
  if (t >= (double)tv.horizon) return;       // an overrunning host loop cannot change a finished record
  const float *o = obs + (size_t)e * USV_NOBS;
  float x[USV_TEV_CH] = {0.f, 0.f};
  if (kind == USV_TASK_TRACK_XY || kind == USV_TASK_TRACK_XYO) {
    const float a = o[3], b = o[4];
    x[0] = sqrtf(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)));
    if (kind == USV_TASK_TRACK_XYO) x[1] = fabsf(o[5]);
  } else {
    x[0] = o[5];
    if (kind == USV_TASK_GO_TO_POSE) x[1] = fabsf(usv_atan2(o[7], o[6]));
  }
  col[USV_TEV_RETURN * N] = col[USV_TEV_RETURN * N] + (double)rew[e];
  col[USV_TEV_RESETS * N] = col[USV_TEV_RESETS * N] + (reset_buf[e] != 0 ? 1.0 : 0.0);
  const int nch = tev_channels(kind);
#pragma unroll
  for (int c = 0; c < USV_TEV_CH; ++c) {
    if (c >= nch) break;
    double *ch = col + (size_t)(USV_TEV_CH_STRIDE * c) * N;
    const float xv = x[c];
    const float thr = tv.thr[c];
    const float thr2 = (float)((double)thr / 2.0);
    const float margin = (float)((double)thr * 7.5);
    bool stay = ch[USV_TEV_STAY * N] != 0.0 && xv < margin;
    if (ch[USV_TEV_FIRST_THR * N] < 0.0 && xv < thr) {
      ch[USV_TEV_FIRST_THR * N] = t;
      stay = true;   // check_stay looks from here on
    }
    ch[USV_TEV_STAY * N] = stay ? 1.0 : 0.0;
    if (ch[USV_TEV_FIRST_THR2 * N] < 0.0 && xv < thr2) ch[USV_TEV_FIRST_THR2 * N] = t;
#pragma unroll
    for (int l = 0; l < USV_TEV_LEVELS; ++l)
      if (xv < tv.level[c][l]) ch[(USV_TEV_UNDER0 + l) * N] = ch[(USV_TEV_UNDER0 + l) * N] + 1.0;
    ch[USV_TEV_ERR_SUM * N] = ch[USV_TEV_ERR_SUM * N] + (double)xv;
    ch[USV_TEV_ERR_LAST * N] = (double)xv;
  }
}

// One workgroup over the whole table (usv_tev_fold.h: the fold, its order and why one workgroup)
__global__ void __launch_bounds__(kTevSumBlock) k_teval_summary(const double *__restrict__ table, int n, int nch,
                                                               double *__restrict__ out) {
  __shared__ double sh[kTevSumBlock];
  tev_summary_fold(table, (size_t)n, n, nch, out, sh);
}

bool tev_pos_finite(float v) { return std::isfinite(v) && v > 0.f; }

// argument checks shared by the entry points (include/usv_hip.h: statuses 1, 2, 3)
int tev_check(const usv_cfg_t *cfg, const usv_bufs_t *b, const usv_teval_t *tv) {
  if (!cfg || !b || !tv || b->n <= 0 || !tv->table) return 1;
  if (tv->horizon < 1) return 2;
  if (cfg->task_kind == USV_TASK_CAPTURE_XY) return 3;
  const int nch = tev_channels(cfg->task_kind);
  if (nch < 1) return 2;   // not a kind of this header
  for (int c = 0; c < nch; ++c) {
    if (!tev_pos_finite(tv->thr[c])) return 2;
    for (int l = 0; l < USV_TEV_LEVELS; ++l)
      if (!tev_pos_finite(tv->level[c][l])) return 2;
  }
  return 0;
}

}  // namespace

extern "C" {

int usv_teval_channels(const usv_cfg_t *cfg) { return cfg ? tev_channels(cfg->task_kind) : 0; }

int usv_teval_begin(const usv_cfg_t *cfg, const usv_bufs_t *b, const usv_teval_t *tev, void *stream) {
  if (const int rc = tev_check(cfg, b, tev)) return rc;
  hipLaunchKernelGGL(k_teval_begin, dim3((b->n + kTevBlock - 1) / kTevBlock), dim3(kTevBlock), 0, (hipStream_t)stream,
                     tev->table, b->n);
  USV_CHECK_LAUNCH();
  return 0;
}

int usv_teval_step(const usv_cfg_t *cfg, const usv_bufs_t *b, const usv_teval_t *tev, void *stream) {
  if (const int rc = tev_check(cfg, b, tev)) return rc;
  if (!b->obs || !b->rew || !b->reset_buf) return 1;
  hipLaunchKernelGGL(k_teval_step, dim3((b->n + kTevBlock - 1) / kTevBlock), dim3(kTevBlock), 0, (hipStream_t)stream,
                     cfg->task_kind, b->n, b->obs, b->rew, b->reset_buf, *tev);
  USV_CHECK_LAUNCH();
  return 0;
}

int usv_teval_summary(const usv_cfg_t *cfg, const usv_bufs_t *b, const usv_teval_t *tev, double *out, void *stream) {
  if (const int rc = tev_check(cfg, b, tev)) return rc;
  if (!out) return 1;
  hipLaunchKernelGGL(k_teval_summary, dim3(1), dim3(kTevSumBlock), 0, (hipStream_t)stream, tev->table, b->n,
                     tev_channels(cfg->task_kind), out);
  USV_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
