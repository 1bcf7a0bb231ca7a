// Batched policy evaluation for MI355X (gfx950): the per-episode record of the reference's play tool
// (scripts/rlgames_play_loopz.py: _compute_step_metrics :305-433, _infer_done_reason :493-501, the episode
// loop's accumulators :1144-1321, _summarize_eval :1046-1073), kept for EVERY env on the device instead of
// env 0 on the host.
//
// One thread per env, struct-of-arrays: every load and store below is a coalesced per-lane stream (the
// obstacle rows [16][2][n] included).  No atomics and no cross-env communication in the per-step kernels:
// episode k of env e owns column k * n + e of the table.  The arithmetic is written operation by operation
// in the reference's precisions (the build has -ffp-contract=off), so a record equals the host loop's bits:
// Python floats are doubles, the obstacle distances and the action delta's 2-norm are numpy float32.
// sqrtf / sqrt are the correctly rounded ones of this build (as in usv_device.h); __fsqrt_rn is NOT: without
// OCML_BASIC_ROUNDED_OPERATIONS the compiler's header maps it to the native, 1-ulp square root.
#include "usv_device.h"

#include <cmath>

namespace {

constexpr int kEvBlock = 256;
constexpr int kSumBlock = 1024;   // usv_eval_summary: one workgroup (see k_eval_summary)

__device__ __forceinline__ double ev_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// min over the 16 obstacles of the float32 distance sqrt(dx * dx + dy * dy), d = obstacle - position
// (_compute_step_metrics :379-382: float32 subtraction, product, two-term sum and sqrt, then np.min)
__device__ __forceinline__ float ev_min_obs(const usv_bufs_t &b, int e, float px, float py) {
  const size_t n = (size_t)b.n;
  float m = INFINITY;
#pragma unroll
  for (int o = 0; o < USV_NOBST; ++o) {
    const float dx = b.obst[(size_t)(2 * o) * n + e] - px;
    const float dy = b.obst[(size_t)(2 * o + 1) * n + e] - py;
    const float d = sqrtf(dx * dx + dy * dy);
    m = d < m ? d : m;
  }
  return m;
}

__global__ void __launch_bounds__(kEvBlock) k_eval_begin(usv_eval_t ev, int n) {
  const size_t i = (size_t)blockIdx.x * kEvBlock + threadIdx.x;
  const size_t cols = (size_t)ev.max_episodes * n;
  if (i < cols) {
#pragma unroll 1
    for (int r = 0; r < USV_EV_ROWS; ++r) ev.episodes[(size_t)r * cols + i] = 0.0;
  }
  if (i < (size_t)n) {
#pragma unroll 1
    for (int r = 0; r < USV_EVA_ROWS; ++r) ev.acc[(size_t)r * n + i] = 0.0;
    ev.ep_count[i] = 0;
  }
}

__global__ void __launch_bounds__(kEvBlock) k_eval_mark(usv_bufs_t b, usv_eval_t ev) {
  const int e = blockIdx.x * kEvBlock + threadIdx.x;
  if (e >= b.n || b.just_reset[e] == 0) return;
  const size_t n = (size_t)b.n;
  double *a = ev.acc + e;
  const double sx = (double)b.px[e], sy = (double)b.py[e];
  a[USV_EVA_START_X * n] = sx;
  a[USV_EVA_START_Y * n] = sy;
  a[USV_EVA_GOAL_X * n] = (double)b.tgt_x[e];
  a[USV_EVA_GOAL_Y * n] = (double)b.tgt_y[e];
  a[USV_EVA_PREV_X * n] = sx;
  a[USV_EVA_PREV_Y * n] = sy;
  a[USV_EVA_PREV_A0 * n] = 0.0;
  a[USV_EVA_PREV_A1 * n] = 0.0;
  a[USV_EVA_HAS_PREV * n] = 0.0;
  a[USV_EVA_DSUM * n] = 0.0;
  a[USV_EVA_DCOUNT * n] = 0.0;
  a[USV_EVA_SAT * n] = 0.0;
  a[USV_EVA_STEPS * n] = 0.0;
  a[USV_EVA_RET * n] = 0.0;
  a[USV_EVA_PATH * n] = 0.0;
  a[USV_EVA_MIN_OBS * n] = (double)INFINITY;
}

__global__ void __launch_bounds__(kEvBlock) k_eval_step(usv_cfg_t c, usv_bufs_t b, usv_eval_t ev,
                                                        const float *__restrict__ actions) {
  const int e = blockIdx.x * kEvBlock + threadIdx.x;
  if (e >= b.n) return;
  const size_t n = (size_t)b.n;
  double *a = ev.acc + e;
  // ---- the step, in the host loop's order (:1225-1279) ----
  const float act0 = actions[2 * (size_t)e], act1 = actions[2 * (size_t)e + 1];
  double dsum = a[USV_EVA_DSUM * n], dcount = a[USV_EVA_DCOUNT * n];
  if (a[USV_EVA_HAS_PREV * n] != 0.0) {
    // np.linalg.norm(action0 - prev_action0) on float32: sqrt(d . d) in float32
    const float d0 = act0 - (float)a[USV_EVA_PREV_A0 * n];
    const float d1 = act1 - (float)a[USV_EVA_PREV_A1 * n];
    dsum = dsum + (double)sqrtf(d0 * d0 + d1 * d1);
    dcount = dcount + 1.0;
  }
  a[USV_EVA_PREV_A0 * n] = (double)act0;
  a[USV_EVA_PREV_A1 * n] = (double)act1;
  a[USV_EVA_HAS_PREV * n] = 1.0;
  a[USV_EVA_DSUM * n] = dsum;
  a[USV_EVA_DCOUNT * n] = dcount;
  // np.abs(action0) > 0.95 * action_scale: the Python float joins the float32 array as a float32
  const float sat_thr = (float)(0.95 * (double)ev.action_scale);
  const double sat = a[USV_EVA_SAT * n] + (double)((fabsf(act0) > sat_thr ? 1 : 0) + (fabsf(act1) > sat_thr ? 1 : 0));
  a[USV_EVA_SAT * n] = sat;
  const double ret = a[USV_EVA_RET * n] + (double)b.rew[e];
  a[USV_EVA_RET * n] = ret;
  const float pxf = b.px[e], pyf = b.py[e];
  const double px = (double)pxf, py = (double)pyf;
  const double ddx = px - a[USV_EVA_PREV_X * n], ddy = py - a[USV_EVA_PREV_Y * n];
  const double path = a[USV_EVA_PATH * n] + sqrt(ddx * ddx + ddy * ddy);
  a[USV_EVA_PATH * n] = path;
  a[USV_EVA_PREV_X * n] = px;
  a[USV_EVA_PREV_Y * n] = py;
  const double steps = a[USV_EVA_STEPS * n] + 1.0;
  a[USV_EVA_STEPS * n] = steps;
  const float min_obs = ev_min_obs(b, e, pxf, pyf);
  const double seen = a[USV_EVA_MIN_OBS * n];
  const double min_ep = (double)min_obs < seen ? (double)min_obs : seen;
  a[USV_EVA_MIN_OBS * n] = min_ep;
  if (b.reset_buf[e] == 0) return;
  // ---- the episode ended: m_end and the episode-level metrics (:1304-1321) ----
  const int k = ev.ep_count[e];
  ev.ep_count[e] = k + 1;
  if (k >= ev.max_episodes) return;   // counted, not kept
  const double gx = (double)b.tgt_x[e], gy = (double)b.tgt_y[e];
  const double gdx = gx - px, gdy = gy - py;
  const double dist = sqrt(gdx * gdx + gdy * gdy);
  const bool coll = (double)min_obs < (double)c.collision_threshold;
  const bool oob = dist > (double)c.kill_dist;
  const bool tol = dist < (double)c.position_tolerance;
  const int reason = coll ? USV_EV_REASON_COLLISION : oob ? USV_EV_REASON_OOB : tol ? USV_EV_REASON_GOAL
                                                                                 : USV_EV_REASON_OTHER;
  const bool success = reason == USV_EV_REASON_GOAL;
  const double sx = a[USV_EVA_START_X * n], sy = a[USV_EVA_START_Y * n];
  const double g0x = a[USV_EVA_GOAL_X * n], g0y = a[USV_EVA_GOAL_Y * n];
  const double ex = g0x - sx, ey = g0y - sy;
  const double straight = sqrt(ex * ex + ey * ey);
  const size_t ncol = (size_t)ev.max_episodes * n;
  double *r = ev.episodes + (size_t)k * n + e;
  r[USV_EV_SUCCESS * ncol] = success ? 1.0 : 0.0;
  r[USV_EV_REASON * ncol] = (double)reason;
  r[USV_EV_LEN_STEPS * ncol] = steps;
  r[USV_EV_TIME_TO_GOAL * ncol] = success ? steps * ev.control_dt : ev_nan();
  r[USV_EV_RETURN * ncol] = ret;
  r[USV_EV_PATH_LENGTH * ncol] = path;
  r[USV_EV_STRAIGHT * ncol] = straight;
  r[USV_EV_PATH_EFF * ncol] = straight / (path > 1e-6 ? path : 1e-6);
  r[USV_EV_SMOOTH_MEAN * ncol] = dcount > 0.0 ? dsum / dcount : ev_nan();
  r[USV_EV_SMOOTH_SUM * ncol] = dsum;
  r[USV_EV_SAT_RATE * ncol] = sat / (2.0 * steps);
  r[USV_EV_COLLISION * ncol] = coll ? 1.0 : 0.0;
  r[USV_EV_OOB * ncol] = oob ? 1.0 : 0.0;
  r[USV_EV_IN_TOL * ncol] = tol ? 1.0 : 0.0;
  r[USV_EV_DIST_TO_GOAL * ncol] = dist;
  r[USV_EV_START_X * ncol] = sx;
  r[USV_EV_START_Y * ncol] = sy;
  r[USV_EV_GOAL_X * ncol] = g0x;
  r[USV_EV_GOAL_Y * ncol] = g0y;
  r[USV_EV_END_X * ncol] = px;
  r[USV_EV_END_Y * ncol] = py;
  r[USV_EV_END_YAW * ncol] = (double)b.yaw[e];
  r[USV_EV_MIN_OBS_END * ncol] = (double)min_obs;
  r[USV_EV_MIN_OBS_EP * ncol] = min_ep;
  r[USV_EV_SCENE_IDX * ncol] = b.scene_last ? (double)b.scene_last[e] : -1.0;
  r[USV_EV_ENV_SUCC * ncol] = (double)b.done_succ[e];
  r[USV_EV_ENV_COLL * ncol] = (double)b.done_coll[e];
  r[USV_EV_SMOOTH_COUNT * ncol] = dcount;
  r[USV_EV_SAT_COUNT * ncol] = sat;
}

// Sum of v over the workgroup in a fixed order: a balanced tree over the thread index in LDS (every thread
// gets the total).  Ends with a barrier, so sh can be reused at once.
__device__ __forceinline__ double ev_block_sum(double v, double *sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
#pragma unroll 1
  for (int s = kSumBlock / 2; s > 0; s >>= 1) {
    if (t < s) sh[t] = sh[t] + sh[t + s];
    __syncthreads();
  }
  const double total = sh[0];
  __syncthreads();
  return total;
}

// The summary is one workgroup: it runs once per evaluation over a few million doubles (131,072 envs x 9 rows
// = 9 MB in the first pass, 6 MB in the second), which one CU reads in about a millisecond, and a single workgroup
// needs no partials buffer, no second launch and no completion counter to be deterministic: thread t folds the
// columns k * n + e of its envs e = t, t + 1024, ... in ascending order (coalesced across the workgroup), then
// the tree above.  Pass 1: the counts and every metric's finite count and sum; pass 2: the squared deviations.
__global__ void __launch_bounds__(kSumBlock) k_eval_summary(usv_eval_t ev, int n, double *__restrict__ out) {
  __shared__ double sh[kSumBlock];
  const int t = threadIdx.x;
  const size_t ncol = (size_t)ev.max_episodes * n;
  constexpr int metric_row[USV_EVS_NMETRIC] = {USV_EV_SUCCESS,     USV_EV_TIME_TO_GOAL, USV_EV_PATH_EFF,
                                               USV_EV_SMOOTH_MEAN, USV_EV_SAT_RATE,     USV_EV_RETURN};
  // counts: episodes, dropped, the four reasons, collision, out of bounds
  double cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double c[USV_EVS_NMETRIC] = {0, 0, 0, 0, 0, 0}, s[USV_EVS_NMETRIC] = {0, 0, 0, 0, 0, 0};
  for (int e = t; e < n; e += kSumBlock) {
    const int k = ev.ep_count[e];
    if (k > ev.max_episodes) cnt[USV_EVS_DROPPED] += (double)(k - ev.max_episodes);
  }
#pragma unroll 1
  for (int k = 0; k < ev.max_episodes; ++k) {
    for (int e = t; e < n; e += kSumBlock) {
      if (k >= ev.ep_count[e]) continue;
      const double *col = ev.episodes + (size_t)k * n + e;
      cnt[USV_EVS_EPISODES] += 1.0;
      const double reason = col[(size_t)USV_EV_REASON * ncol];
#pragma unroll
      for (int r = 0; r < 4; ++r) cnt[USV_EVS_REASONS + r] += reason == (double)r ? 1.0 : 0.0;
      cnt[USV_EVS_COLLISION] += col[(size_t)USV_EV_COLLISION * ncol];
      cnt[USV_EVS_OOB] += col[(size_t)USV_EV_OOB * ncol];
#pragma unroll
      for (int m = 0; m < USV_EVS_NMETRIC; ++m) {
        const double v = col[(size_t)metric_row[m] * ncol];
        if (isfinite(v)) {
          c[m] += 1.0;
          s[m] += v;
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const double total = ev_block_sum(cnt[q], sh);
    if (t == 0) out[q] = total;
  }
  double count[USV_EVS_NMETRIC], mean[USV_EVS_NMETRIC], dev2[USV_EVS_NMETRIC] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int m = 0; m < USV_EVS_NMETRIC; ++m) {
    count[m] = ev_block_sum(c[m], sh);
    mean[m] = ev_block_sum(s[m], sh) / count[m];   // 0 / 0 = NaN when no value is finite
  }
#pragma unroll 1
  for (int k = 0; k < ev.max_episodes; ++k) {
    for (int e = t; e < n; e += kSumBlock) {
      if (k >= ev.ep_count[e]) continue;
      const double *col = ev.episodes + (size_t)k * n + e;
#pragma unroll
      for (int m = 0; m < USV_EVS_NMETRIC; ++m) {
        const double v = col[(size_t)metric_row[m] * ncol];
        if (isfinite(v)) {
          const double d = v - mean[m];
          dev2[m] += d * d;
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < USV_EVS_NMETRIC; ++m) {
    const double var = ev_block_sum(dev2[m], sh) / count[m];
    if (t == 0) {
      out[USV_EVS_METRICS + 3 * m] = count[m];
      out[USV_EVS_METRICS + 3 * m + 1] = count[m] > 0.0 ? mean[m] : ev_nan();
      out[USV_EVS_METRICS + 3 * m + 2] = count[m] > 0.0 ? sqrt(var) : ev_nan();
    }
  }
}

// argument checks shared by the four entry points (include/usv_hip.h: statuses 1, 2, 3)
int ev_check(const usv_cfg_t *cfg, const usv_bufs_t *b, const usv_eval_t *ev) {
  if (!cfg || !b || !ev || b->n <= 0) return 1;
  if (!ev->acc || !ev->episodes || !ev->ep_count) return 1;
  if (ev->max_episodes < 1 || (long long)ev->max_episodes * b->n > 0x7FFFFFFFLL) return 2;
  if (cfg->task_kind != USV_TASK_CAPTURE_XY) return 3;
  return 0;
}

int ev_check_env(const usv_bufs_t *b) {
  return (!b->px || !b->py || !b->yaw || !b->tgt_x || !b->tgt_y || !b->obst || !b->rew || !b->reset_buf ||
          !b->just_reset || !b->done_succ || !b->done_coll) ? 1 : 0;
}

}  // namespace

extern "C" {

int usv_eval_begin(const usv_cfg_t *cfg, const usv_bufs_t *b, const usv_eval_t *ev, void *stream) {
  if (const int rc = ev_check(cfg, b, ev)) return rc;
  const long long cols = (long long)ev->max_episodes * b->n;
  hipLaunchKernelGGL(k_eval_begin, dim3((unsigned)((cols + kEvBlock - 1) / kEvBlock)), dim3(kEvBlock), 0,
                     (hipStream_t)stream, *ev, b->n);
  USV_CHECK_LAUNCH();
  return 0;
}

int usv_eval_mark(const usv_cfg_t *cfg, const usv_bufs_t *b, const usv_eval_t *ev, void *stream) {
  if (const int rc = ev_check(cfg, b, ev)) return rc;
  if (ev_check_env(b)) return 1;
  hipLaunchKernelGGL(k_eval_mark, dim3((b->n + kEvBlock - 1) / kEvBlock), dim3(kEvBlock), 0, (hipStream_t)stream, *b,
                     *ev);
  USV_CHECK_LAUNCH();
  return 0;
}

int usv_eval_step(const usv_cfg_t *cfg, const usv_bufs_t *b, const usv_eval_t *ev, const float *actions,
                  void *stream) {
  if (const int rc = ev_check(cfg, b, ev)) return rc;
  if (ev_check_env(b) || !actions) return 1;
  hipLaunchKernelGGL(k_eval_step, dim3((b->n + kEvBlock - 1) / kEvBlock), dim3(kEvBlock), 0, (hipStream_t)stream,
                     *cfg, *b, *ev, actions);
  USV_CHECK_LAUNCH();
  return 0;
}

int usv_eval_summary(const usv_cfg_t *cfg, const usv_bufs_t *b, const usv_eval_t *ev, double *out, void *stream) {
  if (const int rc = ev_check(cfg, b, ev)) return rc;
  if (!out) return 1;
  hipLaunchKernelGGL(k_eval_summary, dim3(1), dim3(kSumBlock), 0, (hipStream_t)stream, *ev, b->n, out);
  USV_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
