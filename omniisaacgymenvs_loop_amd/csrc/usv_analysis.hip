// Analysis of a comparison for MI355X (gfx950): what the reference's analyze_play_csv.py computes from two play CSVs
// (paired per-scene deltas :633-650, the bootstrap of the mean :198-257, the percentile interval), on the evaluator
// tables that already sit on the device.
//
// Pair deltas: one thread per scenario, double sums in rollout order, as k_cmp_fold.
// Bootstrap: a workgroup per (segment, block of kAnaReps replicates).  The segment is staged once in LDS when it fits
// (USV_ANA_LDS_DOUBLES doubles = 128 KB of the 160 KB), else gathered from global memory; the two classes launch apart,
// each with the dynamic LDS that sets its residency; one wave per replicate, lanes striding over groups of four draws (one Philox4x32-10 call gives four indices).  A lane sums its
// draws in index order and the 64 lanes are folded by a fixed butterfly: no atomics, the same bits on every run.
// Quantiles: one workgroup per row, a bitonic sort in LDS, numpy's _lerp on the order statistics.
#include "usv_device.h"

#include <cmath>

namespace {

constexpr int kAnaBlock = 256;
constexpr int kAnaWaves = kAnaBlock / 64;
constexpr int kAnaReps = 32;    // replicates per workgroup: the staging of the segment is shared by them
constexpr int kAnaSegs = 64;    // segments per launch: their offsets travel as kernel arguments
// A launch that gathers from global memory runs best at one workgroup per CU once its segments outgrow an XCD's 4 MiB
// L2 (more workgroups in flight keep more segments live at once: 13.1 ms against 16.1-17.3 ms at 2, 5 and 8 per CU for
// 8.4 MB of segments), and at full occupancy while they fit (2.07 against 2.46 ms for 1.75 MB).  The limiter is
// dynamic LDS that nothing reads.
constexpr int kAnaGatherLds = (int)(USV_ANA_LDS_DOUBLES * sizeof(double));
constexpr long long kAnaL2Bytes = 4ll << 20;

// ------------------------------------------------------------------ pair deltas
struct SideSums {
  double sum[USV_ANA_PD_ROWS], cnt[USV_ANA_PD_ROWS];
};

__device__ __forceinline__ void side_add(SideSums &a, int m, double v) {
  if (v == v) {   // nanmean: a NaN is left out of the sum and of the count
    a.sum[m] += v;
    a.cnt[m] += 1.0;
  }
}

__device__ __forceinline__ SideSums side_fold(const usv_eval_t &ev, int n, int s, int R, int K, double reward_scale) {
  SideSums a{};
  const size_t ncol = (size_t)ev.max_episodes * n;
#pragma unroll 1
  for (int r = 0; r < R; ++r) {
    const long long p = (long long)s * R + r;
    const int e = (int)(p / K), k = (int)(p % K);
    const int cnt = ev.ep_count[e];
    if (k >= (cnt < K ? cnt : K)) continue;
    const double *col = ev.episodes + (size_t)k * n + e;
    const double succ = col[(size_t)USV_EV_SUCCESS * ncol], ret = col[(size_t)USV_EV_RETURN * ncol];
    side_add(a, USV_ANA_PD_SUCCESS, succ);
    side_add(a, USV_ANA_PD_COLLISION, col[(size_t)USV_EV_COLLISION * ncol]);
    side_add(a, USV_ANA_PD_OOB, col[(size_t)USV_EV_OOB * ncol]);
    side_add(a, USV_ANA_PD_RET_SCALED, ret * reward_scale);
    side_add(a, USV_ANA_PD_RET_RAW, ret);
    side_add(a, USV_ANA_PD_PATH_EFF, col[(size_t)USV_EV_PATH_EFF * ncol]);
    side_add(a, USV_ANA_PD_PATH_LEN, col[(size_t)USV_EV_PATH_LENGTH * ncol]);
    if (succ == 1.0) {
      side_add(a, USV_ANA_PD_TIME_SUCC, col[(size_t)USV_EV_TIME_TO_GOAL * ncol]);
      side_add(a, USV_ANA_PD_STEPS_SUCC, col[(size_t)USV_EV_LEN_STEPS * ncol]);
      side_add(a, USV_ANA_PD_MIN_OBS_SUCC, col[(size_t)USV_EV_MIN_OBS_EP * ncol]);
    }
  }
  return a;
}

__global__ void __launch_bounds__(kAnaBlock)
k_ana_pair_deltas(usv_eval_t control, usv_eval_t treat, int n, int S, int R, int K, double reward_scale,
                  double *__restrict__ out) {
  const int s = blockIdx.x * kAnaBlock + threadIdx.x;
  if (s >= S) return;
  const SideSums c = side_fold(control, n, s, R, K, reward_scale), t = side_fold(treat, n, s, R, K, reward_scale);
#pragma unroll
  for (int m = 0; m < USV_ANA_PD_ROWS; ++m) {
    const double mt = t.sum[m] / t.cnt[m], mc = c.sum[m] / c.cnt[m];   // 0 / 0 = NaN: a side without a row
    out[(size_t)m * S + s] = isfinite(mt) && isfinite(mc) ? mt - mc : (double)NAN;
  }
}

// ------------------------------------------------------------------ bootstrap of the mean
struct AnaSegs {
  long long off[kAnaSegs + 1], inj[kAnaSegs + 1];
};

__global__ void __launch_bounds__(kAnaBlock)
k_ana_bootstrap(AnaSegs sg, int j0, int lds_cap, int staged, const double *__restrict__ values, int B, uint64_t seed,
                const int32_t *__restrict__ inj_idx, int32_t *__restrict__ idx_out, double *__restrict__ means) {
  extern __shared__ double seg[];
  const int jl = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long off = sg.off[jl];
  const int len = (int)(sg.off[jl + 1] - off);
  const double *v = values + off;
  const bool in_lds = len <= lds_cap;   // the same in every thread of the workgroup
  if (in_lds != (staged != 0)) return;  // the other launch's segment (staged and gathered segments launch apart)
  if (in_lds) {
    for (int i = tid; i < len; i += kAnaBlock) seg[i] = v[i];
    __syncthreads();
  }
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), j = (uint32_t)(j0 + jl);
  const int groups = (len + 3) >> 2;
  const int b_end = min(B, ((int)blockIdx.x + 1) * kAnaReps);
  for (int b = (int)blockIdx.x * kAnaReps + wave; b < b_end; b += kAnaWaves) {
    const long long ib = sg.inj[jl] + (long long)b * len;
    double sum = 0.0;
    uint32_t cnt = 0u;
    for (int g = lane; g < groups; g += 64) {
      int32_t id[4];
      if (inj_idx) {
#pragma unroll
        for (int w = 0; w < 4; ++w) id[w] = 4 * g + w < len ? inj_idx[ib + 4 * g + w] : -1;
      } else {
        const u32x4 p = philox4x32_10(u32x4{(uint32_t)g, (uint32_t)b, j, (uint32_t)USV_ANA_SITE}, k0, k1);
        const uint32_t pw[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
        for (int w = 0; w < 4; ++w) id[w] = (int32_t)(((uint64_t)pw[w] * (uint64_t)(uint32_t)len) >> 32);
      }
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        if (4 * g + w >= len) continue;
        if (idx_out) idx_out[ib + 4 * g + w] = id[w];
        if ((uint32_t)id[w] >= (uint32_t)len) continue;   // an injected index outside the segment: a NaN draw
        const double x = in_lds ? seg[id[w]] : v[id[w]];
        if (x == x) {
          sum += x;
          cnt += 1u;
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {   // a + b == b + a: every lane holds the same bits after each stage
      sum += __shfl_xor(sum, o, 64);
      cnt += (uint32_t)__shfl_xor((int)cnt, o, 64);
    }
    if (lane == 0) means[(size_t)j * B + b] = cnt ? sum / (double)cnt : (double)NAN;
  }
}

// ------------------------------------------------------------------ quantiles
__global__ void __launch_bounds__(kAnaBlock)
k_ana_quantiles(const double *__restrict__ x, int B, const double *__restrict__ q, int nq, int nan_mode,
                double *__restrict__ out) {
  __shared__ double s[USV_ANA_MAX_BOOT];
  __shared__ int s_nan[kAnaWaves];
  const int tid = threadIdx.x;
  const double *xr = x + (size_t)blockIdx.x * B;
  int P = 1;
  while (P < B) P <<= 1;
  int nn = 0;
  for (int i = tid; i < P; i += kAnaBlock) {
    double v = i < B ? xr[i] : (double)INFINITY;
    if (v != v) {   // a NaN sorts last, as in numpy: it takes the place of a pad
      nn += 1;
      v = (double)INFINITY;
    }
    s[i] = v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nn += __shfl_xor(nn, o, 64);
  if ((tid & 63) == 0) s_nan[tid >> 6] = nn;
  __syncthreads();
  int nnan = 0;
#pragma unroll
  for (int w = 0; w < kAnaWaves; ++w) nnan += s_nan[w];
  for (int k = 2; k <= P; k <<= 1) {
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int t = tid; t < (P >> 1); t += kAnaBlock) {
        const int i = ((t & ~(jj - 1)) << 1) | (t & (jj - 1)), l = i | jj;
        const double a = s[i], b = s[l];
        if ((a > b) == ((i & k) == 0)) {
          s[i] = b;
          s[l] = a;
        }
      }
      __syncthreads();
    }
  }
  if (tid >= nq) return;
  const int m = nan_mode == USV_ANA_NAN_IGNORE ? B - nnan : B;
  double r = (double)NAN;
  if (m > 0 && !(nan_mode == USV_ANA_NAN_PROPAGATE && nnan > 0)) {
    double pos = q[tid] * (double)(m - 1);
    pos = pos > 0.0 ? (pos > (double)(m - 1) ? (double)(m - 1) : pos) : 0.0;   // q outside [0, 1] or NaN: stay in the row
    const double fl = floor(pos), g = pos - fl;
    const int lo = (int)fl, hi = lo + 1 < m ? lo + 1 : m - 1;
    const double a = s[lo], b = s[hi], d = b - a;
    r = g < 0.5 ? a + d * g : b - d * (1.0 - g);   // numpy's _lerp
  }
  out[(size_t)blockIdx.x * nq + tid] = r;
}

}  // namespace

extern "C" {

int usv_ana_pair_deltas(const usv_eval_t *control, const usv_eval_t *treat, int n, int S, int R, int K,
                        double reward_scale, double *out, void *stream) {
  if (!control || !treat || !out || !control->episodes || !control->ep_count || !treat->episodes ||
      !treat->ep_count || n <= 0 || S <= 0 || R <= 0 || K <= 0)
    return 1;
  const long long rows = (long long)S * R;
  if (S > USV_SCN_MAX_COUNT || rows > 0x7FFFFFFFLL || (long long)K != (rows + n - 1) / n ||
      K > control->max_episodes || control->max_episodes != treat->max_episodes ||
      (long long)control->max_episodes * n > 0x7FFFFFFFLL)
    return 2;
  hipLaunchKernelGGL(k_ana_pair_deltas, dim3((unsigned)((S + kAnaBlock - 1) / kAnaBlock)), dim3(kAnaBlock), 0,
                     (hipStream_t)stream, *control, *treat, n, S, R, K, reward_scale, out);
  USV_CHECK_LAUNCH();
  return 0;
}

int usv_ana_bootstrap(const double *values, const int64_t *seg_off, int J, int B, uint64_t seed,
                      const int32_t *inj_idx, const int64_t *inj_off, int32_t *idx_out, double *means, void *stream) {
  if (!values || !seg_off || !means || J < 1 || B < 1) return 1;
  if ((inj_idx || idx_out) && !inj_off) return 1;
  if (B > USV_ANA_MAX_BOOT) return 2;
  for (int j = 0; j < J; ++j) {
    const long long len = (long long)(seg_off[j + 1] - seg_off[j]);
    if (len < 0 || seg_off[j] < 0) return 1;
    if (len > USV_SCN_MAX_COUNT) return 2;
    if ((inj_idx || idx_out) && (inj_off[j] < 0 || (long long)(inj_off[j + 1] - inj_off[j]) < (long long)B * len))
      return 1;
  }
  for (int j0 = 0; j0 < J; j0 += kAnaSegs) {
    const int ns = J - j0 < kAnaSegs ? J - j0 : kAnaSegs;
    AnaSegs sg{};
    long long fits = 0;   // the longest segment of this chunk that fits the staging capacity
    int n_staged = 0, n_gather = 0;
    long long gather_bytes = 0;
    for (int i = 0; i <= ns; ++i) {
      sg.off[i] = (long long)seg_off[j0 + i];
      sg.inj[i] = inj_off ? (long long)inj_off[j0 + i] : 0;
      const long long len = i ? sg.off[i] - sg.off[i - 1] : 0;
      if (!i) continue;
      if (len <= USV_ANA_LDS_DOUBLES) {
        ++n_staged;
        if (len > fits) fits = len;
      } else {
        ++n_gather;
        gather_bytes += len * (long long)sizeof(double);
      }
    }
    // Staged and gathered segments launch apart, each with the dynamic LDS its class needs: the staged ones what
    // the longest of them takes, the gathered ones none while they fit the L2 and the one-workgroup-per-CU limiter
    // beyond (DESIGN section 16 has the measurement)
    const int lds_cap = (int)fits;
    for (int staged = 1; staged >= 0; --staged) {
      if (staged ? !n_staged : !n_gather) continue;
      const size_t lds = staged ? (size_t)lds_cap * sizeof(double)
                                : (gather_bytes > kAnaL2Bytes ? (size_t)kAnaGatherLds : 0);
      if (lds > 65536 && hipFuncSetAttribute((const void *)k_ana_bootstrap, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(USV_ANA_LDS_DOUBLES * sizeof(double))) != hipSuccess)
        return 90;
      hipLaunchKernelGGL(k_ana_bootstrap, dim3((unsigned)((B + kAnaReps - 1) / kAnaReps), (unsigned)ns),
                         dim3(kAnaBlock), lds, (hipStream_t)stream, sg, j0, lds_cap, staged, values, B, seed, inj_idx,
                         idx_out, means);
      USV_CHECK_LAUNCH();
    }
  }
  return 0;
}

int usv_ana_quantiles(const double *x, int J, int B, const double *q, int nq, int nan_mode, double *out,
                      void *stream) {
  if (!x || !q || !out || J < 1 || B < 1 || nq < 1) return 1;
  if (nan_mode != USV_ANA_NAN_PROPAGATE && nan_mode != USV_ANA_NAN_IGNORE) return 1;
  if (B > USV_ANA_MAX_BOOT || nq > USV_ANA_MAX_Q) return 2;
  hipLaunchKernelGGL(k_ana_quantiles, dim3((unsigned)J), dim3(kAnaBlock), 0, (hipStream_t)stream, x, B, q, nq,
                     nan_mode, out);
  USV_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
