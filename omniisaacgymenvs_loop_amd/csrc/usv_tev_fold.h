// The fixed-order fold of a usv_teval_t table into usv_teval_summary's [USV_TEVS_N] doubles, shared by
// k_teval_summary (usv_task_eval.hip: the whole table) and k_bank_summary (usv_bank.hip: one group of envs of it).
#pragma once
#include "usv_device.h"

namespace {

constexpr int kTevSumBlock = 1024;   // one workgroup per summary (see tev_summary_fold)

enum { kFoldSum = 0, kFoldMin = 1, kFoldMax = 2 };

// v folded over the workgroup in a fixed order: a balanced tree over the thread index in LDS (every thread gets
// the result).  Ends with a barrier, so sh can be reused at once.
template <int OP>
__device__ __forceinline__ double tev_block_fold(double v, double *sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
#pragma unroll 1
  for (int s = kTevSumBlock / 2; s > 0; s >>= 1) {
    if (t < s) {
      const double a = sh[t], b = sh[t + s];
      sh[t] = OP == kFoldSum ? a + b : OP == kFoldMin ? (b < a ? b : a) : (b > a ? b : a);
    }
    __syncthreads();
  }
  const double total = sh[0];
  __syncthreads();
  return total;
}

// One workgroup of kTevSumBlock threads folds the n envs whose columns start at `table` (row stride N doubles:
// the whole table has N = n; a group of envs is the table pointer moved to its first env with N unchanged).
// The table is 19 rows x n doubles (10 MB at 65,536 envs), read once per evaluation; a single workgroup needs no
// partials buffer, no second launch and no completion counter to be deterministic.  Thread t folds envs t,
// t + 1024, ... in ascending order (coalesced across the workgroup), then the tree above.  Pass 1: every count and
// sum; pass 2: the return's squared deviations.
__device__ __forceinline__ void tev_summary_fold(const double *__restrict__ table, size_t N, int n, int nch,
                                                 double *__restrict__ out, double *sh) {
  const int t = threadIdx.x;
  double smin = INFINITY, smax = -INFINITY, resets = 0.0, reset_envs = 0.0, rcount = 0.0, rsum = 0.0;
  double chv[USV_TEV_CH][USV_TEVS_CH_STRIDE];
#pragma unroll
  for (int c = 0; c < USV_TEV_CH; ++c)
#pragma unroll
    for (int q = 0; q < USV_TEVS_CH_STRIDE; ++q) chv[c][q] = 0.0;
  for (int e = t; e < n; e += kTevSumBlock) {
    const double *col = table + e;
    const double steps = col[USV_TEV_STEPS * N], r = col[USV_TEV_RESETS * N], ret = col[USV_TEV_RETURN * N];
    smin = steps < smin ? steps : smin;
    smax = steps > smax ? steps : smax;
    resets += r;
    reset_envs += r > 0.0 ? 1.0 : 0.0;
    if (isfinite(ret)) {
      rcount += 1.0;
      rsum += ret;
    }
#pragma unroll
    for (int c = 0; c < USV_TEV_CH; ++c) {
      if (c >= nch) break;
      const double *ch = col + (size_t)(USV_TEV_CH_STRIDE * c) * N;
      chv[c][USV_TEVS_N_THR] += ch[USV_TEV_FIRST_THR * N] > -1.0 ? 1.0 : 0.0;
      chv[c][USV_TEVS_N_THR2] += ch[USV_TEV_FIRST_THR2 * N] > -1.0 ? 1.0 : 0.0;
      chv[c][USV_TEVS_N_STAY] += ch[USV_TEV_STAY * N] != 0.0 ? 1.0 : 0.0;
#pragma unroll
      for (int l = 0; l < USV_TEV_LEVELS; ++l) chv[c][USV_TEVS_UNDER + l] += ch[(USV_TEV_UNDER0 + l) * N];
      chv[c][USV_TEVS_ERR_SUM] += ch[USV_TEV_ERR_SUM * N];
    }
  }
  smin = tev_block_fold<kFoldMin>(smin, sh);
  smax = tev_block_fold<kFoldMax>(smax, sh);
  resets = tev_block_fold<kFoldSum>(resets, sh);
  reset_envs = tev_block_fold<kFoldSum>(reset_envs, sh);
  if (t == 0) {
    out[USV_TEVS_ENVS] = (double)n;
    out[USV_TEVS_CHANNELS] = (double)nch;
    out[USV_TEVS_STEPS_MIN] = smin;
    out[USV_TEVS_STEPS_MAX] = smax;
    out[USV_TEVS_RESETS] = resets;
    out[USV_TEVS_RESET_ENVS] = reset_envs;
  }
#pragma unroll
  for (int c = 0; c < USV_TEV_CH; ++c)
#pragma unroll
    for (int q = 0; q < USV_TEVS_CH_STRIDE; ++q) {
      const double total = tev_block_fold<kFoldSum>(chv[c][q], sh);
      if (t == 0) out[USV_TEVS_CH + USV_TEVS_CH_STRIDE * c + q] = total;
    }
  const double count = tev_block_fold<kFoldSum>(rcount, sh);
  const double mean = tev_block_fold<kFoldSum>(rsum, sh) / count;   // 0 / 0 = NaN when no return is finite
  double dev2 = 0.0;
  for (int e = t; e < n; e += kTevSumBlock) {
    const double ret = table[USV_TEV_RETURN * N + e];
    if (isfinite(ret)) {
      const double d = ret - mean;
      dev2 += d * d;
    }
  }
  const double var = tev_block_fold<kFoldSum>(dev2, sh) / count;
  if (t == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    out[USV_TEVS_RETURN] = count;
    out[USV_TEVS_RETURN + 1] = count > 0.0 ? mean : nan;
    out[USV_TEVS_RETURN + 2] = count > 0.0 ? sqrt(var) : nan;
  }
}

}  // namespace
