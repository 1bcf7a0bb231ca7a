// Policy banks for MI355X (gfx950): what one rollout of n = M x G envs needs, beside ppo_policy_bank_step
// (ppo.hip), to evaluate M checkpoints at once -- the reference's omniisaacgymenvs/scripts/multi_model_eval.py
// (eval_multi_agents :39-113: one model after the other through one player, every observation copied to the host,
// success rates plus ALV / AAV / AAC per model).
//
// (1) usv_bank_uniforms: the paired run.  Env m G + i gets the random words env i of a G-env run draws, written
//     as the u_step / u_reset tables usv_env_step / usv_reset accept, so every model faces the same G scenarios and
//     group m equals a stand-alone G-env run of model m bit for bit.
// (2) usv_bank_begin / _step: the motion sums behind ALV / AAV / AAC, one thread per env, struct-of-arrays
//     (coalesced rows), no atomics; the norm as k_teval_step forms its own.
// (3) usv_bank_summary: one workgroup per group folds that group's columns of the usv_teval_t table exactly as
//     k_teval_summary folds a whole table (usv_tev_fold.h), then the motion rows in the same order.
#include "usv_device.h"
#include "usv_tev_fold.h"

namespace {

static_assert(USV_BEVS_SPEED_SUM == USV_TEVS_N && USV_BEVS_N == USV_TEVS_N + 4, "a summary row: teval's, then 4");
static_assert(USV_NU_STEP == 8 && SU_PX == 4, "u_step: two Philox blocks");

constexpr int kBankBlock = 256;
constexpr int kResetBlocks = (USV_NU_RESET + 3) / 4;   // Philox blocks of a reset row (the last one partly used)
constexpr int kResetTB = 192;                          // one lane per block: a row is written in 16-byte pieces
constexpr int kResetEnvs = 8;                          // envs per workgroup
static_assert(kResetBlocks <= kResetTB, "one lane per reset block");

// the step index the next usv_reset / usv_env_step pair uses: k_step_begin hands clock[0] to clock[2]
__device__ __forceinline__ uint64_t next_step_of(const usv_bufs_t &b, uint64_t step) {
  return b.clock ? b.clock[0] : step;
}

__global__ void __launch_bounds__(kBankBlock) k_bank_ustep(usv_cfg_t c, usv_bufs_t b, int group, uint64_t seed,
                                                           uint64_t step, float *__restrict__ u_step) {
  const int e = blockIdx.x * kBankBlock + threadIdx.x;
  if (e >= b.n) return;
  step = next_step_of(b, step);
  float u[USV_NU_STEP];
  philox_u4(seed, (uint32_t)(e % group), step, 0u, u);
  if (c.pos_noise_on || c.act_noise_on) philox_u4(seed, (uint32_t)(e % group), step, 1u, u + 4);
  else u[4] = u[5] = u[6] = u[7] = 0.f;
  float *row = u_step + (size_t)e * USV_NU_STEP;
#pragma unroll
  for (int i = 0; i < USV_NU_STEP; ++i) row[i] = u[i];
}

// lane t: block t of the row of every resetting env of this workgroup's kResetEnvs (the branch is uniform)
__global__ void __launch_bounds__(kResetTB) k_bank_ureset(usv_bufs_t b, int group, uint64_t seed, uint64_t step,
                                                          float *__restrict__ u_reset) {
  const int t = threadIdx.x;
  step = next_step_of(b, step);
  const int e0 = blockIdx.x * kResetEnvs;
#pragma unroll 1
  for (int e = e0; e < min(e0 + kResetEnvs, b.n); ++e) {
    if (b.reset_buf[e] == 0 || t >= kResetBlocks) continue;
    float u[4];
    philox_u4(seed, (uint32_t)(e % group), step, 0x100u + (uint32_t)t, u);
    float *row = u_reset + (size_t)e * USV_NU_RESET;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (4 * t + q < USV_NU_RESET) row[4 * t + q] = u[q];
  }
}

__global__ void __launch_bounds__(kBankBlock) k_bank_begin(double *__restrict__ motion, int n) {
  const int e = blockIdx.x * kBankBlock + threadIdx.x;
  if (e >= n) return;
#pragma unroll
  for (int r = 0; r < USV_BEV_ROWS; ++r) motion[(size_t)r * n + e] = 0.0;
}

__global__ void __launch_bounds__(kBankBlock) k_bank_step(int n, const float *__restrict__ obs,
                                                          const float *__restrict__ act, usv_bank_t bk) {
  const int e = blockIdx.x * kBankBlock + threadIdx.x;
  if (e >= n) return;
  const size_t N = (size_t)n;
  double *col = bk.motion + e;
  const double t = col[USV_BEV_STEPS * N];
  col[USV_BEV_STEPS * N] = t + 1.0;
  if (t >= (double)bk.horizon) return;
  const float *o = obs + (size_t)e * USV_NOBS;
  const float vx = o[0], vy = o[1];
  const float speed = sqrtf(__fadd_rn(__fmul_rn(vx, vx), __fmul_rn(vy, vy)));
  col[USV_BEV_SPEED_SUM * N] = col[USV_BEV_SPEED_SUM * N] + (double)speed;
  col[USV_BEV_YAWRATE_SUM * N] = col[USV_BEV_YAWRATE_SUM * N] + (double)fabsf(o[2]);
  col[USV_BEV_ACT_SUM * N] = col[USV_BEV_ACT_SUM * N] + ((double)act[2 * (size_t)e] + (double)act[2 * (size_t)e + 1]);
}

// workgroup m: group m's columns of both tables; thread t folds envs t, t + 1024, ... of the group, then the tree
__global__ void __launch_bounds__(kTevSumBlock) k_bank_summary(const double *__restrict__ table, int n, int nch,
                                                              usv_bank_t bk, double *__restrict__ out) {
  __shared__ double sh[kTevSumBlock];
  const int t = threadIdx.x, G = bk.group;
  const size_t N = (size_t)n, first = (size_t)blockIdx.x * G;
  double *row = out + (size_t)blockIdx.x * USV_BEVS_N;
  tev_summary_fold(table + first, N, G, nch, row, sh);
  const double *mo = bk.motion + first;
  double sum[3] = {0.0, 0.0, 0.0}, pairs = 0.0;
  for (int e = t; e < G; e += kTevSumBlock) {
#pragma unroll
    for (int q = 0; q < 3; ++q) sum[q] += mo[(size_t)q * N + e];
    const double steps = mo[USV_BEV_STEPS * N + e];
    pairs += steps < (double)bk.horizon ? steps : (double)bk.horizon;
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double total = tev_block_fold<kFoldSum>(sum[q], sh);
    if (t == 0) row[USV_BEVS_SPEED_SUM + q] = total;
  }
  pairs = tev_block_fold<kFoldSum>(pairs, sh);
  if (t == 0) row[USV_BEVS_PAIRS] = pairs;
}

int bank_check(const usv_cfg_t *cfg, const usv_bufs_t *b, const usv_bank_t *bk) {
  if (!cfg || !b || !bk || b->n <= 0 || !bk->motion) return 1;
  if (bk->models < 1 || bk->group < 1 || (long long)bk->models * bk->group != (long long)b->n || bk->horizon < 1)
    return 2;
  return 0;
}

}  // namespace

extern "C" {

int usv_bank_uniforms(const usv_cfg_t *cfg, const usv_bufs_t *b, int group, uint64_t seed, uint64_t step,
                      float *u_step, float *u_reset, void *stream) {
  if (!cfg || !b || !u_step || !u_reset || b->n <= 0 || !b->reset_buf) return 1;
  if (group < 1 || b->n % group != 0) return 2;
  hipLaunchKernelGGL(k_bank_ustep, dim3((b->n + kBankBlock - 1) / kBankBlock), dim3(kBankBlock), 0,
                     (hipStream_t)stream, *cfg, *b, group, seed, step, u_step);
  USV_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_bank_ureset, dim3((b->n + kResetEnvs - 1) / kResetEnvs), dim3(kResetTB), 0,
                     (hipStream_t)stream, *b, group, seed, step, u_reset);
  USV_CHECK_LAUNCH();
  return 0;
}

int usv_bank_begin(const usv_cfg_t *cfg, const usv_bufs_t *b, const usv_bank_t *bank, void *stream) {
  if (const int rc = bank_check(cfg, b, bank)) return rc;
  hipLaunchKernelGGL(k_bank_begin, dim3((b->n + kBankBlock - 1) / kBankBlock), dim3(kBankBlock), 0,
                     (hipStream_t)stream, bank->motion, b->n);
  USV_CHECK_LAUNCH();
  return 0;
}

int usv_bank_step(const usv_cfg_t *cfg, const usv_bufs_t *b, const usv_bank_t *bank, const float *actions,
                  void *stream) {
  if (const int rc = bank_check(cfg, b, bank)) return rc;
  if (!b->obs || !actions) return 1;
  hipLaunchKernelGGL(k_bank_step, dim3((b->n + kBankBlock - 1) / kBankBlock), dim3(kBankBlock), 0,
                     (hipStream_t)stream, b->n, b->obs, actions, *bank);
  USV_CHECK_LAUNCH();
  return 0;
}

int usv_bank_summary(const usv_cfg_t *cfg, const usv_bufs_t *b, const usv_teval_t *tev, const usv_bank_t *bank,
                     double *out, void *stream) {
  if (const int rc = bank_check(cfg, b, bank)) return rc;
  if (!tev || !tev->table || !out) return 1;
  const int nch = usv_teval_channels(cfg);
  if (nch < 1) return cfg->task_kind == USV_TASK_CAPTURE_XY ? 3 : 2;
  hipLaunchKernelGGL(k_bank_summary, dim3(bank->models), dim3(kTevSumBlock), 0, (hipStream_t)stream, tev->table,
                     b->n, nch, *bank, out);
  USV_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
