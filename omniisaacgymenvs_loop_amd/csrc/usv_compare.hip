// Teacher-vs-student comparison for MI355X (gfx950): the privileged-tail overrides of the reference's compare tool
// (scripts/rlgames_play_loopz_compare.py: _compute_base_const_all_tail :184-293, _compute_wrong_random_tail
// :296-507, _override_obs_priv_tail :510-522) applied per env and per episode on the device, and the paired
// per-scenario fold of two evaluator tables.
//
// Tail: one thread per env, no atomics.  The reference computes the fake mass, the coupling ratio and the coupled
// scalars as Python floats (doubles) and rounds once when it builds the float32 tensors; the CoM and the encoders
// are float32.  The kernel keeps those precisions (the build has -ffp-contract=off).  Fold: one thread per scenario,
// double sums in rollout order, as k_scn_fold.
#include "usv_device.h"

#include <cmath>

namespace {

constexpr int kCmpBlock = 256;

// constants derived once on the host from usv_cfg_t
struct TailK {
  int mode, priv_dim, priv_mode, mass_relative, com_scaled, com_on, couple_drag, couple_thr, couple_kiz;
  double mass_lo, mass_hi, base_mass, mass_den, r_den, kdrag_min, kdrag_max, thr_rand, kiz_min, kiz_max;
  float base_com[3], com_disp[3], com_div[3];
  float nominal, enc_lo[3], enc_r[3], inv_enc_r[3];   // kdrag, thr, kiz: minmax range / centered scale
  int enc_ok[3];
};

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }
__device__ __forceinline__ double clampd(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

__global__ void __launch_bounds__(kCmpBlock)
k_priv_tail(TailK K, const float *obs_in, float *obs_out, int n, int obs_dim, const float *__restrict__ const_tail,
            const int32_t *__restrict__ episode, uint64_t seed) {
  const int e = blockIdx.x * kCmpBlock + threadIdx.x;
  if (e >= n) return;
  const int head = obs_dim - K.priv_dim;
  const float *in = obs_in + (size_t)e * obs_dim;
  float *out = obs_out + (size_t)e * obs_dim;
  if (in != out)
    for (int d = 0; d < head; ++d) out[d] = in[d];
  float *tail = out + head;
  if (K.mode == USV_PT_CONST) {
    for (int q = 0; q < K.priv_dim; ++q) tail[q] = const_tail[q];
    return;
  }
  const uint32_t ep = episode ? (uint32_t)episode[e] : 0u;
  const u32x4 w = philox4x32_10(u32x4{(uint32_t)e, ep, 0u, (uint32_t)USV_PT_SITE}, (uint32_t)seed,
                                (uint32_t)(seed >> 32));
  const double inv32 = 1.0 / 4294967296.0;
  const double m = K.mass_lo + (K.mass_hi - K.mass_lo) * ((double)w.x * inv32);
  const uint32_t wc[3] = {w.y, w.z, w.w};
  tail[0] = K.mass_relative ? (float)((m - K.base_mass) / K.mass_den) : (float)m;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float c = K.base_com[i];
    if (K.com_on) c = c + (float)(-1.0 + 2.0 * ((double)wc[i] * inv32)) * K.com_disp[i];
    tail[1 + i] = K.com_scaled ? c / K.com_div[i] : c;
  }
  if (K.priv_dim != 8) return;
  const double r = clampd((m - K.base_mass) / K.r_den, 0.0, 1.0);
  const double kd = K.couple_drag ? K.kdrag_min + r * (K.kdrag_max - K.kdrag_min) : 1.0;
  const double th = K.couple_thr ? clampd(1.0 - r * K.thr_rand, 1.0 - K.thr_rand, 1.0) : 1.0;
  const double kz = K.couple_kiz ? K.kiz_min + r * (K.kiz_max - K.kiz_min) : 1.0;
  float v[4] = {(float)kd, (float)th, (float)th, (float)kz};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = q == 0 ? 0 : (q == 3 ? 2 : 1);
    if (K.priv_mode == 1) {          // _encode_centered_priv_param
      v[q] = clampf(div_rn(v[q] - K.nominal, K.enc_r[j], K.inv_enc_r[j]), -1.f, 1.f);
    } else if (K.priv_mode == 2) {   // _encode_minmax_priv_param
      if (!K.enc_ok[j]) {
        v[q] = 0.f;
      } else {
        const float z = div_rn(v[q] - K.enc_lo[j], K.enc_r[j], K.inv_enc_r[j]);
        v[q] = clampf(2.0f * z - 1.0f, -1.f, 1.f);
      }
    }
    tail[4 + q] = v[q];
  }
}

TailK tail_constants(const usv_cfg_t &c, int mode) {
  TailK k{};
  k.mode = mode;
  k.priv_dim = c.priv_dim;
  k.priv_mode = c.priv_mode;
  k.mass_relative = c.mass_relative;
  k.com_scaled = c.com_scaled;
  k.com_on = c.com_mode == 1;
  k.couple_drag = c.couple_drag;
  k.couple_thr = c.couple_thr;
  k.couple_kiz = c.couple_kiz;
  k.mass_lo = (double)c.mass_min;
  k.mass_hi = (double)c.mass_max;
  if (k.mass_hi < k.mass_lo) {
    const double t = k.mass_lo;
    k.mass_lo = k.mass_hi;
    k.mass_hi = t;
  }
  k.base_mass = (double)c.base_mass;
  k.mass_den = std::fabs(k.base_mass) > 1e-6 ? std::fabs(k.base_mass) : 1e-6;
  k.r_den = k.mass_hi - k.base_mass > 1e-6 ? k.mass_hi - k.base_mass : 1e-6;
  k.kdrag_min = (double)c.kdrag_min;
  k.kdrag_max = (double)c.kdrag_max;
  k.thr_rand = (double)c.thr_rand;
  k.kiz_min = (double)c.kiz_min;
  k.kiz_max = (double)c.kiz_max;
  for (int i = 0; i < 3; ++i) {
    k.base_com[i] = c.base_com[i];
    k.com_disp[i] = c.com_disp[i];
    k.com_div[i] = c.com_scale[i] > 1e-6f ? c.com_scale[i] : 1e-6f;   // np.maximum(scale, 1e-6) in float32
  }
  k.nominal = c.priv_nominal;
  const float lo3[3] = {c.kdrag_min, c.thr_min, c.kiz_min}, hi3[3] = {c.kdrag_max, c.thr_max, c.kiz_max};
  for (int j = 0; j < 3; ++j) {
    k.enc_lo[j] = lo3[j];
    if (c.priv_mode == 1) {
      double sc = std::fabs((double)lo3[j] - (double)c.priv_nominal);
      const double hi = std::fabs((double)hi3[j] - (double)c.priv_nominal);
      if (hi > sc) sc = hi;
      if (1e-6 > sc) sc = 1e-6;
      k.enc_r[j] = (float)sc;
      k.enc_ok[j] = 1;
    } else {
      k.enc_r[j] = (float)((double)hi3[j] - (double)lo3[j]);
      k.enc_ok[j] = ((double)hi3[j] - (double)lo3[j]) > 1e-6;
    }
    k.inv_enc_r[j] = k.enc_r[j] != 0.f ? 1.0f / k.enc_r[j] : 0.f;
  }
  return k;
}

struct Rec {
  bool present;
  double reason, steps, ret, dist, min_obs;
};
__device__ __forceinline__ Rec record(const usv_eval_t &ev, int n, int K, long long p) {
  Rec r{};
  const int e = (int)(p / K), k = (int)(p % K);
  const int cnt = ev.ep_count[e];
  r.present = k < (cnt < K ? cnt : K);
  if (!r.present) return r;
  const size_t ncol = (size_t)ev.max_episodes * n;
  const double *col = ev.episodes + (size_t)k * n + e;
  r.reason = col[(size_t)USV_EV_REASON * ncol];
  r.steps = col[(size_t)USV_EV_LEN_STEPS * ncol];
  r.ret = col[(size_t)USV_EV_RETURN * ncol];
  r.dist = col[(size_t)USV_EV_DIST_TO_GOAL * ncol];
  r.min_obs = col[(size_t)USV_EV_MIN_OBS_EP * ncol];
  return r;
}

__global__ void __launch_bounds__(kCmpBlock)
k_cmp_fold(usv_eval_t a, usv_eval_t b, int n, int S, int R, int K, double thr, double *__restrict__ out) {
  const int s = blockIdx.x * kCmpBlock + threadIdx.x;
  if (s >= S) return;
  double pairs = 0.0, both = 0.0, only_a = 0.0, only_b = 0.0, neither = 0.0, coll_a = 0.0, coll_b = 0.0, oob_a = 0.0,
         oob_b = 0.0, n_steps = 0.0, d_steps = 0.0, d_ret = 0.0, d_dist = 0.0, n_margin = 0.0, d_margin = 0.0;
#pragma unroll 1
  for (int r = 0; r < R; ++r) {
    const long long p = (long long)s * R + r;
    const Rec ra = record(a, n, K, p), rb = record(b, n, K, p);
    if (!ra.present || !rb.present) continue;
    const bool sa = ra.reason == (double)USV_EV_REASON_GOAL, sb = rb.reason == (double)USV_EV_REASON_GOAL;
    pairs += 1.0;
    both += sa && sb ? 1.0 : 0.0;
    only_a += sa && !sb ? 1.0 : 0.0;
    only_b += sb && !sa ? 1.0 : 0.0;
    neither += !sa && !sb ? 1.0 : 0.0;
    coll_a += ra.reason == (double)USV_EV_REASON_COLLISION ? 1.0 : 0.0;
    coll_b += rb.reason == (double)USV_EV_REASON_COLLISION ? 1.0 : 0.0;
    oob_a += ra.reason == (double)USV_EV_REASON_OOB ? 1.0 : 0.0;
    oob_b += rb.reason == (double)USV_EV_REASON_OOB ? 1.0 : 0.0;
    if (sa && sb) {
      n_steps += 1.0;
      d_steps += rb.steps - ra.steps;
    }
    d_ret += rb.ret - ra.ret;
    d_dist += rb.dist - ra.dist;
    if (isfinite(ra.min_obs) && isfinite(rb.min_obs)) {
      n_margin += 1.0;
      d_margin += (rb.min_obs - thr) - (ra.min_obs - thr);
    }
  }
  double *o = out + s;
  const size_t st = (size_t)S;
  o[USV_CMP_PAIRS * st] = pairs;
  o[USV_CMP_BOTH_SUCC * st] = both;
  o[USV_CMP_ONLY_A * st] = only_a;
  o[USV_CMP_ONLY_B * st] = only_b;
  o[USV_CMP_NEITHER * st] = neither;
  o[USV_CMP_COLL_A * st] = coll_a;
  o[USV_CMP_COLL_B * st] = coll_b;
  o[USV_CMP_OOB_A * st] = oob_a;
  o[USV_CMP_OOB_B * st] = oob_b;
  o[USV_CMP_D_STEPS * st] = d_steps / n_steps;   // 0 / 0 = NaN without a pair that succeeds in both
  o[USV_CMP_D_RETURN * st] = d_ret / pairs;
  o[USV_CMP_D_FINAL_DIST * st] = d_dist / pairs;
  o[USV_CMP_D_MIN_MARGIN * st] = d_margin / n_margin;
}

}  // namespace

extern "C" {

int usv_priv_tail(const usv_cfg_t *cfg, int mode, const float *obs_in, float *obs_out, int n, int obs_dim,
                  const float *const_tail, const int32_t *episode, uint64_t seed, void *stream) {
  if (!cfg || !obs_in || !obs_out || n <= 0) return 1;
  if (mode != USV_PT_CONST && mode != USV_PT_WRONG_RANDOM) return 1;
  if (mode == USV_PT_CONST && !const_tail) return 1;
  if ((cfg->priv_dim != 4 && cfg->priv_dim != 8) || obs_dim < cfg->priv_dim) return 2;
  if ((long long)n * obs_dim > 0x7FFFFFFFLL) return 2;
  if (mode == USV_PT_WRONG_RANDOM && cfg->com_mode == 2 && cfg->com_legacy_r > 0.f) return 2;
  hipLaunchKernelGGL(k_priv_tail, dim3((unsigned)((n + kCmpBlock - 1) / kCmpBlock)), dim3(kCmpBlock), 0,
                     (hipStream_t)stream, tail_constants(*cfg, mode), obs_in, obs_out, n, obs_dim, const_tail, episode,
                     seed);
  USV_CHECK_LAUNCH();
  return 0;
}

int usv_cmp_fold(const usv_eval_t *a, const usv_eval_t *b, int n, int S, int R, int K, double collision_threshold,
                 double *out, void *stream) {
  if (!a || !b || !out || !a->episodes || !a->ep_count || !b->episodes || !b->ep_count || n <= 0 || S <= 0 ||
      R <= 0 || K <= 0)
    return 1;
  const long long rows = (long long)S * R;
  if (S > USV_SCN_MAX_COUNT || rows > 0x7FFFFFFFLL || (long long)K != (rows + n - 1) / n || K > a->max_episodes ||
      a->max_episodes != b->max_episodes || (long long)a->max_episodes * n > 0x7FFFFFFFLL)
    return 2;
  hipLaunchKernelGGL(k_cmp_fold, dim3((unsigned)((S + kCmpBlock - 1) / kCmpBlock)), dim3(kCmpBlock), 0,
                     (hipStream_t)stream, *a, *b, n, S, R, K, collision_threshold, out);
  USV_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
