// Scenario tables for MI355X (gfx950): candidate mining and the teacher filter's per-scenario aggregate, the
// stages the reference runs one scenario at a time on the host (scripts/build_usv_scenario_table.py: sampling
// :153-209, _compute_metrics :215-258; scripts/teacher_filter_scenario_table.py: aggregate :712-759, verdict and
// difficulty :512-552).
//
// Generate and metrics: one scenario per 16-lane group, one obstacle per lane, four scenarios per wave.  What a
// group shares (any obstacle still invalid, the minima over its obstacles) moves by ballot and 16-wide shuffles:
// no LDS, no atomics.  Fold: one thread per scenario over the evaluator's table, double sums in rollout order.
// The arithmetic is written operation by operation in the reference's precisions (the build has
// -ffp-contract=off): float32 differences, products, two-term sums, correctly rounded sqrtf and division.
#include "usv_device.h"

#include <cmath>

namespace {

constexpr int kScnBlock = 256;
constexpr int kScnGroup = USV_NOBST;                // lanes per scenario
constexpr int kScnPerBlock = kScnBlock / kScnGroup;
static_assert(USV_NOBST == 16, "16-lane groups, one obstacle per lane");
static_assert(USV_SC_OBST == 0 && USV_SC_GOAL + 2 < USV_SCENE_STRIDE, "scene row layout");

constexpr double kTwoPi = 6.283185307179586;   // 2.0 * math.pi
constexpr double kPi = 3.141592653589793;

__device__ __forceinline__ double scn_u(uint32_t w) { return (double)w * (1.0 / 4294967296.0); }
// numpy's uniform: low + (high - low) * u in double, then one rounding to float32
__device__ __forceinline__ float scn_val(double lo, double hi, double u) { return (float)(lo + (hi - lo) * u); }
// np.linalg.norm of a float32 2-vector: sqrt(fl(fl(dx dx) + fl(dy dy)))
__device__ __forceinline__ float scn_norm(float dx, float dy) { return sqrtf(dx * dx + dy * dy); }
__device__ __forceinline__ float scn_min(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float group_min(float v) {
#pragma unroll
  for (int m = 1; m < kScnGroup; m <<= 1) v = scn_min(v, __shfl_xor(v, m, kScnGroup));
  return v;
}

__global__ void __launch_bounds__(kScnBlock)
k_scn_generate(uint64_t seed, long long first, int count, double goal_rand, double rmin, double rmax, double box,
               double safe, int max_iters, int vel_mode, float *__restrict__ rows, float *__restrict__ quat) {
  const int o = threadIdx.x & (kScnGroup - 1), gbase = threadIdx.x & 48;
  const long long idx = (long long)blockIdx.x * kScnPerBlock + (threadIdx.x >> 4);
  const bool live = idx < (long long)count;   // a group past the end runs along (it shares the wave's ballots)
  const uint64_t cand = (uint64_t)(first + idx);
  const uint32_t c0 = (uint32_t)cand, c1 = (uint32_t)(cand >> 32);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const u32x4 p = philox4x32_10(u32x4{c0, c1, 0u, (uint32_t)USV_SCN_SITE_POSE}, k0, k1);
  const float tx = scn_val(-goal_rand, goal_rand, scn_u(p.x));
  const float ty = scn_val(-goal_rand, goal_rand, scn_u(p.y));
  const double r = rmin + (rmax - rmin) * scn_u(p.z);
  const double th = kTwoPi * scn_u(p.w);
  const float sx = (float)(r * cos(th)), sy = (float)(r * sin(th));
  const float boxf = (float)box, safef = (float)safe;
  const double mnx = (double)(tx - boxf), mny = (double)(ty - boxf);
  const double mxx = (double)(tx + boxf), mxy = (double)(ty + boxf);
  float ox, oy;
  auto draw = [&](uint32_t k) {
    const u32x4 w = philox4x32_10(u32x4{c0, c1, k, (uint32_t)(USV_SCN_SITE_OBST + o)}, k0, k1);
    ox = scn_val(mnx, mxx, scn_u(w.x));
    oy = scn_val(mny, mxy, scn_u(w.y));
  };
  auto invalid = [&]() { return scn_norm(ox - sx, oy - sy) < safef || scn_norm(ox - tx, oy - ty) < safef; };
  draw(0u);
  for (int k = 1; k <= max_iters; ++k) {
    const bool bad = invalid();
    if (((__ballot(bad) >> gbase) & 0xFFFFull) == 0ull) break;   // the same in all 16 lanes of the group
    if (bad) draw((uint32_t)k);
  }
  if (invalid()) ox = oy = 999.0f;
  if (!live) return;
  float *row = rows + (size_t)idx * USV_SCENE_STRIDE;
  row[USV_SC_OBST + 2 * o] = ox;
  row[USV_SC_OBST + 2 * o + 1] = oy;
  if (o != 0) return;
  const u32x4 y4 = philox4x32_10(u32x4{c0, c1, 0u, (uint32_t)USV_SCN_SITE_YAW}, k0, k1);
  const double yaw = kPi * scn_u(y4.x);
  row[USV_SC_START] = sx;
  row[USV_SC_START + 1] = sy;
  row[USV_SC_YAW] = (float)yaw;
  row[USV_SC_VEL] = vel_mode ? scn_val(-1.5, 1.5, scn_u(y4.y)) : 0.0f;
  row[USV_SC_VEL + 1] = vel_mode ? scn_val(-1.5, 1.5, scn_u(y4.z)) : 0.0f;
  row[USV_SC_GOAL] = tx;
  row[USV_SC_GOAL + 1] = ty;
  for (int q = USV_SC_GOAL + 2; q < USV_SCENE_STRIDE; ++q) row[q] = 0.0f;
  float *qt = quat + (size_t)idx * 4;
  qt[0] = (float)cos(yaw * 0.5);
  qt[1] = 0.0f;
  qt[2] = 0.0f;
  qt[3] = (float)sin(yaw * 0.5);
}

__global__ void __launch_bounds__(kScnBlock)
k_scn_metrics(const float *__restrict__ rows, int S, double radius, double limbo, float *__restrict__ out) {
  const int o = threadIdx.x & (kScnGroup - 1);
  const long long idx = (long long)blockIdx.x * kScnPerBlock + (threadIdx.x >> 4);
  const bool live = idx < (long long)S;
  const float *row = rows + (size_t)(live ? idx : (long long)S - 1) * USV_SCENE_STRIDE;   // a group past the end
  const float ox = row[USV_SC_OBST + 2 * o], oy = row[USV_SC_OBST + 2 * o + 1];           // re-reads the last row
  const float sx = row[USV_SC_START], sy = row[USV_SC_START + 1];
  const float gx = row[USV_SC_GOAL], gy = row[USV_SC_GOAL + 1];
  const float limf = (float)limbo;
  const bool valid = fabsf(ox) < limf && fabsf(oy) < limf;
  const float apx = ox - sx, apy = oy - sy;
  float d_s = INFINITY, d_g = INFINITY, d_c = INFINITY, d_o = INFINITY;
  if (valid) {
    d_s = scn_norm(apx, apy);
    d_g = scn_norm(ox - gx, oy - gy);
    // _point_to_segment_distance(o, s, g)
    const float abx = gx - sx, aby = gy - sy;
    const float ab2 = abx * abx + aby * aby;
    if ((double)ab2 <= 1e-12) {
      d_c = d_s;
    } else {
      float t = (apx * abx + apy * aby) / ab2;
      t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);   // max(0.0, min(1.0, t))
      const float prx = sx + t * abx, pry = sy + t * aby;
      d_c = scn_norm(ox - prx, oy - pry);
    }
  }
  // the 120 pairs: lane o meets lanes o + 1 .. o + 8 (mod 16); every pair is met once (distance 8: twice)
#pragma unroll
  for (int d = 1; d <= kScnGroup / 2; ++d) {
    const int j = (o + d) & (kScnGroup - 1);
    const float xj = __shfl(ox, j, kScnGroup), yj = __shfl(oy, j, kScnGroup);
    const int vj = __shfl((int)valid, j, kScnGroup);
    if (valid && vj) d_o = scn_min(d_o, scn_norm(ox - xj, oy - yj));
  }
  d_s = group_min(d_s);
  d_g = group_min(d_g);
  d_c = group_min(d_c);
  d_o = group_min(d_o);
  if (!live || o != 0) return;
  // np.float32 - Python float is float32; the corridor and pair distances are Python floats by then (doubles)
  const float radf = (float)radius;
  const float v_s = d_s - radf, v_g = d_g - radf;
  const float v_c = (float)((double)d_c - radius);
  const float v_o = (float)((double)d_o - 2.0 * radius);
  const size_t s = (size_t)S;
  out[USV_SCM_D_SPAWN * s + idx] = v_s;
  out[USV_SCM_D_GOAL * s + idx] = v_g;
  out[USV_SCM_D_CORR * s + idx] = v_c;
  out[USV_SCM_D_OO * s + idx] = v_o;
  out[USV_SCM_DENSITY * s + idx] = scn_min(scn_min(v_s, v_g), v_c);
}

__global__ void __launch_bounds__(kScnBlock)
k_scn_fold(usv_eval_t ev, int n, int S, int R, int K, double thr, int easy_steps, double easy_margin, int max_steps,
           double *__restrict__ out) {
  const int s = blockIdx.x * kScnBlock + threadIdx.x;
  if (s >= S) return;
  const size_t ncol = (size_t)ev.max_episodes * n;
  double present = 0.0, succ = 0.0, coll = 0.0, oob = 0.0, steps = 0.0, ret = 0.0, dist = 0.0;
  double min_obs = (double)INFINITY, min_margin = (double)INFINITY;
#pragma unroll 1
  for (int r = 0; r < R; ++r) {
    const long long p = (long long)s * R + r;
    const int e = (int)(p / K), k = (int)(p % K);
    const int cnt = ev.ep_count[e];
    if (k >= (cnt < K ? cnt : K)) continue;
    const double *col = ev.episodes + (size_t)k * n + e;
    const double reason = col[(size_t)USV_EV_REASON * ncol];
    present += 1.0;
    succ += reason == (double)USV_EV_REASON_GOAL ? 1.0 : 0.0;
    coll += reason == (double)USV_EV_REASON_COLLISION ? 1.0 : 0.0;
    oob += reason == (double)USV_EV_REASON_OOB ? 1.0 : 0.0;
    steps += col[(size_t)USV_EV_LEN_STEPS * ncol];
    ret += col[(size_t)USV_EV_RETURN * ncol];
    dist += col[(size_t)USV_EV_DIST_TO_GOAL * ncol];
    const double mo = col[(size_t)USV_EV_MIN_OBS_EP * ncol];
    if (isfinite(mo)) {   // :464-467
      min_obs = mo < min_obs ? mo : min_obs;
      const double mg = mo - thr;
      min_margin = mg < min_margin ? mg : min_margin;
    }
  }
  const double success_rate = succ / present;   // 0 / 0 = NaN for a scenario without a record
  const bool coll_any = coll > 0.0, oob_any = oob > 0.0;
  const int reason = coll_any ? USV_EV_REASON_COLLISION
                   : oob_any ? USV_EV_REASON_OOB
                   : success_rate >= 1.0 - 1e-9 ? USV_EV_REASON_GOAL
                   : success_rate > 0.0 ? USV_EV_REASON_MIXED : USV_EV_REASON_OTHER;
  const double steps_i = trunc(steps / present);
  int verdict;
  if (present < (double)R) verdict = USV_SCV_INCOMPLETE;
  else if (coll_any || oob_any || !(success_rate > 0.0)) verdict = USV_SCV_HARD_REJECT;
  else if (steps_i <= (double)easy_steps && min_margin >= easy_margin) verdict = USV_SCV_EASY_REJECT;
  else verdict = USV_SCV_KEEP;
  const double tight = (0.5 - min_margin) / 0.5;
  const double tight_c = tight < -2.0 ? -2.0 : (tight > 2.0 ? 2.0 : tight);
  const double ms = (double)max_steps > 1.0 ? (double)max_steps : 1.0;
  double *o = out + s;
  const size_t st = (size_t)S;
  o[USV_SCF_PRESENT * st] = present;
  o[USV_SCF_SUCCESS_RATE * st] = success_rate;
  o[USV_SCF_COLL_RATE * st] = coll / present;
  o[USV_SCF_OOB_RATE * st] = oob / present;
  o[USV_SCF_COLL_ANY * st] = coll_any ? 1.0 : 0.0;
  o[USV_SCF_OOB_ANY * st] = oob_any ? 1.0 : 0.0;
  o[USV_SCF_REASON * st] = (double)reason;
  o[USV_SCF_STEPS * st] = steps_i;
  o[USV_SCF_RETURN * st] = ret / present;
  o[USV_SCF_FINAL_DIST * st] = dist / present;
  o[USV_SCF_MIN_OBS * st] = min_obs;
  o[USV_SCF_MIN_MARGIN * st] = min_margin;
  o[USV_SCF_VERDICT * st] = (double)verdict;
  o[USV_SCF_DIFFICULTY * st] = steps_i / ms + 0.3 * tight_c;
}

}  // namespace

extern "C" {

int usv_scn_generate(uint64_t seed, int64_t first, int count, double goal_random_position, double min_spawn_dist,
                     double max_spawn_dist, double box_half_range, double min_dist_safe, int max_iterations,
                     int init_vel_mode, float *rows, float *spawn_quat, void *stream) {
  if (!rows || !spawn_quat || count <= 0 || first < 0) return 1;
  if (count > USV_SCN_MAX_COUNT || max_iterations < 0 || max_iterations > USV_SCN_MAX_ITERS ||
      (init_vel_mode != 0 && init_vel_mode != 1))
    return 2;
  hipLaunchKernelGGL(k_scn_generate, dim3((unsigned)((count + kScnPerBlock - 1) / kScnPerBlock)), dim3(kScnBlock), 0,
                     (hipStream_t)stream, seed, (long long)first, count, goal_random_position, min_spawn_dist,
                     max_spawn_dist, box_half_range, min_dist_safe, max_iterations, init_vel_mode, rows, spawn_quat);
  USV_CHECK_LAUNCH();
  return 0;
}

int usv_scn_metrics(const float *rows, int S, double obstacle_radius, double limbo_threshold, float *out,
                    void *stream) {
  if (!rows || !out || S <= 0) return 1;
  if (S > USV_SCN_MAX_COUNT) return 2;
  hipLaunchKernelGGL(k_scn_metrics, dim3((unsigned)((S + kScnPerBlock - 1) / kScnPerBlock)), dim3(kScnBlock), 0,
                     (hipStream_t)stream, rows, S, obstacle_radius, limbo_threshold, out);
  USV_CHECK_LAUNCH();
  return 0;
}

int usv_scn_fold(const usv_eval_t *ev, int n, int S, int R, int K, double collision_threshold, int easy_steps_max,
                 double easy_margin_min, int max_steps, double *out, void *stream) {
  if (!ev || !out || !ev->episodes || !ev->ep_count || n <= 0 || S <= 0 || R <= 0 || K <= 0) return 1;
  const long long rows = (long long)S * R;
  if (S > USV_SCN_MAX_COUNT || rows > 0x7FFFFFFFLL || (long long)K != (rows + n - 1) / n || K > ev->max_episodes ||
      (long long)ev->max_episodes * n > 0x7FFFFFFFLL)
    return 2;
  hipLaunchKernelGGL(k_scn_fold, dim3((unsigned)((S + kScnBlock - 1) / kScnBlock)), dim3(kScnBlock), 0,
                     (hipStream_t)stream, *ev, n, S, R, K, collision_threshold, easy_steps_max, easy_margin_min,
                     max_steps, out);
  USV_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
