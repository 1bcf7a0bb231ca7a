// USV CaptureXY env hot path for MI355X (gfx950): thruster LUT, reset path
// (compaction + domain randomisation + spawn/obstacle rejection sampling) and
// the fused control step (action mapping, 10 substeps of 3-DoF hydrodynamics
// with semi-implicit Euler, observation, reward, penalties, kills, stats).
//
// One thread per env, struct-of-arrays state in HBM: every per-env field is a
// coalesced 4-byte-per-lane stream.  The step kernel keeps the 10 substeps in
// registers (state is read once and written once per control step).
//
// Reference call chains replaced (loop-Z/omniisaacgymenvs_loop):
//   envs/vec_env_rlgames.py:120-217          VecEnvRLGames.step
//   tasks/USV_Virtual.py:1042-1133            pre_physics_step, apply_forces
//   tasks/USV_Virtual.py:771-986              update_state, get_observations
//   tasks/USV_Virtual.py:1223-1237,1628-1652  is_done, calculate_metrics
//   tasks/USV_Virtual.py:1502-1618            reset_idx
//   tasks/USV/USV_capture_xy_static_obs.py    get_state_observations, compute_reward,
//                                             update_kills, get_spawns, get_goals
//   envs/USV/{Hydrodynamics,ThrusterDynamics}.py  damping + thruster LUT/lag
// The rigid-body integrator replaces PhysX (no reference implementation).
#include "usv_device.h"
#include "usv_layout_gen.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>

namespace {

constexpr int kBlock = 256;

// ------------------------------------------------------------------------
// Thruster LUT: F.interpolate(linear, align_corners=True) 21 -> 1000 points
// (ThrusterDynamics.py:152-177).  The CPU build of the reference contracts
// l0*t[i0] + l1*t[i1] into fma(l0, t[i0], l1*t[i1]).
// ------------------------------------------------------------------------
__global__ void k_build_lut(const float *__restrict__ tl, const float *__restrict__ tr, int n_in,
                            float *__restrict__ lut) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= USV_LUT_N) return;
  const float scale = (float)(n_in - 1) / (float)(USV_LUT_N - 1);
  const float src = scale * (float)i;
  int i0 = (int)src;
  if (i0 > n_in - 1) i0 = n_in - 1;
  const int off = (i0 < n_in - 1) ? 1 : 0;
  const float l1 = src - (float)i0;
  const float l0 = 1.0f - l1;
  lut[i] = fmaf(l0, tl[i0], l1 * tl[i0 + off]);
  lut[USV_LUT_N + i] = fmaf(l0, tr[i0], l1 * tr[i0 + off]);
}

// step index / action bias of this step: the device clock when present
__device__ __forceinline__ uint64_t step_of(const usv_bufs_t &b, uint64_t step) { return b.clock ? b.clock[2] : step; }
// USVVirtual.step at this step's reset (which = 4) or after its calculate_metrics (which = 5); without the device
// clock, from the step index (exact for power-of-two horizons)
__device__ __forceinline__ double ref_step_of(const usv_cfg_t &c, const usv_bufs_t &b, uint64_t step, int which) {
  if (b.clock) return __longlong_as_double((long long)b.clock[which]);
  return (double)(step + (which == 5 ? 1 : 0)) * c.step_inc;
}
// GoToPoseTask's spawn curriculum (USV_go_to_pose.py:266-290 radii, :188-202 kill distance): linear in the
// reference step between warmup and end, in the reference's double arithmetic
__device__ __forceinline__ double curriculum_lerp(const usv_cfg_t &c, double st, double cur, double fin) {
  if (st < c.cur_warmup) return cur;
  if (st > c.cur_end) return fin;
  const double r = (st - c.cur_warmup) / (c.cur_end - c.cur_warmup);
  return r * (fin - cur) + cur;
}
__device__ __forceinline__ float bias_of(const usv_cfg_t &c, const usv_bufs_t &b, float bias) {
  if (!b.clock) return bias;
  return (c.act_bias_steps > 0 && b.clock[3] < (uint64_t)c.act_bias_steps) ? c.act_bias : 0.f;
}

// reset-slot uniform i of env e (injected row e, or Philox site 0x100)
struct ResetRng {
  const float *inj;
  uint64_t seed, step;
  uint32_t env;
  int cached_blk = -1;
  float buf[4];
  __device__ float operator()(int i) {
    if (inj) return inj[(size_t)env * USV_NU_RESET + i];
    const int blk = i >> 2;
    if (blk != cached_blk) {
      philox_u4(seed, env, step, 0x100u + (uint32_t)blk, buf);
      cached_blk = blk;
    }
    return buf[i & 3];
  }
};

// ------------------------------------------------------------------------
// Per-step scratch reset (reset count, field maxima, extras sums): one tiny
// kernel instead of four memset nodes.
// ------------------------------------------------------------------------
__global__ void k_step_begin(usv_bufs_t b, double step_inc) {
  const int t = threadIdx.x;
  if (t == 0 && b.clock) {   // device step clock: this step's index and bias-call count
    b.clock[2] = b.clock[0]++;
    b.clock[3] = b.clock[1]++;
    // USVVirtual.step (a double, += 1 / horizon_length per calculate_metrics, USV_Virtual.py:1633): its value
    // at this step's reset_idx and after this step's calculate_metrics, accumulated as the reference does
    const uint64_t after = b.clock[5];
    b.clock[4] = after;
    b.clock[5] = (uint64_t)__double_as_longlong(__longlong_as_double((long long)after) + step_inc);
  }
  if (t == 0) b.ctl[USV_CTL_RESET_COUNT] = 0;
  if (t == 3 && b.ctl[USV_CTL_STEPPED]) {   // a step has run: prev_* are no longer None
    b.ctl[USV_CTL_POT_VALID] = 1;
    b.ctl[USV_CTL_PEN_VALID] = 1;
    b.ctl[USV_CTL_REW_VALID] = 1;
  }
  if (t == 1) b.ctl[USV_CTL_ANY_INSIDE] = 0;
  if (t == 2) b.ctl[USV_CTL_ANY_FINITE] = 0;
  if (t < 4) b.fscratch[t] = 0.f;
  // completion counters of this step's kernels: their last workgroup also returns them to 0,
  // but a step never depends on that (a counter left non-zero by an aborted launch would
  // otherwise make every later "last workgroup" test fail silently)
  if (t == 4) b.ctl[USV_CTL_OBST_DONE] = 0;
  if (t == 5) b.ctl[USV_CTL_BATCH_DONE] = 0;
}

// ------------------------------------------------------------------------
// Reset path (USVVirtual.reset_idx, USV_Virtual.py:1502-1618).  One thread per
// env; threads of envs with reset_buf==1 do the work.  The reset list is
// compacted with a wave ballot + one atomic per wave (order is irrelevant:
// draws are keyed by env id, the potential-field batch statistics are maxima).
// Obstacle rejection sampling follows in the same kernel, one whole wave per
// reset env (place_obstacles).
// ------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_reset(usv_cfg_t c, usv_bufs_t b, uint64_t seed, uint64_t step,
                                                  const float *__restrict__ inj) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = b.n;
  const bool active = (e < n) && (b.reset_buf[e] != 0);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  // episode-extras sums of this workgroup's resetting envs, per wave (fixed order)
  __shared__ float wsum[kBlock / 64][USV_NSTAT];
  step = step_of(b, step);
  // ---- compaction: reset_buf.nonzero() (USV_Virtual.py:1045): wave ballots, a workgroup
  // prefix in LDS and one atomic per workgroup (slots are workgroup-contiguous) ----
  const uint64_t mask = __ballot(active);
  __shared__ int wbase[kBlock / 64];
  if (lane == 0) wbase[wid] = __popcll(mask);
  if (c.stats_on && mask == 0 && lane < USV_NSTAT) wsum[wid][lane] = 0.f;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) { const int k = wbase[w]; wbase[w] = tot; tot += k; }
    const int base0 = tot ? atomicAdd(&b.ctl[USV_CTL_RESET_COUNT], tot) : 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) wbase[w] += base0;
  }
  __syncthreads();
  if (mask != 0) {
    const int leader = __ffsll((long long)mask) - 1;
    const int base = wbase[wid];
    // ---- episode extras: sums of the envs being reset (:1591-1612): wave sums here, the
    // workgroup's partial at the end, folded in workgroup order by the last workgroup ----
    if (c.stats_on) {
      // all 28 loads first, then 28 independent wave sums (their shuffles interleave)
      const int ec = min(e, n - 1);
      float v[USV_NSTAT];
#pragma unroll
      for (int q = 0; q < USV_NSTAT; ++q) v[q] = b.stats[(size_t)q * n + ec];
      v[ST_SUCCESS] = (float)b.done_succ[ec];
      v[ST_COLLISION] = (float)b.done_coll[ec];
      if (active) {
#pragma unroll
        for (int q = 0; q < USV_NSTAT; ++q) b.stats[(size_t)q * n + e] = 0.f;
      }
#pragma unroll
      for (int q = 0; q < USV_NSTAT; ++q) v[q] = wave_sum(active ? v[q] : 0.f);
      if (lane == leader) {
#pragma unroll
        for (int q = 0; q < USV_NSTAT; ++q) wsum[wid][q] = v[q];
      }
    }
    float sx = 0.f, sy = 0.f, tx = 0.f, ty = 0.f;
    if (active) {
      const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
      b.reset_ids[slot] = e;
      ResetRng U{inj, seed, step, (uint32_t)e};
      // ---- CaptureXYTask.reset (static_obs.py:767-778) ----
      b.goal_cnt[e] = 0;
      b.done_succ[e] = 0;
      b.done_coll[e] = 0;
      b.just_reset[e] = 1;
      // ---- MassDistributionDisturbances.randomize_masses / _randomize_com (USV_disturbances.py:94-150) ----
      float mass;
      if (c.mass_dr_on) mass = U(RU_MASS) * (float)((double)c.mass_max - (double)c.mass_min) + c.mass_min;
      else mass = U(RU_MASS) * 0.0f + c.base_mass;
      float cx = c.base_com[0], cy = c.base_com[1], cz = c.base_com[2];
      if (c.mass_dr_on && c.com_mode == 1) {
        cx = c.base_com[0] + (U(RU_COM + 0) * 2.0f - 1.0f) * c.com_disp[0];
        cy = c.base_com[1] + (U(RU_COM + 1) * 2.0f - 1.0f) * c.com_disp[1];
        cz = c.base_com[2] + (U(RU_COM + 2) * 2.0f - 1.0f) * c.com_disp[2];
      } else if (c.mass_dr_on && c.com_mode == 2 && c.com_legacy_r > 0.f) {
        const float r = U(RU_COM) * c.com_legacy_r;
        const float th = U(RU_COM + 1) * USV_PI_F * 2.0f;
        float sth, cth;
        usv_sincos_cr(th, &sth, &cth);
        cx = c.base_com[0] + cth * r;
        cy = c.base_com[1] + sth * r;
      }
      b.mass[e] = mass;
      b.com_x[e] = cx;
      b.com_y[e] = cy;
      b.com_z[e] = cz;
      // ---- independent randomisations (yaw inertia :193-240, drag :136-174, thrusters :112-127) ----
      if (c.indep_kiz_on && !c.couple_kiz) {
        const float u = U(RU_KIZ);
        b.k_iz[e] = c.kiz_log ? expf(logf(c.kiz_min) + u * (logf(c.kiz_max) - logf(c.kiz_min)))
                              : c.kiz_min + u * (c.kiz_max - c.kiz_min);
      }
      if (c.drag_rand_on && b.lin_damp) {
        for (int a = 0; a < 3; ++a) {
          b.lin_damp[(size_t)a * n + e] = c.lin_damp[a] + (U(RU_DRAG + a) * 2.0f - 1.0f) * c.lin_rand[a];
          b.quad_damp[(size_t)a * n + e] = c.quad_damp[a] + (U(RU_DRAG + 6 + a) * 2.0f - 1.0f) * c.quad_rand[a];
        }
      }
      if (c.indep_kdrag_on) {
        const float u = U(RU_KDRAG);
        b.k_drag[e] = c.kdrag_log ? expf(logf(c.kdrag_min) + u * (logf(c.kdrag_max) - logf(c.kdrag_min)))
                                  : c.kdrag_min + u * (c.kdrag_max - c.kdrag_min);
      }
      if (c.indep_thr_on) {
        if (c.thr_separate) {
          b.thr_l[e] = U(RU_THR) * 2.0f * c.left_rand + (1.0f - c.left_rand);
          b.thr_r[e] = U(RU_THR + 1) * 2.0f * c.right_rand + (1.0f - c.right_rand);
        } else {
          const float m = U(RU_THR) * 2.0f * c.thr_rand + (1.0f - c.thr_rand);
          b.thr_l[e] = m;
          b.thr_r[e] = m;
        }
      }
      // ---- ForceDisturbance.generate_force / TorqueDisturbance.generate_torque
      // (USV_disturbances.py:327-508, called from reset_idx:1517-1518) ----
      if (b.dist) {
        float *D = b.dist;
        const size_t nn = (size_t)n;
        if (c.fdist_on && c.fsin_on) {
          const float fr_ = (float)((double)c.ffreq_max - (double)c.ffreq_min);
          const float sr_ = (float)((double)c.fshift_max - (double)c.fshift_min);
          D[DI_FXF * nn + e] = U(RU_FSIN) * fr_ + c.ffreq_min;
          D[DI_FYF * nn + e] = U(RU_FSIN + 1) * fr_ + c.ffreq_min;
          D[DI_FXS * nn + e] = U(RU_FSIN + 2) * sr_ + c.fshift_min;
          D[DI_FYS * nn + e] = U(RU_FSIN + 3) * sr_ + c.fshift_min;
          D[DI_FAMP * nn + e] = U(RU_FSIN + 4) * (float)((double)c.fsin_max - (double)c.fsin_min) + c.fsin_min;
        }
        if (c.fdist_on && c.fconst_on) {
          const float r = U(RU_FCONST) * (float)((double)c.fconst_max - (double)c.fconst_min) + c.fconst_min;
          const float th = U(RU_FCONST + 1) * USV_PI_F * 2.0f;
          float sth, cth;
          usv_sincos_cr(th, &sth, &cth);
          if (c.inj_trig && inj) { cth = U(RU_TRIG + 4); sth = U(RU_TRIG + 5); }
          D[DI_FCX * nn + e] = cth * r;
          D[DI_FCY * nn + e] = sth * r;
        }
        if (c.tdist_on && c.tsin_on) {
          D[DI_TF * nn + e] = U(RU_TSIN) * (float)((double)c.tfreq_max - (double)c.tfreq_min) + c.tfreq_min;
          D[DI_TS * nn + e] = U(RU_TSIN + 1) * (float)((double)c.tshift_max - (double)c.tshift_min) + c.tshift_min;
          D[DI_TAMP * nn + e] = U(RU_TSIN + 2) * (float)((double)c.tsin_max - (double)c.tsin_min) + c.tsin_min;
        }
        if (c.tdist_on && c.tconst_on) {
          float r = U(RU_TCONST) * (float)((double)c.tconst_max - (double)c.tconst_min) + c.tconst_min;
          if (U(RU_TCONST + 1) > 0.5f) r = r * -1.0f;   // half of the envs at random (:505-507)
          D[DI_TC * nn + e] = r;
        }
      }
      // ---- _apply_mass_driven_coupling (USV_Virtual.py:988-1040) ----
      if (c.couple_drag || c.couple_thr || c.couple_kiz) {
        const double den_d = (double)c.mass_max - (double)c.base_mass;
        const float den = (float)(den_d > 1e-6 ? den_d : 1e-6);
        const float r = clampt((mass - c.base_mass) / den, 0.f, 1.f);
        b.mass_r[e] = r;
        if (c.couple_drag) b.k_drag[e] = c.kdrag_min + r * (float)((double)c.kdrag_max - (double)c.kdrag_min);
        if (c.couple_thr) {
          const float s = clampt(1.0f - r * c.thr_rand, (float)(1.0 - (double)c.thr_rand), 1.0f);
          b.thr_l[e] = s;
          b.thr_r[e] = s;
        }
        if (c.couple_kiz) b.k_iz[e] = c.kiz_min + r * (float)((double)c.kiz_max - (double)c.kiz_min);
      }
      // ---- task.get_spawns, previous-episode target (get_goals runs later, USV_Virtual.py:1618) ----
      tx = b.tgt_x[e];
      ty = b.tgt_y[e];
      // the spawn heading reaches the stand-in as the quaternion (cos(yaw0 / 2), 0, 0, sin(yaw0 / 2))
      // (static_obs.py:959-961) and set_world_poses turns it into its yaw (usv_yaw_of_quat)
      const bool inj_trig = c.inj_trig && inj;   // parity tests: the reference's recorded torch.cos / sin values
      float qz0, qw0;
      usv_sincos_cr(U(RU_YAW) * USV_PI_F * 0.5f, &qz0, &qw0);
      if (inj_trig) { qw0 = U(RU_TRIG + 2); qz0 = U(RU_TRIG + 3); }
      const float yaw0 = usv_yaw_of_quat(qw0, qz0);
      if (c.task_kind == USV_TASK_CAPTURE_XY) {   // CaptureXYTask.get_spawns (static_obs.py:936-1060)
        const float r = U(RU_SPAWN_R) * (c.spawn_rmax - c.spawn_rmin) + c.spawn_rmin;
        const float th = U(RU_SPAWN_TH) * 2.0f * USV_PI_F;
        float sth, cth;
        usv_sincos_cr(th, &sth, &cth);
        if (inj_trig) { cth = U(RU_TRIG); sth = U(RU_TRIG + 1); }
        sx = r * cth;
        sy = r * sth;
        b.field_old_tgt[e] = tx;
        b.field_old_tgt[n + e] = ty;
      } else if (c.task_kind == USV_TASK_GO_TO_POSE || c.task_kind == USV_TASK_GO_TO_XY ||
                 c.task_kind == USV_TASK_KEEP_XY) {
        // GoToPoseTask.get_spawns (USV_go_to_pose.py:256-319); GoToXYTask / KeepXYTask.get_spawns are the same
        // expressions on the same draws (USV_go_to_xy.py:257-321, USV_keep_xy.py:216-280)
        double rmax = c.spawn_rmax, rmin = c.spawn_rmin;
        if (c.curriculum_on) {   // :266-290, with the step the reference passes (USV_Virtual.py:1546)
          const double st = ref_step_of(c, b, step, 4);
          rmax = curriculum_lerp(c, st, c.cur_max_dist, c.max_spawn_d);
          rmin = curriculum_lerp(c, st, c.cur_min_dist, c.min_spawn_d);
        }
        const float r = U(RU_SPAWN_R) * (float)(rmax - rmin) + (float)rmin;
        const float th = U(RU_SPAWN_TH) * 2.0f * USV_PI_F;
        float sth, cth;
        usv_sincos_cr(th, &sth, &cth);
        if (inj_trig) { cth = U(RU_TRIG); sth = U(RU_TRIG + 1); }
        sx = r * cth + tx;
        sy = r * sth + ty;
        // GoToPoseTask.reset: prev_position_dist = 0 (:227).  GoToXYReward.prev_position_error survives a reset
        // (USV_task_rewards.py:126-151; the step zeroes the reset envs' distance reward instead)
        if (c.task_kind != USV_TASK_GO_TO_XY) b.prev_dist[e] = 0.f;
      } else {   // TrackXYOVelocityTask / TrackXYVelocityTask.get_spawns (:203-219, :158-170): env origin, yaw only
        sx = 0.f;
        sy = 0.f;
      }
      // ---- the reference's cached root state still holds this pre-reset pose when the first substep
      // computes its drag and disturbances (USV_Virtual.py:1103-1117): keep those inputs ----
      if (c.stale_root) {
        const float opx = b.px[e], opy = b.py[e], ovx = b.vx[e], ovy = b.vy[e];
        const QuatRot qr = usv_quat_rot(b.yaw[e]);
        const float so = qr.S, co = qr.C;
        float ub = co * ovx + so * ovy;               // R^T v (Utils.py:10-14, Hydrodynamics.py:209-217)
        float vb = -so * ovx + co * ovy;
        if (c.current_on) {                           // relative to the water (Hydrodynamics.py:224-237)
          ub = ub - (co * c.flow_vel[0] + so * c.flow_vel[1]);
          vb = vb - (-so * c.flow_vel[0] + co * c.flow_vel[1]);
        }
        b.stale[USV_STALE_UB * (size_t)n + e] = ub;
        b.stale[USV_STALE_VB * (size_t)n + e] = vb;
        b.stale[USV_STALE_RB * (size_t)n + e] = b.wz[e];
        b.stale[USV_STALE_PX * (size_t)n + e] = opx;
        b.stale[USV_STALE_PY * (size_t)n + e] = opy;
      }
      // ---- pose / velocities / bookkeeping (USV_Virtual.py:1541-1579) ----
      if (b.scene) {
        // scene replay (_scene_replay_take_scene_indices / _scene_replay_apply, USV_Virtual.py:1372-1457,
        // CaptureXYTask.apply_scene static_obs.py:785-863): pose, velocity, goal and obstacles from the
        // env's next scene; the field is built for the NEW goal; no spawn / velocity / goal draws
        int idx = b.scene_next[e];
        b.scene_next[e] = idx + 1;
        const int ns = b.n_scenes;
        if (b.scene_cycle) {
          idx %= ns;
          if (idx < 0) idx += ns;   // torch's floor modulo
        } else if (idx < 0 || idx >= ns) {
          atomicOr(&b.ctl[USV_CTL_SCENE_ERR], 1);   // the reference raises IndexError (:1387-1391)
          idx = min(max(idx, 0), ns - 1);
        }
        b.scene_last[e] = idx;
        const float *sc = b.scene + (size_t)idx * USV_SCENE_STRIDE;
#pragma unroll
        for (int q = 0; q < 2 * USV_NOBST; ++q) b.obst[(size_t)q * n + e] = sc[USV_SC_OBST + q];
        b.px[e] = sc[USV_SC_START];
        b.py[e] = sc[USV_SC_START + 1];
        {   // the yaw-only quaternion of the scene's start yaw (USV_Virtual.py:1447-1450) through set_world_poses
          float hz, hw;
          usv_sincos_cr(0.5f * sc[USV_SC_YAW], &hz, &hw);
          if (inj_trig) { hw = U(RU_TRIG + 2); hz = U(RU_TRIG + 3); }
          b.yaw[e] = usv_yaw_of_quat(hw, hz);
        }
        b.vx[e] = sc[USV_SC_VEL];
        b.vy[e] = sc[USV_SC_VEL + 1];
        b.tgt_x[e] = sc[USV_SC_GOAL];
        b.tgt_y[e] = sc[USV_SC_GOAL + 1];
        b.field_old_tgt[e] = sc[USV_SC_GOAL];
        b.field_old_tgt[n + e] = sc[USV_SC_GOAL + 1];
      } else {
        b.px[e] = sx;
        b.py[e] = sy;
        b.yaw[e] = yaw0;
        b.vx[e] = U(RU_VX) * 3.0f - 1.5f;
        b.vy[e] = U(RU_VY) * 3.0f - 1.5f;
      }
      b.wz[e] = 0.f;
      b.reset_buf[e] = 0;
      b.progress[e] = 0;
      b.prev_cmd[e] = 0.f;
      b.prev_cmd[n + e] = 0.f;
      // ---- set_targets -> task.get_goals (not called under scene replay, :1613-1616) ----
      if (b.scene) {
      } else if (c.task_kind == USV_TASK_TRACK_XY) {    // USV_track_xy_velocity.py:144-156: target velocity
        const float g = c.goal_random_velocity;
        b.tgt_x[e] = U(RU_GOAL) * g * 2.0f - g;
        b.tgt_y[e] = U(RU_GOAL + 1) * g * 2.0f - g;
      } else if (c.task_kind != USV_TASK_TRACK_XYO) {   // static_obs.py:913-930, USV_go_to_pose.py:229-254,
        const float g = c.goal_random_position;         // USV_go_to_xy.py:238-255, USV_keep_xy.py:197-214
        b.tgt_x[e] = U(RU_GOAL) * g * 2.0f - g;
        b.tgt_y[e] = U(RU_GOAL + 1) * g * 2.0f - g;
        if (c.task_kind == USV_TASK_GO_TO_POSE) b.tgt_h[e] = U(RU_GOAL_H) * USV_PI_F * 2.0f;
      } else {                                   // USV_track_xyo_velocity.py:178-199: target velocities
        const float gl = c.tk_goal_rand[0], ga = c.tk_goal_rand[1];
        b.tgt_x[e] = U(RU_GOAL) * gl * 2.0f - gl;
        b.tgt_y[e] = U(RU_GOAL + 1) * gl * 2.0f - gl;
        b.tgt_h[e] = U(RU_GOAL_H) * ga * 2.0f - ga;
      }
    }
    (void)sx; (void)sy; (void)tx; (void)ty;
  }
  // ---- obstacles: placed by the potential-field kernel, one workgroup per reset env
  // (place_obstacles, usv_device.h); this kernel hands over the draw keys ----
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    b.ctl[USV_CTL_H_SEED_LO] = (int32_t)(uint32_t)seed;
    b.ctl[USV_CTL_H_SEED_HI] = (int32_t)(uint32_t)(seed >> 32);
    b.ctl[USV_CTL_H_STEP_LO] = (int32_t)(uint32_t)step;
    b.ctl[USV_CTL_H_STEP_HI] = (int32_t)(uint32_t)(step >> 32);
    b.ctl[USV_CTL_H_INJ_LO] = (int32_t)(uint32_t)(uintptr_t)inj;
    b.ctl[USV_CTL_H_INJ_HI] = (int32_t)(uint32_t)((uint64_t)(uintptr_t)inj >> 32);
    b.ctl[USV_CTL_PLACE] = b.scene ? 0 : 1;   // scene replay: obstacles come from the scene
  }
  // ---- extras["episode"] = means over this step's resets (:1591-1612), finalised by k_extras_fold in a
  // one-workgroup launch of its own (no device-scope completion counter and fences in this kernel).
  // Per-workgroup partials (no float atomics: one address per statistic would serialise
  // every wave of the grid on it, and the sum order would vary run to run) ----
  __syncthreads();
  const int qs = threadIdx.x;
  if (c.stats_on && qs < USV_NSTAT) {
    float a = wsum[0][qs];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) a += wsum[w][qs];
    b.extras_acc[(size_t)blockIdx.x * USV_NSTAT + qs] = a;
  }
  // the fold runs as k_extras_fold right behind this launch (stream order publishes the partials)
}

__global__ __launch_bounds__(kBlock) void k_extras_fold(usv_cfg_t c, usv_bufs_t b, int nblk) {
  const int qs = threadIdx.x;
  __shared__ float fold[8][32];
  const int count = min(b.ctl[USV_CTL_RESET_COUNT], b.n);
  const int G = nblk;
  if (c.stats_on && count > 0) {
    // 8 interleaved block subsets per statistic, each summed in block order, then combined in order
    static_assert(USV_NSTAT <= 32 && kBlock == 256, "fold layout");
    const int q = qs & 31, k = qs >> 5;
    float a = 0.f;
    if (q < USV_NSTAT) {
      // blocks k, k+8, k+16, ... in that order; 16 loads in flight per batch
      for (int b0 = k; b0 < G; b0 += 128) {
        float x[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) x[u] = b.extras_acc[(size_t)min(b0 + 8 * u, G - 1) * USV_NSTAT + q];
#pragma unroll
        for (int u = 0; u < 16; ++u)
          if (b0 + 8 * u < G) a += x[u];
      }
    }
    fold[k][q] = a;
    __syncthreads();
    if (qs < USV_NSTAT) {
      float tot = fold[0][qs];
#pragma unroll
      for (int kk = 1; kk < 8; ++kk) tot += fold[kk][qs];
      float m = tot / (float)count;
      if (qs != ST_SUCCESS && qs != ST_COLLISION) m = m / (float)c.max_episode_length;
      // USV_NAN_PROBE: the reference raises on a NaN extra before zeroing it (USV_Virtual.py:1601-1605)
      if (c.nan_probe && isnan(m)) atomicOr(&b.ctl[USV_CTL_NAN_FLAG], (int)USV_NAN_EXTRAS);
      b.extras[qs] = isnan(m) ? 0.f : m;
    }
  }
  if (qs == 0) b.ctl[USV_CTL_OBST_DONE] = 0;
}

// ------------------------------------------------------------------------
// grid_sample(field, 2*pos/map, bilinear, border, align_corners=False)
// (static_obs.py:302-326) in the arithmetic of PyTorch's CPU kernel.  Split in
// two: field_taps issues the 4 texel loads as soon as the position is known,
// field_blend combines them where the reward needs the potential.
// ------------------------------------------------------------------------
struct FieldTaps {
  float g_nw, g_ne, g_sw, g_se;    // raw costs of the 4 texels (the env's tiles)
  float4 fn0, fn1;                 // the env's normalisation constants (usv_bufs_t.fnorm)
  float nw, ne, sw, se;
  int i0, i1c, j0, j1c;
  bool i_out, j_out;
};
// F: the env's cost tiles, FN: its USV_FNORM constants
__device__ __forceinline__ FieldTaps field_taps(const float *__restrict__ F, const float *__restrict__ FN,
                                                float map_size, float x, float y) {
  constexpr int G = USV_GRID;
  const float gx = 2.0f * x / map_size, gy = 2.0f * y / map_size;
  const float half = (float)G / 2.0f;
  float ix = fmaf(gx + 1.f, half, -0.5f);
  float iy = fmaf(gy + 1.f, half, -0.5f);
  ix = minf((float)(G - 1), maxf(ix, 0.f));
  iy = minf((float)(G - 1), maxf(iy, 0.f));
  const float xw = floorf(ix), yn = floorf(iy);
  const float w = ix - xw, ee = 1.f - w;
  const float nn = iy - yn, ss = 1.f - nn;
  FieldTaps t;
  t.nw = ss * ee; t.ne = ss * w; t.sw = nn * ee; t.se = nn * w;
  const int i0 = (int)xw, j0 = (int)yn, i1 = i0 + 1, j1 = j0 + 1;
  // border clamp: i1/j1 == G only when the weight of that tap is 0 (ix, iy <= G-1);
  // the tap then reads the last column/row (any finite value) and is replaced by 0
  const int i1c = min(i1, G - 1), j1c = min(j1, G - 1);
  t.g_nw = F[field_idx(j0, i0)];
  t.g_ne = F[field_idx(j0, i1c)];
  t.g_sw = F[field_idx(j1c, i0)];
  t.g_se = F[field_idx(j1c, i1c)];
  t.fn0 = reinterpret_cast<const float4 *>(FN)[0];
  t.fn1 = reinterpret_cast<const float4 *>(FN)[1];
  t.i0 = i0; t.i1c = i1c; t.j0 = j0; t.j1c = j1c;
  t.i_out = i1 >= G;
  t.j_out = j1 >= G;
  return t;
}
// the field's grid coordinates from the host-derived (start, end, step) or the override table
struct GridK {
  float start, end, step;
  const float *lin;
  __device__ __forceinline__ float operator()(int i) const { return lin ? lin[i] : grid_coord_k(start, end, step, i); }
};
// the texels from their parts (the SDF from the env's obstacles ob(o), field_value: the reference's
// normalisation), then the bilinear blend
template <class Ob>
__device__ __forceinline__ float field_blend(const usv_cfg_t &c, const FieldTaps &t, Ob ob, const GridK &gk, float cell,
                                             float inv_r, float inv_safe) {
  const FieldNorm k = field_norm_of(t.fn0, t.fn1);
  const float x0 = gk(t.i0), x1 = gk(t.i1c), y0 = gk(t.j0), y1 = gk(t.j1c);
  const float r = c.obstacle_radius;
  const float v_nw = field_value(c, k, cell_sdf(ob, x0, y0, r), t.g_nw, cell, inv_r, inv_safe);
  float v_ne = field_value(c, k, cell_sdf(ob, x1, y0, r), t.g_ne, cell, inv_r, inv_safe);
  float v_sw = field_value(c, k, cell_sdf(ob, x0, y1, r), t.g_sw, cell, inv_r, inv_safe);
  float v_se = field_value(c, k, cell_sdf(ob, x1, y1, r), t.g_se, cell, inv_r, inv_safe);
  if (t.i_out) { v_ne = 0.f; v_se = 0.f; }
  if (t.j_out) { v_sw = 0.f; v_se = 0.f; }
  return fmaf(v_se, t.se, fmaf(v_sw, t.sw, fmaf(v_ne, t.ne, v_nw * t.nw)));
}

__device__ __forceinline__ float pen_scalar(int kind, float k, float x0, float cc, float x) {
  if (kind == PEN_DEADZONE) return -maxf(fabsf(x) - x0, 0.f) * k + cc;
  if (kind == PEN_EXPABS) return (usv_exp(x0 * fabsf(x)) - 1.0f) * k + cc;
  return 0.f;
}

// ------------------------------------------------------------------------
// Fused control step.  One thread per env.  Every per-env array lives in one
// <2 GiB window of HBM (StepWin: byte offsets from the window base), so all
// per-env loads/stores are buffer instructions with ONE shared 32-bit lane
// offset and a scalar per-array offset: no per-access 64-bit address VALU work.
// ------------------------------------------------------------------------
// reward terms of compute_reward (static_obs.py:335-657) that do not depend on the
// potential, and the potential-dependent tail
struct RewardPre {
  float dist_r0, align0, g, ggate, turning, sf, goal_r, coll, speed_r, ang_r, hi_r, pen_sum;
};
struct RewardOut {
  float pot, total, rew, dist_r, align_r, shaping, turn_haz, danger, gate_pos;
};
__device__ __forceinline__ RewardOut reward_tail(const usv_cfg_t &c, const RewardPre &p, float pot, bool pot_is_prev,
                                                 float prev_pot_mem) {
  constexpr float kXs = 0.3f + 1e-6f, kPa = 2.0f + 1e-6f;
  RewardOut o;
  o.pot = pot;
  const float pn = clampt(pot, 0.f, 1.f);
  const float xs = clampt(div_rn(pn - 0.6f, kXs, 1.0f / kXs), 0.f, 1.f);
  o.danger = xs * xs * (3.0f - 2.0f * xs);
  o.align_r = p.align0 * maxf(0.3f, 1.0f - o.danger);
  float dist_r = p.dist_r0 * maxf(0.6f, 1.0f - o.danger * 0.5f);
  dist_r = minf(dist_r, 0.f) + p.g * maxf(dist_r, 0.f);
  o.dist_r = dist_r;
  const float prev_pot = pot_is_prev ? pot : prev_pot_mem;
  float praw = (prev_pot - pot) * 100.0f;
  if (fabsf(praw) < 0.01f) praw = 0.f;
  const float pa1 = 2.0f * usv_tanh(div_rn(praw, kPa, 1.0f / kPa));
  const float ppos = maxf(pa1, 0.f), pneg = minf(pa1, 0.f);
  o.gate_pos = (ppos < 0.5f) ? 1.0f : p.ggate;
  o.shaping = o.gate_pos * ppos + pneg;
  const bool worsening = o.shaping < -0.05f;
  o.turn_haz = (float)(worsening && p.turning != 0.f) * (-10.0f) * (p.g * p.g) * p.sf;
  o.total = dist_r * 0.5f + o.align_r * 0.5f + o.shaping * 2.0f + o.turn_haz + p.goal_r + c.time_reward + p.coll +
            p.speed_r + p.ang_r + p.hi_r;
  o.rew = o.total + p.pen_sum;
  return o;
}

typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

struct StepWin {
  uint32_t px, py, yaw, vx, vy, wz, fl, fr, mass, k_iz, k_drag, thr_l, thr_r, com_x, com_y, com_z;
  uint32_t lin_damp, quad_damp, progress, tgt_x, tgt_y, obst, goal_cnt, prev_dist, prev_head, prev_pot, prev_wz;
  uint32_t stats, prev_cmd, rew, reset_buf, dones, done_coll, done_succ, just_reset, obs;
  uint32_t dist, env_org, stale;
  uint32_t n4;      // bytes of one [n] f32 row
  uint32_t bytes;   // window size
};
// The same offsets as compile-time constants for the canonical slab (include/usv_hip.h USV_SLAB_*) with
// 2^kShift-byte rows: the general StepWin keeps ~45 offsets live in scalar registers across the kernel and the
// compiler spills them into VGPR lanes (~560 v_readlane / v_writelane per wave); constants are rematerialised
template <int kShift>
struct FixedWin {
  static constexpr uint32_t R(int row) { return (uint32_t)row << kShift; }
  static constexpr uint32_t px = R(USV_SLAB_STATE), py = R(USV_SLAB_STATE + 1), yaw = R(USV_SLAB_STATE + 2),
                            vx = R(USV_SLAB_STATE + 3), vy = R(USV_SLAB_STATE + 4), wz = R(USV_SLAB_STATE + 5),
                            fl = R(USV_SLAB_STATE + 6), fr = R(USV_SLAB_STATE + 7);
  static constexpr uint32_t mass = R(USV_SLAB_PARAMS), com_x = R(USV_SLAB_PARAMS + 1), com_y = R(USV_SLAB_PARAMS + 2),
                            com_z = R(USV_SLAB_PARAMS + 3), k_drag = R(USV_SLAB_PARAMS + 4),
                            thr_l = R(USV_SLAB_PARAMS + 5), thr_r = R(USV_SLAB_PARAMS + 6), k_iz = R(USV_SLAB_PARAMS + 7);
  static constexpr uint32_t lin_damp = R(USV_SLAB_LIN_DAMP), quad_damp = R(USV_SLAB_QUAD_DAMP);
  static constexpr uint32_t tgt_x = R(USV_SLAB_TGT), tgt_y = R(USV_SLAB_TGT + 1), obst = R(USV_SLAB_OBST);
  static constexpr uint32_t prev_cmd = R(USV_SLAB_PREV_CMD);
  static constexpr uint32_t prev_dist = R(USV_SLAB_HIST), prev_head = R(USV_SLAB_HIST + 1),
                            prev_pot = R(USV_SLAB_HIST + 2), prev_wz = R(USV_SLAB_HIST + 3);
  static constexpr uint32_t goal_cnt = R(USV_SLAB_IBUF), progress = R(USV_SLAB_IBUF + 1),
                            reset_buf = R(USV_SLAB_IBUF + 2), done_succ = R(USV_SLAB_IBUF + 3),
                            done_coll = R(USV_SLAB_IBUF + 4);
  static constexpr uint32_t just_reset = R(USV_SLAB_JUST_RESET), stats = R(USV_SLAB_STATS), obs = R(USV_SLAB_OBS),
                            rew = R(USV_SLAB_REW), dones = R(USV_SLAB_DONES), dist = R(USV_SLAB_DIST),
                            env_org = R(USV_SLAB_ENV_ORG), stale = R(USV_SLAB_STALE);
  static constexpr uint32_t n4 = 1u << kShift;
  static constexpr uint32_t bytes = (uint32_t)USV_SLAB_ROWS << kShift;
  static_assert((unsigned long long)USV_SLAB_ROWS << kShift < 0x80000000ull, "window < 2 GiB");
};
constexpr int kFixedShiftMin = 13, kFixedShiftMax = 22;   // n in (1024, 1048576]

// uniform constants derived on the host from usv_cfg_t (float/double arithmetic of the
// reference done once; divisors with their correctly rounded reciprocals for div_rn)
struct StepK {
  float act_rng, pos_rng, vel_rng, head_rng;
  float mass_den, inv_mass_den;
  float com_div[3], inv_com_div[3];
  float priv_base[8];             // the 8 privileged values when they do not depend on the env
  float enc_lo[3], enc_r[3], inv_enc_r[3];   // kdrag, thr, kiz: minmax range / centered scale
  int enc_ok[3];
  float inv_exp_coeff;
  float cell, inv_r, inv_safe;    // the potential field's cell size, 1 / influence radius, RN(1 / safe_radius)
  float gstart, gend, gstep;      // its grid coordinates (grid_coord's float values)
};

// privileged observation tail (USV_Virtual.py:840-976): raw / centered / minmax encoders
template <class Put>
__device__ __forceinline__ void write_priv_tail(const usv_cfg_t &c, const StepK &K, float m, float comx, float comy,
                                                float comz, float k_drag, float thr_l, float thr_r, float k_iz,
                                                Put put) {
  const int pt = USV_NOBS_BASE;
  if (c.masscom_base) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (q < c.priv_dim) put(pt + q, K.priv_base[q]);
    return;
  }
  put(pt, c.mass_relative ? div_rn(m - c.base_mass, K.mass_den, K.inv_mass_den) : m);
  put(pt + 1, c.com_scaled ? div_rn(comx, K.com_div[0], K.inv_com_div[0]) : comx);
  put(pt + 2, c.com_scaled ? div_rn(comy, K.com_div[1], K.inv_com_div[1]) : comy);
  put(pt + 3, c.com_scaled ? div_rn(comz, K.com_div[2], K.inv_com_div[2]) : comz);
  if (c.priv_dim == 8) {
    float v[4] = {k_drag, thr_l, thr_r, k_iz};
    const bool on[4] = {c.priv_drag_on != 0, c.priv_thr_on != 0, c.priv_thr_on != 0, c.priv_kiz_on != 0};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = q == 0 ? 0 : (q == 3 ? 2 : 1);
      if (c.priv_mode == 1) {          // enc_centered
        v[q] = clampt(div_rn(v[q] - c.priv_nominal, K.enc_r[j], K.inv_enc_r[j]), -1.f, 1.f);
      } else if (c.priv_mode == 2) {   // enc_minmax
        if (!on[q] || !K.enc_ok[j]) {
          v[q] = 0.f;
        } else {
          const float z = div_rn(v[q] - K.enc_lo[j], K.enc_r[j], K.inv_enc_r[j]);
          v[q] = clampt(2.0f * z - 1.0f, -1.f, 1.f);
        }
      }
      put(pt + 4 + q, v[q]);
    }
  }
}

__device__ __forceinline__ float bld(__amdgpu_buffer_rsrc_t R, uint32_t so, uint32_t vo) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(R, vo, so, 0));
}
__device__ __forceinline__ int32_t bldi(__amdgpu_buffer_rsrc_t R, uint32_t so, uint32_t vo) {
  return (int32_t)__builtin_amdgcn_raw_buffer_load_b32(R, vo, so, 0);
}
__device__ __forceinline__ void bst(__amdgpu_buffer_rsrc_t R, uint32_t so, uint32_t vo, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), R, vo, so, 0);
}
__device__ __forceinline__ void bsti(__amdgpu_buffer_rsrc_t R, uint32_t so, uint32_t vo, int32_t v) {
  __builtin_amdgcn_raw_buffer_store_b32((uint32_t)v, R, vo, so, 0);
}

// 64-bit (distance bits, obstacle index) compare-exchange for the top-5 network:
// keys are distinct, so the network reproduces torch.topk(largest=False)'s
// order exactly (ties -> lower index first)
__device__ __forceinline__ void cx64(uint64_t &a, uint64_t &b) {
  const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo; b = hi;
}
__device__ __forceinline__ void mn64(uint64_t &a, uint64_t b) { a = a < b ? a : b; }
__device__ __forceinline__ void mx64(uint64_t a, uint64_t &b) { b = a < b ? b : a; }

// the 5 smallest of 16 keys in ascending order in k[0..4]: Batcher's odd-even
// merge sort pruned to the comparators that reach outputs 0..4 (50 of 63;
// checked exhaustively by the 0-1 principle)
__device__ __forceinline__ void top5_of_16(uint64_t k[16]) {
  cx64(k[0], k[1]); cx64(k[2], k[3]); cx64(k[0], k[2]); cx64(k[1], k[3]); cx64(k[1], k[2]);
  cx64(k[4], k[5]); cx64(k[6], k[7]); cx64(k[4], k[6]); cx64(k[5], k[7]); cx64(k[5], k[6]);
  cx64(k[0], k[4]); cx64(k[2], k[6]); cx64(k[2], k[4]); cx64(k[1], k[5]); mn64(k[3], k[7]);
  cx64(k[3], k[5]); cx64(k[1], k[2]); cx64(k[3], k[4]); mn64(k[5], k[6]);
  cx64(k[8], k[9]); cx64(k[10], k[11]); cx64(k[8], k[10]); cx64(k[9], k[11]); cx64(k[9], k[10]);
  cx64(k[12], k[13]); cx64(k[14], k[15]); cx64(k[12], k[14]); cx64(k[13], k[15]); cx64(k[13], k[14]);
  cx64(k[8], k[12]); cx64(k[10], k[14]); cx64(k[10], k[12]); cx64(k[9], k[13]); mn64(k[11], k[15]);
  cx64(k[11], k[13]); cx64(k[9], k[10]); cx64(k[11], k[12]); mn64(k[13], k[14]);
  cx64(k[0], k[8]); mn64(k[4], k[12]); mn64(k[4], k[8]); mn64(k[2], k[10]); cx64(k[2], k[4]);
  cx64(k[1], k[9]); mn64(k[5], k[13]); mn64(k[5], k[9]); mn64(k[3], k[11]); mn64(k[3], k[5]);
  cx64(k[1], k[2]); cx64(k[3], k[4]);
}

// the episode sums whose step value comes out of reward_tail (the potential-dependent part of the reward)
__device__ __forceinline__ constexpr bool stat_of_reward(int key) {
  return key == ST_TOTAL_REWARD || key == ST_DISTANCE_REWARD || key == ST_ALIGNMENT_REWARD ||
         key == ST_POTENTIAL_SHAPING_REWARD || key == ST_TURN_HAZARD_PENALTY || key == ST_DANGER_MEAN ||
         key == ST_DANGER_HI_RATE || key == ST_G_GATE_MEAN;
}

// The config and the host-derived constants travel as ONE first kernel argument, so the kernel can re-read
// them from the kernel-argument segment (scalar loads through a laundered pointer) at the start of a section:
// values loaded at the top stay live in scalar registers across the whole kernel otherwise, and the ~50 of
// them that do not fit were spilled to VGPR lanes (371 v_readlane + the s_nop hazards they bring)
struct StepCfg {
  usv_cfg_t c;
  StepK K;
};
typedef __attribute__((address_space(4))) const StepCfg KStepCfg;
__device__ __forceinline__ StepCfg step_cfg_reload() {
#if defined(__HIP_DEVICE_COMPILE__)
  KStepCfg *p = (KStepCfg *)__builtin_amdgcn_kernarg_segment_ptr();
  __asm__ volatile("" : "+s"(p));   // a new pointer value: nothing loaded before this point is reused
  return *p;
#else
  return StepCfg{};   // (host pass: never called)
#endif
}

// ------------------------------------------------------------------------
// What every control step does, whatever the task: k_env_step (CaptureXY) and k_env_step_task call these; each
// kernel keeps its own loads, stores and config reload points and hands in the c / K of its current reload.
// ------------------------------------------------------------------------
// VecEnvRLGames.step clamp (vec_env_rlgames.py:136-140) + pre_physics_step (USV_Virtual.py:1050-1099) + the index
// of DynamicsFirstOrder.get_cmd_interpolated (ThrusterDynamics.py:179-219); the caller reads its LUT copy
struct ActionMap {
  float cmd0, cmd1;             // the clamped actions
  float prev_cmd0, prev_cmd1;   // what the observation shows as the previous command (0 at a reset)
  float t0, t1, unit0, unit1;   // biased, noised, clamped command and its thrust unit in [0, 1]
  int i0, i1;                   // LUT rows (a reset env commands 0 thrust)
};
__device__ __forceinline__ ActionMap action_map(const usv_cfg_t &c, const StepK &K, float2 a2, bool was_reset,
                                                float bias, const float *u) {
  ActionMap a;
  a.cmd0 = clampt(a2.x, -c.clip_actions, c.clip_actions);
  a.cmd1 = clampt(a2.y, -c.clip_actions, c.clip_actions);
  a.prev_cmd0 = was_reset ? 0.f : a.cmd0;
  a.prev_cmd1 = was_reset ? 0.f : a.cmd1;
  float t0 = a.cmd0, t1 = a.cmd1;
  if (bias != 0.f) { t0 = t0 + bias; t1 = t1 + bias; }
  if (c.act_noise_on) {
    t0 = t0 + (u[SU_ACT] * K.act_rng + c.act_noise_min);
    t1 = t1 + (u[SU_ACT + 1] * K.act_rng + c.act_noise_min);
  }
  a.t0 = clampt(t0, -1.f, 1.f);
  a.t1 = clampt(t1, -1.f, 1.f);
  const float unit0 = c.affine_thrust ? 0.5f * (a.t0 + 1.0f) : clampt(a.t0, 0.f, 1.f);
  const float unit1 = c.affine_thrust ? 0.5f * (a.t1 + 1.0f) : clampt(a.t1, 0.f, 1.f);
  a.unit0 = clampt(unit0, 0.f, 1.f);
  a.unit1 = clampt(unit1, 0.f, 1.f);
  const float uu0 = was_reset ? 0.f : a.unit0, uu1 = was_reset ? 0.f : a.unit1;
  const int i0 = (int)rintf(((uu0 + 1.0f) / 2.0f) * (float)(USV_LUT_N - 1));
  const int i1 = (int)rintf(((uu1 + 1.0f) / 2.0f) * (float)(USV_LUT_N - 1));
  a.i0 = min(max(i0, 0), USV_LUT_N - 1);
  a.i1 = min(max(i1, 0), USV_LUT_N - 1);
  return a;
}

// damping per body axis (Hydrodynamics.py:239-243): (linear + quadratic |v|) scaling_damping [k_drag]; the drag
// force is -D v.  kd is the env's k_drag (read only with use_drag_scale)
struct Damping {
  float lin0, lin1, lin2, qd0, qd1, qd2;
};
struct Drag3 {
  float D0, D1, D2;
};
__device__ __forceinline__ Drag3 drag_coeffs(const usv_cfg_t &c, const Damping &d, float kd, float ub, float vb,
                                             float rb) {
  Drag3 D{d.lin0 + d.qd0 * fabsf(ub), d.lin1 + d.qd1 * fabsf(vb), d.lin2 + d.qd2 * fabsf(rb)};
  D.D0 = D.D0 * c.scaling_damping; D.D1 = D.D1 * c.scaling_damping; D.D2 = D.D2 * c.scaling_damping;
  if (c.use_drag_scale) { D.D0 = D.D0 * kd; D.D1 = D.D1 * kd; D.D2 = D.D2 * kd; }
  return D;
}

// ---- the substeps: thruster lag, planar forces, semi-implicit Euler.  The integrator is this build's own (it
// replaces PhysX): accelerations divide by m and Izz through their reciprocals with one correction step
// (div_rn == the IEEE quotient for quotients in [2^-90, 2^120]) ----
struct BodyState {
  float px, py, yaw, vx, vy, wz, fl, fr;
};
struct SubstepIn {
  float lut0, lut1;                      // the thruster LUT's entries at ActionMap::i0 / i1
  float m, k_iz, k_drag, thr_l, thr_r, comy;
  Damping damp;                          // the env's (drag DR) or the config's
  float dp[USV_NDIST], orgx, orgy;       // disturbance parameters (drawn at reset), env origin: read with dist only
  bool stl;                              // a reset env's first substep sees the pre-reset inputs usv_reset kept
  float st_ub, st_vb, st_rb, st_px, st_py;   // (st_px / st_py with dist only)
};
// dist: any disturbance term or the water current on (a compile-time constant in k_env_step, uniform in the
// task kernel)
__device__ __forceinline__ void integrate_substeps(const usv_cfg_t &c, const SubstepIn &in, bool dist, BodyState &s) {
  float tgt0 = in.lut0, tgt1 = in.lut1;
  if (c.use_thr_mult) { tgt0 = tgt0 * in.thr_l; tgt1 = tgt1 * in.thr_r; }
  const float m = in.m, izz = c.izz0 * in.k_iz;
  const float inv_m = 1.0f / m, inv_izz = 1.0f / izz;
  const float kd = c.use_drag_scale ? in.k_drag : 1.0f;
  const float al = c.thr_alpha, oma = 1.0f - c.thr_alpha;
  const float dt = c.dt;
  const float arm_l = -(c.thr_y - in.comy), arm_r = c.thr_y + in.comy;
  const float *dp = in.dp;
  float px = s.px, py = s.py, yaw = s.yaw, vx = s.vx, vy = s.vy, wz = s.wz, fl = s.fl, fr = s.fr;
  for (int i = 0; i < c.substeps; ++i) {
    fl = fl * al + oma * tgt0;                      // ThrusterDynamics.py:133-136
    fr = fr * al + oma * tgt1;
    // the attitude the reference reads back: R = quaternion_to_matrix(q(yaw)) (usv_quat_rot)
    const QuatRot qr = usv_quat_rot(yaw);
    const float sy_ = qr.S, cy_ = qr.C;
    float ub = cy_ * vx + sy_ * vy;                 // R^T v (Utils.py:10-14, Hydrodynamics.py:209-217)
    float vb = -sy_ * vx + cy_ * vy;
    float rb = wz;
    float hpx = px, hpy = py;
    if (dist && c.current_on) {                     // relative to the water (Hydrodynamics.py:224-237)
      ub = ub - (cy_ * c.flow_vel[0] + sy_ * c.flow_vel[1]);
      vb = vb - (-sy_ * c.flow_vel[0] + cy_ * c.flow_vel[1]);
    }
    if (i == 0) {                                   // the cached pre-reset root state
      ub = in.stl ? in.st_ub : ub;
      vb = in.stl ? in.st_vb : vb;
      rb = in.stl ? in.st_rb : rb;
      hpx = in.stl ? in.st_px : hpx;
      hpy = in.stl ? in.st_py : hpy;
    }
    float dfx = 0.f, dfy = 0.f, dtz = 0.f;
    if (dist) {
      // get_disturbance_forces / get_torque_disturbance at root_pos (USV_disturbances.py:386-410,510-530)
      const float wx = hpx + in.orgx, wy = hpy + in.orgy;
      dfx = dp[DI_FCX];
      dfy = dp[DI_FCY];
      dtz = dp[DI_TC];
      if (c.fsin_on) {
        dfx = dfx + usv_sin_cr(wx * dp[DI_FXF] + dp[DI_FXS]) * dp[DI_FAMP];
        dfy = dfy + usv_sin_cr(wy * dp[DI_FYF] + dp[DI_FYS]) * dp[DI_FAMP];
      }
      if (c.tsin_on) dtz = dtz + usv_sin_cr((wx + wy) * dp[DI_TF] + dp[DI_TS]) * dp[DI_TAMP];
    }
    const Drag3 D = drag_coeffs(c, in.damp, kd, ub, vb, rb);
    // base force = disturbance + drag (+ hydrostatics, 0 in the plane), thrusters (USV_Virtual.py:1118-1132)
    const float X = dist ? fl + fr + (dfx + (-D.D0 * ub)) : fl + fr + (-D.D0 * ub);   // Hydrodynamics.py:243
    const float Y = dist ? dfy + (-D.D1 * vb) : -D.D1 * vb;
    const float N = dist ? arm_l * fl + arm_r * fr + (dtz + (-D.D2 * rb)) : arm_l * fl + arm_r * fr + (-D.D2 * rb);
    const float ax = div_rn(cy_ * X - sy_ * Y, m, inv_m);
    const float ay = div_rn(sy_ * X + cy_ * Y, m, inv_m);
    const float aw = div_rn(N, izz, inv_izz);
    vx = vx + ax * dt;
    vy = vy + ay * dt;
    wz = wz + aw * dt;
    px = px + vx * dt;
    py = py + vy * dt;
    float yw = yaw + wz * dt;
    if (yw > USV_PI_F) yw -= USV_2PI_F;
    else if (yw <= -USV_PI_F) yw += USV_2PI_F;
    yaw = yw;
  }
  s = BodyState{px, py, yaw, vx, vy, wz, fl, fr};
}

// ---- update_state's noise (USV_Virtual.py:771-813).  The position stands alone: k_env_step issues the
// potential's texel loads as soon as it exists ----
__device__ __forceinline__ float2 observed_position(const usv_cfg_t &c, const StepK &K, const float *u, float px,
                                                    float py) {
  float pxn = px, pyn = py;
  if (c.pos_noise_on) {
    pxn = pxn + (u[SU_PX] * K.pos_rng + c.pos_noise_min);
    pyn = pyn + (u[SU_PX + 1] * K.pos_rng + c.pos_noise_min);
  }
  return make_float2(pxn, pyn);
}
struct ObservedMotion {
  float vxn, vyn, wzn;
  float yawn, hs, hc;   // the noisy heading, its sine and cosine
};
__device__ __forceinline__ ObservedMotion observed_motion(const usv_cfg_t &c, const StepK &K, const float *u,
                                                          const BodyState &s) {
  ObservedMotion o{s.vx, s.vy, s.wz, 0.f, 0.f, 0.f};
  if (c.vel_noise_on) {
    o.vxn = o.vxn + (u[SU_VX] * K.vel_rng + c.vel_noise_min);
    o.vyn = o.vyn + (u[SU_VY] * K.vel_rng + c.vel_noise_min);
    o.wzn = o.wzn + (u[SU_WZ] * K.vel_rng + c.vel_noise_min);
  }
  // update_state's heading: atan2 of the read-back quaternion (USV_Virtual.py:776-786), then its noise
  o.yawn = usv_heading(usv_quat_rot(s.yaw));
  if (c.head_noise_on) o.yawn = o.yawn + (u[SU_HEAD] * K.head_rng + c.head_noise_min);
  usv_sincos(o.yawn, &o.hs, &o.hc);
  return o;
}
// observation columns 0-2: the velocity in the body or the world frame (static_obs.py:193-299, USV_core.py:55-121)
template <class Put>
__device__ __forceinline__ void put_velocity_columns(const usv_cfg_t &c, const ObservedMotion &o, Put put) {
  if (c.obs_local) {
    put(0, o.hc * o.vxn + o.hs * o.vyn);
    put(1, -o.hs * o.vxn + o.hc * o.vyn);
  } else {
    put(0, o.vxn);
    put(1, o.vyn);
  }
  put(2, o.wzn);
}

// ---- Penalties.compute_penalty (USV_task_rewards.py:440-523) without its action-variation term ----
struct StepPenalties {
  float p_ang, p_angv, p_en;   // the terms with an episode sum
  float sum;                   // ((p_lin + p_ang) + p_angv) + p_en
};
__device__ __forceinline__ StepPenalties step_penalties(const usv_cfg_t &c, const ActionMap &a, const ObservedMotion &o,
                                                        bool pen_valid, float prev_wz_mem) {
  const float pact0 = c.pen_use_u ? a.unit0 : a.cmd0, pact1 = c.pen_use_u ? a.unit1 : a.cmd1;
  float p_lin = 0.f, p_ang = 0.f, p_angv = 0.f, p_en = 0.f;
  if (c.pen_lin_kind == PEN_NORM) p_lin = -tnorm2(o.vxn, o.vyn) * c.pen_lin_k + c.pen_lin_c;
  if (c.pen_ang_kind) p_ang = pen_scalar(c.pen_ang_kind, c.pen_ang_k, c.pen_ang_x0, c.pen_ang_c, o.wzn);
  if (c.pen_angv_kind) {
    const float prev_w = pen_valid ? prev_wz_mem : o.wzn;
    p_angv = pen_scalar(c.pen_angv_kind, c.pen_angv_k, c.pen_angv_x0, c.pen_angv_c, o.wzn - prev_w);
  }
  if (c.pen_en_kind == PEN_SUM) p_en = -(pact0 + pact1) * c.pen_en_k + c.pen_en_c;
  else if (c.pen_en_kind == PEN_SUMSQ) p_en = -(pact0 * pact0 + pact1 * pact1) * c.pen_en_k + c.pen_en_c;
  return StepPenalties{p_ang, p_angv, p_en, ((p_lin + p_ang) + p_angv) + p_en};
}

// the NaN probe's bits for the clamped actions and the observed state (the reward's and the obs row's are the caller's)
__device__ __forceinline__ uint32_t nan_bits_actions_state(const ActionMap &a, float2 pn, const ObservedMotion &o) {
  return ((nonfinite(a.cmd0) | nonfinite(a.cmd1)) ? USV_NAN_ACTIONS : 0u) |
         ((nonfinite(pn.x) | nonfinite(pn.y) | nonfinite(o.yawn) | nonfinite(o.vxn) | nonfinite(o.vyn) |
           nonfinite(o.wzn)) ? USV_NAN_STATE : 0u);
}

// the step's addends to the state statistics every task keeps (USV_Virtual.py:584-601)
constexpr int kStateStatKey[6] = {ST_NORMED_LINEAR_VEL, ST_NORMED_ANGULAR_VEL, ST_CMD_NEG_RATE,
                                  ST_U_MEAN,            ST_U_LOW_RATE,         ST_U_SUM};
struct StateStats {
  float v[6];   // kStateStatKey's order
};
__device__ __forceinline__ StateStats state_stats(const ActionMap &a, const ObservedMotion &o) {
  return StateStats{{tnorm2(o.vxn, o.vyn), fabsf(o.wzn), ((float)(a.t0 < 0.f) + (float)(a.t1 < 0.f)) / 2.0f,
                     (a.unit0 + a.unit1) / 2.0f, ((float)(a.unit0 < 0.05f) + (float)(a.unit1 < 0.05f)) / 2.0f,
                     a.unit0 + a.unit1}};
}

template <bool kStats, bool kInj, bool kDist, class Win>
__global__ __launch_bounds__(kBlock) void k_env_step(StepCfg ck, usv_bufs_t b, Win w,
                                                     const char *__restrict__ wbase, const float *__restrict__ actions,
                                                     const float *__restrict__ lut, float bias, uint64_t seed,
                                                     uint64_t step, const float *__restrict__ inj, int part) {
  __shared__ float sobs[kBlock * USV_NOBS];
  __shared__ float2 sob[USV_NOBST][kBlock];
  __shared__ float slut[2 * USV_LUT_N];
  __shared__ uint8_t keep[kBlock];
  const usv_cfg_t &c = ck.c;
  const StepK &K = ck.K;
  const int n = b.n;
  const int tid = threadIdx.x;
  const int e = blockIdx.x * kBlock + tid;
  const __amdgpu_buffer_rsrc_t R = __builtin_amdgcn_make_buffer_rsrc((void *)wbase, 0, (int)w.bytes, 0x00020000);
  // thruster LUT -> registers first (the oldest loads in flight: waiting for them before
  // the LDS write below does not wait for the per-env loads issued after them)
  static_assert(2 * USV_LUT_N / 4 <= 2 * kBlock, "LUT staging: two float4 per thread");
  const float4 *lut4 = reinterpret_cast<const float4 *>(lut);
  const bool lut_hi = tid + kBlock < 2 * USV_LUT_N / 4;
  const float4 lut_a = lut4[tid];
  const float4 lut_b = lut4[min(tid + kBlock, 2 * USV_LUT_N / 4 - 1)];   // unconditional: no branch, no early wait
  // part 0: every env; 1: envs not reset this step (they do not read this step's new
  // fields, so this part can run concurrently with the potential-field kernels);
  // 2: the envs reset this step, after their fields are built
  // Every lane runs the whole step (lanes past n on env n-1); the stores of lanes that
  // are not `mine` go to an offset past the window, which the buffer range check drops.
  const int ec = min(e, n - 1);
  const uint32_t v4 = (uint32_t)ec * 4u;
  // loads in the order they are consumed (vmcnt waits retire loads in issue order):
  // action + reset flag (LUT index), state and parameters (substeps), then the rest
  const float2 a2 = reinterpret_cast<const float2 *>(actions)[ec];
  const bool was_reset = __builtin_amdgcn_raw_buffer_load_b8(R, (uint32_t)ec, w.just_reset, 0) != 0;
  __builtin_amdgcn_sched_barrier(0);
  constexpr uint32_t kDrop = 0x80000000u;   // > w.bytes
  const int32_t *ctl = b.ctl;
  // control words: plain (non-short-circuit) scalar reads, so no branch waits on memory here
  const int32_t ctl_pot = ctl[USV_CTL_POT_VALID], ctl_cnt = ctl[USV_CTL_RESET_COUNT];
  const bool pot_none = (ctl_pot == 0) | (ctl_cnt > 0);
  const bool pen_valid = ctl[USV_CTL_PEN_VALID] != 0;
  const bool rew_valid = ctl[USV_CTL_REW_VALID] != 0;
  step = step_of(b, step);
  bias = bias_of(c, b, bias);
  // obs row staged in LDS (odd row stride: conflict-free), clamped on write
  // (_process_data clamp, vec_env_rlgames.py:85-95); slots no branch writes are zeroed
  float *obs = sobs + tid * USV_NOBS;
  const float clip = c.clip_obs;
  auto put = [&](int q, float v) { obs[q] = clampt(v, -clip, clip); };
  obs[6] = 0.f;
  obs[7] = 0.f;
  if (c.priv_dim == 4) { obs[29] = 0.f; obs[30] = 0.f; obs[31] = 0.f; obs[32] = 0.f; }   // input padding
  {
    // ---- every per-env input that does not depend on this step's results is loaded
    // up front, so the HBM latencies overlap each other and the physics ----
    BodyState s{bld(R, w.px, v4), bld(R, w.py, v4), bld(R, w.yaw, v4), bld(R, w.vx, v4), bld(R, w.vy, v4),
                bld(R, w.wz, v4), bld(R, w.fl, v4), bld(R, w.fr, v4)};
    const float m = bld(R, w.mass, v4);
    const float k_iz = bld(R, w.k_iz, v4), k_drag = bld(R, w.k_drag, v4);
    const float thr_l = bld(R, w.thr_l, v4), thr_r = bld(R, w.thr_r, v4);
    const float comx = bld(R, w.com_x, v4), comy = bld(R, w.com_y, v4), comz = bld(R, w.com_z, v4);
    // per-env damping (drag DR) or the config's: loaded unconditionally (offset 0 is inside
    // the window when absent) and selected, so no branch sits between the loads
    const bool dr = b.lin_damp != nullptr;
    const float l0 = bld(R, w.lin_damp, v4), l1 = bld(R, w.lin_damp + w.n4, v4), l2 = bld(R, w.lin_damp + 2 * w.n4, v4);
    const float q0 = bld(R, w.quad_damp, v4), q1 = bld(R, w.quad_damp + w.n4, v4);
    const float q2 = bld(R, w.quad_damp + 2 * w.n4, v4);
    SubstepIn in;
    in.damp = Damping{dr ? l0 : c.lin_damp[0], dr ? l1 : c.lin_damp[1], dr ? l2 : c.lin_damp[2],
                      dr ? q0 : c.quad_damp[0], dr ? q1 : c.quad_damp[1], dr ? q2 : c.quad_damp[2]};
    // disturbance parameters (drawn at reset) and the env origin (root_pos is world-frame)
    in.orgx = 0.f;
    in.orgy = 0.f;
    if (kDist) {
#pragma unroll
      for (int q = 0; q < USV_NDIST; ++q) in.dp[q] = bld(R, w.dist + (uint32_t)q * w.n4, v4);
      const float ox_ = bld(R, w.env_org, v4), oy_ = bld(R, w.env_org + w.n4, v4);
      in.orgx = b.env_org ? ox_ : 0.f;
      in.orgy = b.env_org ? oy_ : 0.f;
    }
    // a reset env's first substep: the pre-reset inputs usv_reset kept; the other lanes
    // read past the window (no memory access, 0)
    in.stl = c.stale_root && was_reset;
    const uint32_t vst = in.stl ? v4 : kDrop;
    in.st_ub = bld(R, w.stale + USV_STALE_UB * w.n4, vst);
    in.st_vb = bld(R, w.stale + USV_STALE_VB * w.n4, vst);
    in.st_rb = bld(R, w.stale + USV_STALE_RB * w.n4, vst);
    in.st_px = in.st_py = 0.f;
    if (kDist) {
      in.st_px = bld(R, w.stale + USV_STALE_PX * w.n4, vst);
      in.st_py = bld(R, w.stale + USV_STALE_PY * w.n4, vst);
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the substep inputs ahead of the loads below
    const int progress0 = bldi(R, w.progress, v4);
    const float tgx = bld(R, w.tgt_x, v4), tgy = bld(R, w.tgt_y, v4);
    float obx[USV_NOBST], oby[USV_NOBST];
#pragma unroll
    for (int o = 0; o < USV_NOBST; ++o) {
      obx[o] = bld(R, w.obst + (uint32_t)(2 * o) * w.n4, v4);
      oby[o] = bld(R, w.obst + (uint32_t)(2 * o + 1) * w.n4, v4);
    }
    const int goal_cnt0 = bldi(R, w.goal_cnt, v4);

    const float prev_d_mem = bld(R, w.prev_dist, v4), prev_head_mem = bld(R, w.prev_head, v4);
    const float prev_pot_mem = bld(R, w.prev_pot, v4), prev_wz_mem = bld(R, w.prev_wz, v4);
    // episode sums that this step adds to (the other keys are written by the reset path only)
    constexpr int kSum[25] = {ST_TOTAL_REWARD, ST_DISTANCE_REWARD, ST_ALIGNMENT_REWARD, ST_HEADING_IMPROVE_REWARD,
                              ST_POTENTIAL_SHAPING_REWARD, ST_SPEED_REWARD, ST_ANGULAR_REWARD,
                              ST_TURN_HAZARD_PENALTY, ST_GOAL_REWARD, ST_TIME_REWARD, ST_COLLISION_REWARD,
                              ST_DANGER_MEAN, ST_DANGER_HI_RATE, ST_G_GATE_MEAN, ST_POSITION_ERROR,
                              ST_BOUNDARY_PENALTY, ST_ANGULAR_VEL_PENALTY, ST_ANGULAR_VEL_VARIATION_PENALTY,
                              ST_ENERGY_PENALTY, ST_NORMED_LINEAR_VEL, ST_NORMED_ANGULAR_VEL, ST_CMD_NEG_RATE,
                              ST_U_MEAN, ST_U_LOW_RATE, ST_U_SUM};
    const bool sum_on[25] = {true, true, true, true, true, true, true, true, true, true, true, true, true,
                             true, true, true, c.pen_ang_kind != 0, c.pen_angv_kind != 0, c.pen_en_kind != 0,
                             true, true, true, true, true, true};
    float sums[25];
    if (kStats) {
#pragma unroll
      for (int q = 0; q < 25; ++q) sums[q] = bld(R, w.stats + (uint32_t)kSum[q] * w.n4, v4);
    }
    // ---- uniforms of this step (SU_* layout; the second Philox block only when drawn from) ----
    float u[USV_NU_STEP];
    if (kInj) {
#pragma unroll
      for (int i = 0; i < USV_NU_STEP; ++i) u[i] = inj[(size_t)ec * USV_NU_STEP + i];
    } else {
      philox_u4(seed, (uint32_t)e, step, 0u, u);
      if (c.pos_noise_on || c.act_noise_on) philox_u4(seed, (uint32_t)e, step, 1u, u + 4);
      else u[4] = u[5] = u[6] = u[7] = 0.f;
    }
    const ActionMap am = action_map(c, K, a2, was_reset, bias, u);
    bool mine = e < n;
    if (part == 1 || part == 2) mine = mine && ((part == 1) ? !was_reset : was_reset);
    // part 3: every env, but the envs reset this step leave their potential-dependent reward to
    // usv_env_step_late (their fields are still being built): stash + no rew / prev_pot / reward sums
    const bool defer = part == 3 && was_reset;
    keep[tid] = mine ? 1 : 0;
    const uint32_t vs = mine ? v4 : kDrop;
    reinterpret_cast<float4 *>(slut)[tid] = lut_a;
    if (lut_hi) reinterpret_cast<float4 *>(slut)[tid + kBlock] = lut_b;
    __syncthreads();   // LUT staged
    in.lut0 = slut[am.i0];
    in.lut1 = slut[USV_LUT_N + am.i1];
    in.m = m; in.k_iz = k_iz; in.k_drag = k_drag; in.thr_l = thr_l; in.thr_r = thr_r; in.comy = comy;
    integrate_substeps(c, in, kDist, s);
    bst(R, w.px, vs, s.px); bst(R, w.py, vs, s.py); bst(R, w.yaw, vs, s.yaw);
    bst(R, w.vx, vs, s.vx); bst(R, w.vy, vs, s.vy); bst(R, w.wz, vs, s.wz);
    bst(R, w.fl, vs, s.fl); bst(R, w.fr, vs, s.fr);
    // the rest of the step reads its config afresh (see StepCfg)
    const StepCfg ck2 = step_cfg_reload();
    const usv_cfg_t &c = ck2.c;
    const StepK &K = ck2.K;
    // ---- post_physics_step: progress, update_state noise (USV_Virtual.py:771-813) ----
    const int progress = progress0 + 1;
    bsti(R, w.progress, vs, progress);
    const float2 pn = observed_position(c, K, u, s.px, s.py);
    const float pxn = pn.x, pyn = pn.y;
    // the potential sample only needs the position: issue its 4 texel loads now
    const FieldTaps taps = field_taps(b.field + (size_t)ec * USV_FIELD_STRIDE, b.fnorm + (size_t)ec * USV_FNORM,
                                      c.map_size, pxn, pyn);
    const ObservedMotion om = observed_motion(c, K, u, s);
    const float vxn = om.vxn, vyn = om.vyn, wzn = om.wzn, hs = om.hs, hc = om.hc;
    // ---- get_state_observations (static_obs.py:193-299) ----
    const float ex = tgx - pxn, ey = tgy - pyn;
    const float theta = usv_atan2(hs, hc);
    const float beta = usv_atan2(ey, ex);
    const float alpha = fmodf((beta - theta) + USV_PI_F, USV_2PI_F) - USV_PI_F;
    const float herr = fabsf(alpha);
    const float dist = sqrtf(ex * ex + ey * ey);
    const float dist_n = tnorm2(ex, ey);
    float st, ct, sa, ca;
    usv_sincos(theta, &st, &ct);
    usv_sincos(alpha, &sa, &ca);     // usv_sincos's cos is exactly even: ca == cos(herr) as well
    // 16 obstacle distances; the 5 nearest (torch.topk largest=False, ascending) by a
    // selection network over (distance bits, index) keys -- distances are >= 0 so
    // their bit patterns order like the floats
    uint64_t key[USV_NOBST];
    float min_od = INFINITY, coll = 0.f;
#pragma unroll
    for (int o = 0; o < USV_NOBST; ++o) {
      const float d = tnorm2(obx[o] - pxn, oby[o] - pyn);
      min_od = fminf(min_od, d);
      coll += (float)(d < c.collision_threshold) * (-10.0f) * 10.0f;
      key[o] = ((uint64_t)__float_as_uint(d) << 4) | (uint64_t)o;
      sob[o][tid] = make_float2(obx[o], oby[o]);
    }
    top5_of_16(key);
    put_velocity_columns(c, om, put);
    put(3, ca);
    put(4, sa);
    put(5, dist_n);
#pragma unroll
    for (int q = 0; q < USV_NCLOSE; ++q) {
      const int o = (int)(key[q] & 15u);
      const float2 ob = sob[o][tid];
      const float bx = ob.x - pxn, by = ob.y - pyn;
      const float bd = __uint_as_float((uint32_t)(key[q] >> 4));
      const float vbx = bx * ct + by * st;
      const float vby = -bx * st + by * ct;
      const float nf = sqrtf(vbx * vbx + vby * vby + 1e-6f);
      const float inv_nf = 1.0f / nf;
      put(8 + 3 * q, bd - c.obstacle_radius);
      put(9 + 3 * q, div_rn(-vbx, nf, inv_nf));
      put(10 + 3 * q, div_rn(-vby, nf, inv_nf));
    }
    const int pa = USV_NOBS_BASE - 2;
    put(pa, am.prev_cmd0);
    put(pa + 1, am.prev_cmd1);
    bst(R, w.prev_cmd, vs, am.prev_cmd0);
    bst(R, w.prev_cmd + w.n4, vs, am.prev_cmd1);
    // ---- privileged tail (USV_Virtual.py:840-976) ----
    write_priv_tail(c, K, m, comx, comy, comz, k_drag, thr_l, thr_r, k_iz, put);
    {   // the reward / kill / statistics section reads its config afresh too (see StepCfg)
    const StepCfg ck3 = step_cfg_reload();
    const usv_cfg_t &c = ck3.c;
    const StepK &K = ck3.K;
    // ---- compute_reward (static_obs.py:335-657): the potential-independent terms first ----
    constexpr float kGv = (0.15f - 0.02f) + 1e-6f, kGd = 0.01f + 1e-6f;
    constexpr float kSf = (0.60f - 0.15f) + 1e-6f, kSp = 0.8f + 1e-6f, kAn = 0.2f;
    const float bover = maxf(dist - c.kill_dist, 0.f);
    const float bpen = -expm1f(minf(bover / 0.25f, 20.0f)) * c.boundary_cost;
    const int gir = dist < c.position_tolerance;
    const int goal_cnt = goal_cnt0 * gir + gir;
    bsti(R, w.goal_cnt, vs, goal_cnt);
    const float prev_err = rew_valid ? prev_d_mem : dist;
    RewardPre rp;
    if (c.reward_mode == 0) rp.dist_r0 = c.position_scale * (prev_err - dist);
    else if (c.reward_mode == 1) rp.dist_r0 = c.position_scale * (prev_err * prev_err - dist * dist);
    else rp.dist_r0 = c.position_scale * (usv_exp(div_rn(-dist, c.exp_coeff, K.inv_exp_coeff)) -
                                          usv_exp(div_rn(-prev_err, c.exp_coeff, K.inv_exp_coeff)));
    const float h2 = herr * herr;
    rp.align0 = c.align_la1 * (usv_exp(c.align_la2 * (h2 * h2)) + usv_exp(c.align_la3 * h2));
    if (was_reset) rp.dist_r0 = 0.f;
    const float prev_dist = was_reset ? dist : (rew_valid ? prev_d_mem : dist);
    rp.g = clampt(ca, 0.f, 1.f);
    const float prev_h = (rew_valid && !was_reset) ? prev_head_mem : herr;
    const float hi = clampt(prev_h - herr, -0.4f, 0.4f);
    rp.hi_r = hi * 0.05f;
    bst(R, w.prev_head, vs, herr);
    const float dd = dist + 1e-6f, inv_dd = 1.0f / dd;
    const float gdx = div_rn(ex, dd, inv_dd), gdy = div_rn(ey, dd, inv_dd);
    const float vtp = maxf(vxn * gdx + vyn * gdy, 0.f);
    const float ddp = maxf(prev_dist - dist, 0.f);
    const float gv = clampt(div_rn(vtp - 0.02f, kGv, 1.0f / kGv), 0.f, 1.f);
    const float gd = clampt(div_rn(ddp, kGd, 1.0f / kGd), 0.f, 1.f);
    rp.ggate = maxf(gv, gd) * rp.g;
    rp.turning = fabsf(wzn) > 0.2f ? 1.f : 0.f;
    const float vfwd = vxn * hc + vyn * hs;
    rp.sf = clampt(div_rn(fabsf(vfwd) - 0.15f, kSf, 1.0f / kSf), 0.f, 1.f);
    rp.speed_r = (1.0f - usv_exp(div_rn(-vtp, kSp, 1.0f / kSp))) * 0.05f;
    const float sgn = (alpha > 0.f) ? 1.f : ((alpha < 0.f) ? -1.f : 0.f);
    const float tang = (herr > 1.0f) ? sgn * 1.0f : sgn * 0.2f;
    const float dw = wzn - tang;
    rp.ang_r = usv_exp(div_rn(-(dw * dw), kAn, 1.0f / kAn)) * 0.03f;
    rp.goal_r = ((float)goal_cnt * c.goal_reward) * 5.0f;
    rp.coll = coll;
    bst(R, w.prev_dist, vs, dist);
    const StepPenalties pen = step_penalties(c, am, om, pen_valid, prev_wz_mem);
    bst(R, w.prev_wz, vs, wzn);
    rp.pen_sum = pen.sum;
    // ---- the potential-dependent tail ----
    const RewardOut ro = reward_tail(c, rp, field_blend(c, taps, [&](int o) { return sob[o][tid]; }, GridK{K.gstart, K.gend, K.gstep, b.grid_lin},
                                                 K.cell, K.inv_r, K.inv_safe), pot_none || was_reset, prev_pot_mem);
    const uint32_t vr = defer ? kDrop : vs;   // the potential-dependent outputs
    bst(R, w.prev_pot, vr, ro.pot);
    bst(R, w.rew, vr, ro.rew);
    if (defer && mine) {
      const float st[USV_RSTASH_ROWS] = {rp.dist_r0, rp.align0, rp.g, rp.ggate, rp.turning, rp.sf, rp.goal_r, rp.coll,
                                         rp.speed_r, rp.ang_r, rp.hi_r, rp.pen_sum, pxn, pyn};
#pragma unroll
      for (int q = 0; q < USV_RSTASH_ROWS; ++q) b.rstash[(size_t)q * n + e] = st[q];
    }
    // ---- update_kills / is_done (static_obs.py:661-706, USV_Virtual.py:1223-1237) ----
    const bool dkill = dist > c.kill_dist;
    const bool ckill = min_od < c.collision_threshold;
    const bool skill = goal_cnt >= c.kill_after_n;
    const bool die = dkill || ckill || skill;
    if (die) {
      bsti(R, w.done_coll, vs, ckill);
      bsti(R, w.done_succ, vs, skill && !ckill);
    }
    const int tout = progress >= c.max_episode_length - 1;
    const int rb = c.fixed_horizon_eval ? tout : (tout ? 1 : (int)die);
    bsti(R, w.reset_buf, vs, rb);
    const u32x2_t rb64 = {(uint32_t)rb, 0u};
    __builtin_amdgcn_raw_buffer_store_b64(rb64, R, mine ? (uint32_t)ec * 8u : kDrop, w.dones, 0);
    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)0, R, mine ? (uint32_t)ec : kDrop, w.just_reset, 0);
    if (c.nan_probe) {   // clamped actions, the observed state, the reward (obs: at the row store below)
      const uint32_t bits = nan_bits_actions_state(am, pn, om) | ((!defer && nonfinite(ro.rew)) ? USV_NAN_REWARD : 0u);
      nan_report(&b.ctl[USV_CTL_NAN_FLAG], mine ? bits : 0u);
    }
    if (kStats) {
      const StateStats ss = state_stats(am, om);
      static_assert(kSum[19] == kStateStatKey[0] && kSum[20] == kStateStatKey[1] && kSum[21] == kStateStatKey[2] &&
                    kSum[22] == kStateStatKey[3] && kSum[23] == kStateStatKey[4] && kSum[24] == kStateStatKey[5],
                    "kSum ends in the state statistics");
      const float add[25] = {ro.total, ro.dist_r, ro.align_r, rp.hi_r, ro.shaping, rp.speed_r, rp.ang_r, ro.turn_haz,
                             rp.goal_r, c.time_reward, coll, ro.danger, (float)(ro.danger > 0.5f), ro.gate_pos, dist,
                             bpen, pen.p_ang, pen.p_angv, pen.p_en,
                             ss.v[0], ss.v[1], ss.v[2], ss.v[3], ss.v[4], ss.v[5]};
#pragma unroll
      for (int q = 0; q < 25; ++q)
        if (sum_on[q]) bst(R, w.stats + (uint32_t)kSum[q] * w.n4, stat_of_reward(kSum[q]) ? vr : vs, sums[q] + add[q]);
    }
    }
  }
  // ---- coalesced obs store: rows of 33 floats staged through LDS ----
  __syncthreads();
  const int row0 = blockIdx.x * kBlock;
  const int rows = min(kBlock, n - row0);
  const uint32_t obase = (uint32_t)row0 * (uint32_t)(USV_NOBS * 4);
  // obs entries are clamped to +-clip_obs, so only a NaN is non-finite: x != x
  uint32_t obad = 0u;
  if (part == 0 || part == 3) {
    const int nv = rows * USV_NOBS / 4;       // whole float4s (row0 * 33 * 4 B is 16-B aligned)
    for (int i = tid; i < nv; i += kBlock) {
      const float4 v = reinterpret_cast<const float4 *>(sobs)[i];
      obad |= (uint32_t)((v.x != v.x) | (v.y != v.y) | (v.z != v.z) | (v.w != v.w));
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v),
                                             R, obase + (uint32_t)i * 16u, w.obs, 0);
    }
    for (int i = nv * 4 + tid; i < rows * USV_NOBS; i += kBlock) {
      obad |= (uint32_t)(sobs[i] != sobs[i]);
      bst(R, w.obs, obase + (uint32_t)i * 4u, sobs[i]);
    }
  } else {
    for (int i = tid; i < rows * USV_NOBS; i += kBlock)
      if (keep[i / USV_NOBS]) {
        obad |= (uint32_t)(sobs[i] != sobs[i]);
        bst(R, w.obs, obase + (uint32_t)i * 4u, sobs[i]);
      }
  }
  if (c.nan_probe) nan_report(&b.ctl[USV_CTL_NAN_FLAG], obad ? USV_NAN_OBS : 0u);
  // ---- the step has consumed the Nones (:361, :448, USV_task_rewards.py:450): marked here,
  // promoted to the POT/PEN/REW_VALID flags by the next usv_reset, so the flags never change
  // while a step kernel that reads them runs ----
  if (blockIdx.x == 0 && tid == 0) b.ctl[USV_CTL_STEPPED] = 1;
}


// usv_env_step_late: the potential-dependent reward of the envs reset this step, once their fields
// exist (after usv_env_step_part(.., 3) and the field kernels): the stashed potential-independent terms,
// the field sample at the stashed position, reward_tail with prev_potential None (a reset env), the
// reward, prev_pot and the reward sums -- the operations part 0 runs for these envs, in the same order.
#ifndef USV_LATE_GRID
#define USV_LATE_GRID 256
#endif
constexpr int kLateGrid = USV_LATE_GRID;
__global__ __launch_bounds__(64) void k_env_reward_late(usv_cfg_t c, usv_bufs_t b) {
  const int n = b.n;
  const float cell = (float)((double)c.map_size / USV_GRID);
  const float inv_r = (float)(1.0 / (double)c.influence_radius);
  const float inv_safe = 1.0f / c.safe_radius;
  const double cell_d = (double)c.map_size / USV_GRID;
  const float g_start = (float)(-(double)c.map_size / 2 + cell_d / 2), g_end = (float)((double)c.map_size / 2 - cell_d / 2);
  const GridK gk{g_start, g_end, (g_end - g_start) / (float)(USV_GRID - 1), b.grid_lin};
  const int count = min(b.ctl[USV_CTL_RESET_COUNT], n);
  // slots spread thinly over many one-wave workgroups (lane l of workgroup g takes slot g + G l, ...): every
  // lane's loads are gathers from scattered envs, so a wave with few active lanes issues them in few cycles
  // and every CU takes a share (64 consecutive slots per wave put ~74 x 64 scattered lines on one CU)
  const int G = (int)gridDim.x;
  for (int slot = (int)blockIdx.x + G * (int)threadIdx.x; slot < count; slot += G * (int)blockDim.x) {
    const int e = b.reset_ids[slot];
    float st[USV_RSTASH_ROWS];
#pragma unroll
    for (int q = 0; q < USV_RSTASH_ROWS; ++q) st[q] = b.rstash[(size_t)q * n + e];
    const RewardPre rp{st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8], st[9], st[10], st[11]};
    const FieldTaps taps = field_taps(b.field + (size_t)e * USV_FIELD_STRIDE, b.fnorm + (size_t)e * USV_FNORM,
                                      c.map_size, st[12], st[13]);
    float2 obs_c[USV_NOBST];
#pragma unroll
    for (int o = 0; o < USV_NOBST; ++o)
      obs_c[o] = make_float2(b.obst[(size_t)(2 * o) * n + e], b.obst[(size_t)(2 * o + 1) * n + e]);
    const RewardOut ro = reward_tail(c, rp, field_blend(c, taps, [&](int o) { return obs_c[o]; }, gk, cell, inv_r, inv_safe),
                                     true, 0.f);
    b.prev_pot[e] = ro.pot;
    b.rew[e] = ro.rew;
    if (c.stats_on) {
      const float add[8] = {ro.total, ro.dist_r, ro.align_r, ro.shaping, ro.turn_haz, ro.danger,
                            (float)(ro.danger > 0.5f), ro.gate_pos};
      constexpr int key[8] = {ST_TOTAL_REWARD, ST_DISTANCE_REWARD, ST_ALIGNMENT_REWARD, ST_POTENTIAL_SHAPING_REWARD,
                              ST_TURN_HAZARD_PENALTY, ST_DANGER_MEAN, ST_DANGER_HI_RATE, ST_G_GATE_MEAN};
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        float *p = b.stats + (size_t)key[q] * n + e;
        *p = *p + add[q];
      }
    }
    if (c.nan_probe && nonfinite(ro.rew)) atomicOr(&b.ctl[USV_CTL_NAN_FLAG], (int)USV_NAN_REWARD);
  }
}

// ------------------------------------------------------------------------
// GoToPose / TrackXYOVelocity control step.  The action map, the substeps, the observed state, the
// penalties, the NaN probe's action / state bits, the state statistics and the privileged tail are the functions
// the CaptureXY step calls (action_map, integrate_substeps, observed_position / observed_motion,
// put_velocity_columns, step_penalties, nan_bits_actions_state, state_stats, write_priv_tail); the task
// part follows GoToPoseTask (tasks/USV/USV_go_to_pose.py:89-209) and
// TrackXYOVelocityTask (USV_track_xyo_velocity.py:75-166) with their rewards
// (USV_task_rewards.py:160-249, 328-393).  Glue where the reference cannot run
// these tasks: the task_data block is the Core layout's 20 columns
// (unwritten columns 0), update_kills(step) is the task's own, the reward is
// task.compute_reward(current_state, actions) + penalties as calculate_metrics
// (USV_Virtual.py:1628-1652) does for every task.
// The same template carries GoToXY, KeepXY and TrackXYVelocity (USV_go_to_xy.py:96-218, USV_keep_xy.py:92-179,
// USV_track_xy_velocity.py:76-128; rewards USV_task_rewards.py:117-153, 270-325): three task columns (two for
// TrackXYVelocity), no third target component (tgt_h may be NULL), one launch.  Reproduced as the code runs, not as
// its comments read: GoToXY's previous distance survives resets and the reset envs' distance reward is zeroed; its
// boundary penalty reaches the episode sums only; KeepXY never increments its goal counter; GoToXY / KeepXY kill
// at goal_cnt >= kill_after, TrackXYVelocity at > (usv_cfg_t.kill_after_ge).  Every non-CaptureXY kind takes
// Penalties.penalize_action_variation (see p_actv below).
// TrackXYOVelocity's angular error is reduced over ALL envs
// (torch.square(err).sum(-1) of a 1-D tensor, :121-123), so its step is two
// launches: this kernel writes per-block partial sums, k_track_finish completes.
// ------------------------------------------------------------------------
__device__ __forceinline__ float task_term(int mode, float x, float coeff) {
  if (mode == 0) return 1.0f / (1.0f + x);
  if (mode == 1) return 1.0f / (1.0f + x * x);
  return usv_exp(-x / coeff);
}

template <int kKind, bool kStats, bool kInj>
__global__ __launch_bounds__(kBlock) void k_env_step_task(StepCfg ck, usv_bufs_t b,
                                                          const float *__restrict__ actions,
                                                          const float *__restrict__ lut, float bias, uint64_t seed,
                                                          uint64_t step, const float *__restrict__ inj) {
  __shared__ float sobs[kBlock * USV_NOBS];
  __shared__ float sred[kBlock / 64];
  const usv_cfg_t &c = ck.c;
  const StepK &K = ck.K;
  const int n = b.n;
  const int tid = threadIdx.x;
  const int e = blockIdx.x * kBlock + tid;
  const int ec = min(e, n - 1);
  const bool mine = e < n;
  const size_t nn = (size_t)n;
  step = step_of(b, step);
  bias = bias_of(c, b, bias);
  const bool pen_valid = b.ctl[USV_CTL_PEN_VALID] != 0;
  float *obs = sobs + tid * USV_NOBS;
  const float clip = c.clip_obs;
  auto put = [&](int q, float v) { obs[q] = clampt(v, -clip, clip); };
  // ---- loads ----
  const float2 a2 = reinterpret_cast<const float2 *>(actions)[ec];
  const bool was_reset = b.just_reset[ec] != 0;
  BodyState s{b.px[ec], b.py[ec], b.yaw[ec], b.vx[ec], b.vy[ec], b.wz[ec], b.fl[ec], b.fr[ec]};
  const float m = b.mass[ec], k_iz = b.k_iz[ec], k_drag = b.k_drag[ec];
  const float thr_l = b.thr_l[ec], thr_r = b.thr_r[ec];
  const float comx = b.com_x[ec], comy = b.com_y[ec], comz = b.com_z[ec];
  SubstepIn in;
  in.damp = Damping{c.lin_damp[0], c.lin_damp[1], c.lin_damp[2], c.quad_damp[0], c.quad_damp[1], c.quad_damp[2]};
  if (b.lin_damp)
    in.damp = Damping{b.lin_damp[ec], b.lin_damp[nn + ec], b.lin_damp[2 * nn + ec],
                      b.quad_damp[ec], b.quad_damp[nn + ec], b.quad_damp[2 * nn + ec]};
  in.orgx = 0.f;
  in.orgy = 0.f;
  const bool has_dist = b.dist != nullptr;
  if (has_dist) {
#pragma unroll
    for (int q = 0; q < USV_NDIST; ++q) in.dp[q] = b.dist[q * nn + ec];
    if (b.env_org) { in.orgx = b.env_org[ec]; in.orgy = b.env_org[nn + ec]; }
  }
  const int progress0 = b.progress[ec], goal_cnt0 = b.goal_cnt[ec];
  constexpr bool kHasH = kKind == USV_TASK_GO_TO_POSE || kKind == USV_TASK_TRACK_XYO;   // the kinds with a tgt_h
  const float tgx = b.tgt_x[ec], tgy = b.tgt_y[ec], tgh = kHasH ? b.tgt_h[ec] : 0.f;
  const float prev_pd = b.prev_dist[ec], prev_wz_mem = b.prev_wz[ec];
  // Penalties.prev_actions as its action sum (penalize_action_variation); never cleared at a reset
  const float prev_asum = c.pen_actv_kind ? b.prev_head[ec] : 0.f;
  const bool rew_valid = b.ctl[USV_CTL_REW_VALID] != 0;
  // a reset env's first substep: the pre-reset inputs usv_reset kept
  in.stl = c.stale_root && was_reset;
  in.st_ub = in.st_vb = in.st_rb = in.st_px = in.st_py = 0.f;
  if (in.stl) {
    in.st_ub = b.stale[USV_STALE_UB * nn + ec];
    in.st_vb = b.stale[USV_STALE_VB * nn + ec];
    in.st_rb = b.stale[USV_STALE_RB * nn + ec];
    in.st_px = b.stale[USV_STALE_PX * nn + ec];
    in.st_py = b.stale[USV_STALE_PY * nn + ec];
  }
  float sums[USV_NSTAT];
  if (kStats) {
#pragma unroll
    for (int q = 0; q < USV_NSTAT; ++q) sums[q] = b.stats[q * nn + ec];
  }
  float u[USV_NU_STEP];
  if (kInj) {
#pragma unroll
    for (int i = 0; i < USV_NU_STEP; ++i) u[i] = inj[(size_t)ec * USV_NU_STEP + i];
  } else {
    philox_u4(seed, (uint32_t)e, step, 0u, u);
    if (c.pos_noise_on || c.act_noise_on) philox_u4(seed, (uint32_t)e, step, 1u, u + 4);
    else u[4] = u[5] = u[6] = u[7] = 0.f;
  }
  // ---- the shared step: action map, substeps (the LUT read is this kernel's: global memory) ----
  const ActionMap am = action_map(c, K, a2, was_reset, bias, u);
  const float cmd0 = am.cmd0, cmd1 = am.cmd1;
  in.lut0 = lut[am.i0];
  in.lut1 = lut[USV_LUT_N + am.i1];
  in.m = m; in.k_iz = k_iz; in.k_drag = k_drag; in.thr_l = thr_l; in.thr_r = thr_r; in.comy = comy;
  integrate_substeps(c, in, has_dist, s);
  if (mine) {
    b.px[e] = s.px; b.py[e] = s.py; b.yaw[e] = s.yaw; b.vx[e] = s.vx; b.vy[e] = s.vy; b.wz[e] = s.wz;
    b.fl[e] = s.fl; b.fr[e] = s.fr;
  }
  {   // the rest of the step reads its config afresh (see StepCfg)
  const StepCfg ck2 = step_cfg_reload();
  const usv_cfg_t &c = ck2.c;
  const StepK &K = ck2.K;
  // ---- post_physics_step: progress, update_state noise (USV_Virtual.py:771-813) ----
  const int progress = progress0 + 1;
  const float2 pn = observed_position(c, K, u, s.px, s.py);
  const ObservedMotion om = observed_motion(c, K, u, s);
  const float pxn = pn.x, pyn = pn.y, vxn = om.vxn, vyn = om.vyn, wzn = om.wzn, hs = om.hs, hc = om.hc;
  // ---- Core.update_observation_tensor (USV_core.py:55-121) ----
  put_velocity_columns(c, om, put);
#pragma unroll
  for (int q = 3; q < USV_NOBS - 10; ++q) obs[q] = 0.f;   // task_data columns no task writes
  const int pa = USV_NOBS_BASE - 2;
  if (c.priv_dim == 4) { obs[29] = 0.f; obs[30] = 0.f; obs[31] = 0.f; obs[32] = 0.f; }   // input padding
  put(pa, am.prev_cmd0);
  put(pa + 1, am.prev_cmd1);
  write_priv_tail(c, K, m, comx, comy, comz, k_drag, thr_l, thr_r, k_iz, put);
  {
  const StepCfg ck3 = step_cfg_reload();
  const usv_cfg_t &c = ck3.c;
  const StepK &K = ck3.K;
  const StepPenalties pen = step_penalties(c, am, om, pen_valid, prev_wz_mem);
  // penalize_action_variation (:497-506): sum(actions) - sum(prev_actions).  With penalties_use_thrust_u the
  // reference hands compute_penalty its persistent thrust_cmds_unit tensor (USV_Virtual.py:1095, 1634-1639) and
  // keeps that same object as prev_actions (:515), so the difference is identically 0; without it the actions
  // are a fresh clone every step (:1050-1052) and the difference is the real one, across resets too
  float p_actv = 0.f;
  const float asum = cmd0 + cmd1;
  if (c.pen_actv_kind) {
    const float dsum = (c.pen_use_u || !pen_valid) ? 0.f : asum - prev_asum;
    p_actv = pen_scalar(c.pen_actv_kind, c.pen_actv_k, c.pen_actv_x0, c.pen_actv_c, dsum);
  }
  const float pen_sum = c.pen_actv_kind ? pen.sum + p_actv : pen.sum;
  const int tout = progress >= c.max_episode_length - 1;
  float t_add[5];
  t_add[4] = 0.f;
  float overall = 0.f;
  int goal_cnt = goal_cnt0, die = 0;
  if (kKind == USV_TASK_GO_TO_XY || kKind == USV_TASK_KEEP_XY) {
    // GoToXYTask / KeepXYTask.get_state_observations (USV_go_to_xy.py:96-111, USV_keep_xy.py:92-105)
    const float ex = tgx - pxn, ey = tgy - pyn;
    const float theta = usv_atan2(hs, hc);
    const float beta = usv_atan2(ey, ex);
    const float alpha = fmodf((beta - theta) + USV_PI_F, USV_2PI_F) - USV_PI_F;
    float sa, ca;
    usv_sincos(alpha, &sa, &ca);
    put(3, ca);
    put(4, sa);
    put(5, tnorm2(ex, ey));
    // compute_reward (USV_go_to_xy.py:129-180, USV_keep_xy.py:123-141)
    const float pdist = sqrtf(ex * ex + ey * ey);
    const float bdist = pdist - c.kill_dist;
    const float bpen = -usv_exp(-bdist / 0.25f) * c.boundary_cost;   // episode sums only, never the reward
    if (kKind == USV_TASK_GO_TO_XY) {
      const int gir = pdist < c.position_tolerance;
      goal_cnt = goal_cnt0 * gir + gir;
      // GoToXYReward.compute_reward (USV_task_rewards.py:117-153): the previous error is a per-env value that
      // no reset clears; the task zeroes the distance reward of the envs reset this step (:161)
      const float prev_err = rew_valid ? prev_pd : pdist;
      float dist_r;
      if (c.reward_mode == 0) dist_r = c.position_scale * (prev_err - pdist);
      else if (c.reward_mode == 1) dist_r = c.position_scale * (prev_err * prev_err - pdist * pdist);
      else dist_r = c.position_scale * (usv_exp(-pdist / c.exp_coeff) - usv_exp(-prev_err / c.exp_coeff));
      if (was_reset) dist_r = 0.f;
      const float herr = fabsf(alpha), h2 = herr * herr;
      const float align_r = c.align_la1 * (usv_exp(c.align_la2 * (h2 * h2)) + usv_exp(c.align_la3 * h2));
      if (mine) b.prev_dist[e] = pdist;
      overall = ((dist_r + align_r) + (float)goal_cnt * c.goal_reward) + c.time_reward;
      t_add[0] = dist_r; t_add[1] = align_r; t_add[2] = pdist; t_add[3] = bpen; t_add[4] = bdist;
    } else {
      // KeepXYReward.compute_reward (:270-287); _goal_reached is never incremented (goal_cnt stays 0)
      overall = task_term(c.tk_mode[0], pdist, c.tk_coeff[0]);
      t_add[0] = overall; t_add[1] = pdist; t_add[2] = bpen; t_add[3] = bdist;
    }
    // update_kills (USV_go_to_xy.py:182-218, USV_keep_xy.py:143-179)
    const float kd = c.curriculum_on ? (float)curriculum_lerp(c, ref_step_of(c, b, step, 5), c.cur_kill_dist,
                                                              c.kill_dist_d)
                                     : c.kill_dist;
    die = (pdist > kd) || (c.kill_after_ge ? goal_cnt >= c.kill_after_n : goal_cnt > c.kill_after_n);
  } else if (kKind == USV_TASK_TRACK_XY) {
    // TrackXYVelocityTask.get_state_observations / compute_reward / update_kills (USV_track_xy_velocity.py:76-128)
    const float lex = tgx - vxn, ley = tgy - vyn;
    put(3, lex);
    put(4, ley);
    const float pos_d = sqrtf(pxn * pxn + pyn * pyn);
    const float lin_d = sqrtf(lex * lex + ley * ley);
    const int gir = lin_d < c.tk_tol[0];
    goal_cnt = goal_cnt0 * gir + gir;
    overall = task_term(c.tk_mode[0], lin_d, c.tk_coeff[0]);   // TrackXYVelocityReward (:308-325)
    die = (pos_d > c.kill_dist) || (c.kill_after_ge ? goal_cnt >= c.kill_after_n : goal_cnt > c.kill_after_n);
    t_add[0] = overall; t_add[1] = lin_d; t_add[2] = 0.f; t_add[3] = 0.f;
  } else if (kKind == USV_TASK_GO_TO_POSE) {
    // GoToPoseTask.get_state_observations (:89-130)
    const float ex = tgx - pxn, ey = tgy - pyn;
    const float theta = usv_atan2(hs, hc);
    const float beta = usv_atan2(ey, ex);
    const float alpha = fmodf((beta - theta) + USV_PI_F, USV_2PI_F) - USV_PI_F;
    const float hraw = fmodf((tgh - theta) + USV_PI_F, USV_2PI_F) - USV_PI_F;
    float shr, chr;
    usv_sincos(hraw, &shr, &chr);
    const float herr = usv_atan2(shr, chr);
    float sa, ca, sh, ch;
    usv_sincos(alpha, &sa, &ca);
    usv_sincos(herr, &sh, &ch);
    put(3, ca);
    put(4, sa);
    put(5, tnorm2(ex, ey));
    put(6, ch);
    put(7, sh);
    // compute_reward (:134-181)
    const float pdist = sqrtf(ex * ex + ey * ey);
    const float hdist = fabsf(herr);
    const float prog_r = 2.0f * clampt(prev_pd - pdist, -2.0f, 2.0f);
    if (mine) b.prev_dist[e] = pdist;
    const float speed = tnorm2(vxn, vyn);
    const int gir = (pdist < c.position_tolerance) & (speed < 0.1f);
    goal_cnt = goal_cnt0 * gir + gir;
    // GoToPoseReward.compute_reward (USV_task_rewards.py:190-233)
    const float hw = 1.0f - 1.0f / (1.0f + usv_exp(-c.sig_gain * (pdist - 2.0f)));
    const float pos_r = c.tk_scale[0] * task_term(c.tk_mode[0], pdist, c.tk_coeff[0]);
    const float head_r = hw * c.tk_scale[1] * task_term(c.tk_mode[1], hdist, c.tk_coeff[1]);
    const float act_pen = -0.05f * (fabsf(cmd0) + fabsf(cmd1));
    overall = (((pos_r + head_r) + prog_r) + 2.0f * (float)gir) + act_pen;
    // update_kills (:183-209): kill_dist (the curriculum's at the step after calculate_metrics) / goal counter
    const float kd = c.curriculum_on ? (float)curriculum_lerp(c, ref_step_of(c, b, step, 5), c.cur_kill_dist,
                                                              c.kill_dist_d)
                                     : c.kill_dist;
    die = (pdist > kd) || (goal_cnt >= c.kill_after_n);
    t_add[0] = pos_r; t_add[1] = head_r; t_add[2] = pdist; t_add[3] = speed;   // update_statistics (:211-219)
  } else {
    // TrackXYOVelocityTask.get_state_observations (:75-101)
    const float lex = tgx - vxn, ley = tgy - vyn, aerr = tgh - wzn;
    put(3, lex);
    put(4, ley);
    put(5, aerr);
    // compute_reward (:103-141): the angular part waits for the all-env sum
    const float pos_d = sqrtf(pxn * pxn + pyn * pyn);
    const float lin_d = sqrtf(lex * lex + ley * ley);
    const float lin_r = task_term(c.tk_mode[0], lin_d, c.tk_coeff[0]) * c.tk_scale[0];
    float part = mine ? aerr * aerr : 0.f;
    part = wave_sum(part);
    if ((tid & 63) == 0) sred[tid >> 6] = part;
    float *ts = b.task_scratch;
    if (mine) {
      ts[USV_TS_LIN_REW * nn + e] = lin_r;
      ts[USV_TS_PEN * nn + e] = pen_sum;
      ts[USV_TS_LIN_OK * nn + e] = (float)(lin_d < c.tk_tol[0]);
      ts[USV_TS_POS_KILL * nn + e] = (float)(pos_d > c.kill_dist);
    }
    t_add[0] = lin_r; t_add[1] = lin_d; t_add[2] = 0.f; t_add[3] = 0.f;
  }
  if (mine) {
    b.progress[e] = progress;
    b.prev_cmd[e] = am.prev_cmd0;
    b.prev_cmd[nn + e] = am.prev_cmd1;
    b.prev_wz[e] = wzn;
    if (c.pen_actv_kind) b.prev_head[e] = asum;
    b.just_reset[e] = 0;
    if (kKind != USV_TASK_TRACK_XYO) {   // TrackXYOVelocity: k_track_finish
      const float rew = overall + pen_sum;
      const int rb = c.fixed_horizon_eval ? tout : (tout ? 1 : die);
      b.goal_cnt[e] = goal_cnt;
      b.rew[e] = rew;
      b.reset_buf[e] = rb;
      b.dones[e] = rb;
    }
    if (kStats) {
      const StateStats ss = state_stats(am, om);
      float add[USV_NSTAT];
#pragma unroll
      for (int q = 0; q < USV_NSTAT; ++q) add[q] = 0.f;
      add[0] = t_add[0]; add[1] = t_add[1]; add[2] = t_add[2]; add[3] = t_add[3]; add[4] = t_add[4];
      add[USV_ST_ACTION_VARIATION] = p_actv;
      add[ST_ANGULAR_VEL_PENALTY] = pen.p_ang;
      add[ST_ANGULAR_VEL_VARIATION_PENALTY] = pen.p_angv;
      add[ST_ENERGY_PENALTY] = pen.p_en;
#pragma unroll
      for (int q = 0; q < 6; ++q) add[kStateStatKey[q]] = ss.v[q];
#pragma unroll
      for (int q = 0; q < USV_NSTAT; ++q)
        if (q != ST_SUCCESS && q != ST_COLLISION && (kKind != USV_TASK_TRACK_XYO || (q != 2 && q != 3)))
          b.stats[q * nn + e] = sums[q] + add[q];
    }
  }
  __syncthreads();
  if (kKind == USV_TASK_TRACK_XYO && tid == 0) {
    float sblk = 0.f;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) sblk += sred[w];
    b.task_scratch[USV_TS_ROWS * nn + blockIdx.x] = sblk;
  }
  // ---- coalesced obs store ----
  const int row0 = blockIdx.x * kBlock;
  const int rows = min(kBlock, n - row0);
  float *ob = b.obs + (size_t)row0 * USV_NOBS;
  uint32_t obad = 0u;
  for (int i = tid; i < rows * USV_NOBS; i += kBlock) {
    obad |= (uint32_t)(sobs[i] != sobs[i]);
    ob[i] = sobs[i];
  }
  if (c.nan_probe) {   // clamped actions, the observed state, the reward (TrackXYO: k_track_finish), obs
    const uint32_t bits = nan_bits_actions_state(am, pn, om) |
                          ((kKind != USV_TASK_TRACK_XYO && nonfinite(overall + pen_sum)) ? USV_NAN_REWARD : 0u);
    nan_report(&b.ctl[USV_CTL_NAN_FLAG], (mine ? bits : 0u) | (obad ? USV_NAN_OBS : 0u));
  }
  if (blockIdx.x == 0 && tid == 0) b.ctl[USV_CTL_STEPPED] = 1;
  }
  }
}

// TrackXYOVelocity, phase 2: angular velocity distance over all envs, then the
// angular reward, goal counter, kills and dones of every env (:103-166)
template <bool kStats>
__global__ __launch_bounds__(kBlock) void k_track_finish(usv_cfg_t c, usv_bufs_t b, int nblk) {
  __shared__ float sred[kBlock];
  const int n = b.n;
  const size_t nn = (size_t)n;
  const int tid = threadIdx.x;
  const float *part = b.task_scratch + USV_TS_ROWS * nn;
  float acc = 0.f;
  for (int i = tid; i < nblk; i += kBlock) acc += part[i];   // fixed order: every block gets the same sum
  sred[tid] = acc;
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if (tid < w) sred[tid] += sred[tid + w];
    __syncthreads();
  }
  const float ang_d = sqrtf(sred[0]);
  const int e = blockIdx.x * kBlock + tid;
  if (c.nan_probe) {   // the reward of every env (one wave-uniform probe ahead of the per-env tail)
    const int ec = min(e, n - 1);
    const float *ts = b.task_scratch;
    const float ang_r = task_term(c.tk_mode[1], ang_d, c.tk_coeff[1]) * c.tk_scale[1];
    const float rew = (ts[USV_TS_LIN_REW * nn + ec] + ang_r) + ts[USV_TS_PEN * nn + ec];
    nan_report(&b.ctl[USV_CTL_NAN_FLAG], (e < n && nonfinite(rew)) ? USV_NAN_REWARD : 0u);
  }
  if (e >= n) return;
  const float *ts = b.task_scratch;
  const int ang_ok = ang_d < c.tk_tol[1];
  const int gir = (int)ts[USV_TS_LIN_OK * nn + e] * ang_ok;
  const int goal_cnt = b.goal_cnt[e] * gir + gir;
  const float ang_r = task_term(c.tk_mode[1], ang_d, c.tk_coeff[1]) * c.tk_scale[1];
  const float rew = (ts[USV_TS_LIN_REW * nn + e] + ang_r) + ts[USV_TS_PEN * nn + e];
  const int die = (ts[USV_TS_POS_KILL * nn + e] != 0.f) || (goal_cnt > c.kill_after_n);
  const int tout = b.progress[e] >= c.max_episode_length - 1;
  const int rb = c.fixed_horizon_eval ? tout : (tout ? 1 : die);
  b.goal_cnt[e] = goal_cnt;
  b.rew[e] = rew;
  b.reset_buf[e] = rb;
  b.dones[e] = rb;
  if (kStats) {
    b.stats[2 * nn + e] += ang_r;
    b.stats[3 * nn + e] += ang_d;
  }
}

// planar forces only (parity with Hydrodynamics.ComputeHydrodynamicsEffects)
// Hydrostatic wrench (usv_hydrostatics): one thread per env, the reference's operation order.
__global__ void k_hydrostatics(usv_hydro_t h, int n, const float *__restrict__ quat, const float *__restrict__ root_z,
                               float *__restrict__ volume, float *__restrict__ euler, float *__restrict__ wrench) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const float4 q = reinterpret_cast<const float4 *>(quat)[e];
  const float w = q.x, x = q.y, y = q.z, z = q.w;
  // USVVirtual.update_state (USV_Virtual.py:791-798)
  const float high = clampt(h.zero_height - root_z[e], 0.f, h.zero_height + 20.0f);
  const float vol = clampt(high * h.waterplane_area, 0.f, h.max_volume);
  // get_euler_angles (:815-835): the rotation-matrix entries as the reference forms them
  const float r00 = 1.0f - 2.0f * (y * y) - 2.0f * (z * z);
  const float r10 = 2.0f * x * y + 2.0f * w * z;
  const float r20 = 2.0f * x * z - 2.0f * w * y;
  const float r21 = 2.0f * y * z + 2.0f * w * x;
  const float r22 = 1.0f - 2.0f * (x * x) - 2.0f * (y * y);
  const float roll = atan2f(r21, r22), pitch = asinf(-r20), yaw = atan2f(r10, r00);
  // compute_archimedes_metacentric_global (Hydrostatics.py:63-98); the Python scalars fold first
  const float fz = (-h.water_density * h.gravity) * vol;
  const float tx = (-1.0f * h.metacentric_width) * (sinf(roll) * h.avg_force);
  const float ty = (-1.0f * h.metacentric_length) * (sinf(pitch) * h.avg_force);
  // _local (:100-133): R = quaternion_to_matrix(q) (pytorch3d, real first); F_local = R^T (0, 0, fz)
  const float two_s = 2.0f / (((w * w + x * x) + y * y) + z * z);
  const float R20 = two_s * (x * z - y * w), R21 = two_s * (y * z + x * w), R22 = 1.0f - two_s * (x * x + y * y);
  float *out = wrench + (size_t)e * 6;
  out[0] = R20 * fz;
  out[1] = R21 * fz;
  out[2] = R22 * fz;
  out[3] = tx * h.amplify_torque;   // torque not rotated (:123)
  out[4] = ty * h.amplify_torque;
  out[5] = 0.0f * h.amplify_torque;
  volume[e] = vol;
  euler[(size_t)e * 3 + 0] = roll;
  euler[(size_t)e * 3 + 1] = pitch;
  euler[(size_t)e * 3 + 2] = yaw;
}

__global__ void k_forces(usv_cfg_t c, usv_bufs_t b, float *__restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = b.n;
  if (e >= n) return;
  const QuatRot qr = usv_quat_rot(b.yaw[e]);   // R = quaternion_to_matrix(q(yaw)) (Hydrodynamics.py:209-217)
  const float sy_ = qr.S, cy_ = qr.C;
  const float vx = b.vx[e], vy = b.vy[e], wz = b.wz[e];
  float ub = cy_ * vx + sy_ * vy, vb = -sy_ * vx + cy_ * vy;
  if (c.current_on) {   // relative to the water (Hydrodynamics.py:224-237)
    ub = ub - (cy_ * c.flow_vel[0] + sy_ * c.flow_vel[1]);
    vb = vb - (-sy_ * c.flow_vel[0] + cy_ * c.flow_vel[1]);
  }
  Damping d{c.lin_damp[0], c.lin_damp[1], c.lin_damp[2], c.quad_damp[0], c.quad_damp[1], c.quad_damp[2]};
  if (b.lin_damp)
    d = Damping{b.lin_damp[e], b.lin_damp[n + e], b.lin_damp[2 * n + e],
                b.quad_damp[e], b.quad_damp[n + e], b.quad_damp[2 * n + e]};
  // the damping expression the step kernels integrate
  const Drag3 D = drag_coeffs(c, d, c.use_drag_scale ? b.k_drag[e] : 1.0f, ub, vb, wz);
  const float fl = b.fl[e], fr = b.fr[e], comy = b.com_y[e];
  out[3 * e] = fl + fr + (-D.D0 * ub);
  out[3 * e + 1] = -D.D1 * vb;
  out[3 * e + 2] = -(c.thr_y - comy) * fl + (c.thr_y + comy) * fr + (-D.D2 * wz);
}

// ---- host side of the step launch ----
// k_env_step's per-env arrays: where each lies, its size, the StepWin member that takes its window offset, its
// row in the canonical slab (include/usv_hip.h USV_SLAB_*) and whether the step can run without it
struct StepArr {
  const void *p;
  size_t bytes;
  uint32_t StepWin::*off;
  int row;
  bool required = true;
};
constexpr int kStepArrs = 39;
std::array<StepArr, kStepArrs> step_arrays(const usv_cfg_t &c, const usv_bufs_t &b) {
  const size_t n = (size_t)b.n, f = n * 4;
  // quad_damp is read with lin_damp only; stats / stale when the config turns them on
  const bool dr = b.lin_damp != nullptr, st = c.stats_on != 0, sr = c.stale_root != 0;
  return {{{b.px, f, &StepWin::px, USV_SLAB_STATE}, {b.py, f, &StepWin::py, USV_SLAB_STATE + 1},
          {b.yaw, f, &StepWin::yaw, USV_SLAB_STATE + 2}, {b.vx, f, &StepWin::vx, USV_SLAB_STATE + 3},
          {b.vy, f, &StepWin::vy, USV_SLAB_STATE + 4}, {b.wz, f, &StepWin::wz, USV_SLAB_STATE + 5},
          {b.fl, f, &StepWin::fl, USV_SLAB_STATE + 6}, {b.fr, f, &StepWin::fr, USV_SLAB_STATE + 7},
          {b.mass, f, &StepWin::mass, USV_SLAB_PARAMS}, {b.com_x, f, &StepWin::com_x, USV_SLAB_PARAMS + 1},
          {b.com_y, f, &StepWin::com_y, USV_SLAB_PARAMS + 2}, {b.com_z, f, &StepWin::com_z, USV_SLAB_PARAMS + 3},
          {b.k_drag, f, &StepWin::k_drag, USV_SLAB_PARAMS + 4}, {b.thr_l, f, &StepWin::thr_l, USV_SLAB_PARAMS + 5},
          {b.thr_r, f, &StepWin::thr_r, USV_SLAB_PARAMS + 6}, {b.k_iz, f, &StepWin::k_iz, USV_SLAB_PARAMS + 7},
          {b.lin_damp, 3 * f, &StepWin::lin_damp, USV_SLAB_LIN_DAMP, false},
          {dr ? b.quad_damp : nullptr, 3 * f, &StepWin::quad_damp, USV_SLAB_QUAD_DAMP, dr},
          {b.tgt_x, f, &StepWin::tgt_x, USV_SLAB_TGT}, {b.tgt_y, f, &StepWin::tgt_y, USV_SLAB_TGT + 1},
          {b.obst, 2 * USV_NOBST * f, &StepWin::obst, USV_SLAB_OBST},
          {b.prev_cmd, 2 * f, &StepWin::prev_cmd, USV_SLAB_PREV_CMD},
          {b.prev_dist, f, &StepWin::prev_dist, USV_SLAB_HIST},
          {b.prev_head, f, &StepWin::prev_head, USV_SLAB_HIST + 1},
          {b.prev_pot, f, &StepWin::prev_pot, USV_SLAB_HIST + 2}, {b.prev_wz, f, &StepWin::prev_wz, USV_SLAB_HIST + 3},
          {b.goal_cnt, f, &StepWin::goal_cnt, USV_SLAB_IBUF}, {b.progress, f, &StepWin::progress, USV_SLAB_IBUF + 1},
          {b.reset_buf, f, &StepWin::reset_buf, USV_SLAB_IBUF + 2},
          {b.done_succ, f, &StepWin::done_succ, USV_SLAB_IBUF + 3},
          {b.done_coll, f, &StepWin::done_coll, USV_SLAB_IBUF + 4},
          {b.just_reset, n, &StepWin::just_reset, USV_SLAB_JUST_RESET},
          {st ? b.stats : nullptr, USV_NSTAT * f, &StepWin::stats, USV_SLAB_STATS, st},
          {b.obs, USV_NOBS * f, &StepWin::obs, USV_SLAB_OBS}, {b.rew, f, &StepWin::rew, USV_SLAB_REW},
          {b.dones, 2 * f, &StepWin::dones, USV_SLAB_DONES},
          {b.dist, USV_NDIST * f, &StepWin::dist, USV_SLAB_DIST, false},
          {b.dist ? b.env_org : nullptr, 2 * f, &StepWin::env_org, USV_SLAB_ENV_ORG, false},
          {sr ? b.stale : nullptr, USV_STALE_ROWS * f, &StepWin::stale, USV_SLAB_STALE, sr}}};
}

// byte offsets of the step kernel's per-env arrays inside one window; status 2 when
// they span 2 GiB or more (allocate them from one slab, as tasks/usv_virtual.py does)
int step_window(const usv_cfg_t &c, const usv_bufs_t &b, const char **base, StepWin *w) {
  const auto arr = step_arrays(c, b);
  uintptr_t lo = UINTPTR_MAX, hi = 0;
  for (const StepArr &a : arr) {
    if (!a.p) {
      if (a.required) return 1;
      continue;
    }
    lo = std::min(lo, (uintptr_t)a.p);
    hi = std::max(hi, (uintptr_t)a.p + a.bytes);
  }
  if (hi - lo >= 0x7FFFFFFFull) return 2;
  for (const StepArr &a : arr) w->*a.off = a.p ? (uint32_t)((uintptr_t)a.p - lo) : 0u;
  w->n4 = (uint32_t)(4 * (size_t)b.n);
  w->bytes = (uint32_t)(hi - lo);
  *base = (const char *)lo;
  return 0;
}

// kShift when every array the step kernel touches sits at its canonical slab row (include/usv_hip.h USV_SLAB_*)
// with 2^kShift-byte rows, 2^kShift the next power of two >= 4 n; -1 otherwise (the general window path)
int fixed_slab_shift(const usv_cfg_t &c, const usv_bufs_t &b) {
  int sh = 8;
  while ((1ull << sh) < 4ull * (unsigned long long)b.n) ++sh;
  if (sh < kFixedShiftMin || sh > kFixedShiftMax || !b.px) return -1;
  const char *base = reinterpret_cast<const char *>(b.px);
  const size_t rb = (size_t)1 << sh;
  for (const StepArr &a : step_arrays(c, b)) {
    if (!a.p) {
      if (a.required) return -1;
      continue;
    }
    if (reinterpret_cast<const char *>(a.p) != base + (size_t)a.row * rb) return -1;
  }
  return sh;
}

// k_env_step_task<kind, stats on, injected uniforms>; nullptr for a kind it does not carry
using TaskKern = void (*)(StepCfg, usv_bufs_t, const float *, const float *, float, uint64_t, uint64_t, const float *);
template <int kKind>
TaskKern task_kern_of(bool st, bool ij) {
  return st ? (ij ? k_env_step_task<kKind, true, true> : k_env_step_task<kKind, true, false>)
            : (ij ? k_env_step_task<kKind, false, true> : k_env_step_task<kKind, false, false>);
}
TaskKern task_kern(int kind, bool st, bool ij) {
  switch (kind) {
    case USV_TASK_GO_TO_POSE: return task_kern_of<USV_TASK_GO_TO_POSE>(st, ij);
    case USV_TASK_TRACK_XYO: return task_kern_of<USV_TASK_TRACK_XYO>(st, ij);
    case USV_TASK_GO_TO_XY: return task_kern_of<USV_TASK_GO_TO_XY>(st, ij);
    case USV_TASK_KEEP_XY: return task_kern_of<USV_TASK_KEEP_XY>(st, ij);
    case USV_TASK_TRACK_XY: return task_kern_of<USV_TASK_TRACK_XY>(st, ij);
    default: return nullptr;
  }
}

// any per-substep disturbance term on (then usv_bufs_t.dist must be set)
bool step_has_dist(const usv_cfg_t &c) { return c.fdist_on || c.tdist_on || c.current_on; }

float enc_centered_scale(float xmin, float xmax, float nominal) {
  double sc = std::fabs((double)xmin - nominal);
  if (std::fabs((double)xmax - nominal) > sc) sc = std::fabs((double)xmax - nominal);
  if (1e-6 > sc) sc = 1e-6;
  return (float)sc;
}
// host restatements of the reference's privileged-observation encoders (USV_Virtual.py:97-151)
float enc_centered_h(float x, float xmin, float xmax, float nominal) {
  const float s = enc_centered_scale(xmin, xmax, nominal);
  const float z = (x - nominal) / s;
  return z < -1.f ? -1.f : (z > 1.f ? 1.f : z);
}
float enc_minmax_h(float x, float xmin, float xmax) {
  if ((double)xmax - (double)xmin <= 1e-6) return 0.f;
  const float z = (x - xmin) / (float)((double)xmax - (double)xmin);
  const float y = 2.0f * z - 1.0f;
  return y < -1.f ? -1.f : (y > 1.f ? 1.f : y);
}

StepK step_constants(const usv_cfg_t &c) {
  StepK k{};
  k.cell = (float)((double)c.map_size / USV_GRID);
  k.inv_r = (float)(1.0 / (double)c.influence_radius);
  k.inv_safe = 1.0f / c.safe_radius;
  {
    const double cell_d = (double)c.map_size / USV_GRID;
    k.gstart = (float)(-(double)c.map_size / 2 + cell_d / 2);
    k.gend = (float)((double)c.map_size / 2 - cell_d / 2);
    k.gstep = (k.gend - k.gstart) / (float)(USV_GRID - 1);
  }
  k.act_rng = (float)((double)c.act_noise_max - (double)c.act_noise_min);
  k.pos_rng = (float)((double)c.pos_noise_max - (double)c.pos_noise_min);
  k.vel_rng = (float)((double)c.vel_noise_max - (double)c.vel_noise_min);
  k.head_rng = (float)((double)c.head_noise_max - (double)c.head_noise_min);
  k.mass_den = (float)(std::fabs((double)c.base_mass) > 1e-6 ? std::fabs((double)c.base_mass) : 1e-6);
  k.inv_mass_den = 1.0f / k.mass_den;
  for (int i = 0; i < 3; ++i) {
    k.com_div[i] = c.com_scale[i] + 1e-6f;
    k.inv_com_div[i] = 1.0f / k.com_div[i];
  }
  const float lo3[3] = {c.kdrag_min, c.thr_min, c.kiz_min}, hi3[3] = {c.kdrag_max, c.thr_max, c.kiz_max};
  for (int j = 0; j < 3; ++j) {
    k.enc_lo[j] = lo3[j];
    if (c.priv_mode == 1) {
      k.enc_r[j] = enc_centered_scale(lo3[j], hi3[j], c.priv_nominal);
      k.enc_ok[j] = 1;
    } else {
      k.enc_r[j] = (float)((double)hi3[j] - (double)lo3[j]);
      k.enc_ok[j] = ((double)hi3[j] - (double)lo3[j]) > 1e-6;
    }
    k.inv_enc_r[j] = k.enc_r[j] != 0.f ? 1.0f / k.enc_r[j] : 0.f;
  }
  k.inv_exp_coeff = c.exp_coeff != 0.f ? 1.0f / c.exp_coeff : 0.f;
  // privileged values of the "base" source: the same for every env
  float v[8];
  v[0] = c.mass_relative ? 0.f : c.base_mass;
  for (int i = 0; i < 3; ++i) v[1 + i] = c.com_scaled ? c.base_com[i] / (c.com_scale[i] + 1e-6f) : c.base_com[i];
  float kdv = 1.f, tl = 1.f, tr = 1.f, kz = 1.f;
  if (c.priv_mode == 2) {
    kdv = 0.5f * (c.kdrag_min + c.kdrag_max);
    tl = tr = c.couple_thr ? (1.0f - 0.5f * c.thr_rand) : 1.0f;
    kz = 0.5f * (c.kiz_min + c.kiz_max);
  }
  if (c.priv_mode == 1) {
    kdv = enc_centered_h(kdv, c.kdrag_min, c.kdrag_max, c.priv_nominal);
    tl = enc_centered_h(tl, c.thr_min, c.thr_max, c.priv_nominal);
    tr = enc_centered_h(tr, c.thr_min, c.thr_max, c.priv_nominal);
    kz = enc_centered_h(kz, c.kiz_min, c.kiz_max, c.priv_nominal);
  } else if (c.priv_mode == 2) {
    kdv = c.priv_drag_on ? enc_minmax_h(kdv, c.kdrag_min, c.kdrag_max) : 0.f;
    tl = c.priv_thr_on ? enc_minmax_h(tl, c.thr_min, c.thr_max) : 0.f;
    tr = c.priv_thr_on ? enc_minmax_h(tr, c.thr_min, c.thr_max) : 0.f;
    kz = c.priv_kiz_on ? enc_minmax_h(kz, c.kiz_min, c.kiz_max) : 0.f;
  }
  v[4] = kdv; v[5] = tl; v[6] = tr; v[7] = kz;
  for (int i = 0; i < 8; ++i) k.priv_base[i] = v[i];
  return k;
}

}  // namespace

extern "C" {

int usv_build_lut(const float *table_l21, const float *table_r21, int n_table, float *lut_dev, void *stream) {
  if (!table_l21 || !table_r21 || !lut_dev || n_table < 2) return 1;
  hipLaunchKernelGGL(k_build_lut, dim3((USV_LUT_N + 255) / 256), dim3(256), 0, (hipStream_t)stream, table_l21,
                     table_r21, n_table, lut_dev);
  USV_CHECK_LAUNCH();
  return 0;
}

int usv_reset_part(const usv_cfg_t *cfg, const usv_bufs_t *b, uint64_t seed, uint64_t step, const float *u_inject,
                   int part, void *stream) {
  if (!cfg || !b || b->n <= 0 || part < 0 || part > 2) return 1;
  if (b->scene && (b->n_scenes <= 0 || !b->scene_next || !b->scene_last || cfg->task_kind != USV_TASK_CAPTURE_XY))
    return 1;
  if (cfg->stale_root && !b->stale) return 1;   // the first substep's cached-state inputs have nowhere to go
  hipStream_t s = (hipStream_t)stream;
  const int grid = (b->n + kBlock - 1) / kBlock;
  if (part != 2) {
    // per-step scratch: reset count, field maxima, extras sums
    hipLaunchKernelGGL(k_step_begin, dim3(1), dim3(64), 0, s, *b, cfg->step_inc);
    USV_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_reset, dim3(grid), dim3(kBlock), 0, s, *cfg, *b, seed, step, u_inject);
    USV_CHECK_LAUNCH();
  }
  if (part != 1 && cfg->stats_on) {
    hipLaunchKernelGGL(k_extras_fold, dim3(1), dim3(kBlock), 0, s, *cfg, *b, grid);
    USV_CHECK_LAUNCH();
  }
  return 0;
}

int usv_reset(const usv_cfg_t *cfg, const usv_bufs_t *b, uint64_t seed, uint64_t step, const float *u_inject,
              void *stream) {
  return usv_reset_part(cfg, b, seed, step, u_inject, 0, stream);
}

int usv_env_step_part(const usv_cfg_t *cfg, const usv_bufs_t *b, const float *actions, const float *lut_dev,
                      float action_bias, uint64_t seed, uint64_t step, const float *u_inject, int part,
                      void *stream) {
  if (!cfg || !b || !actions || !lut_dev || b->n <= 0 || part < 0 || part > 3) return 1;
  if (part == 3 && (cfg->task_kind != USV_TASK_CAPTURE_XY || !b->rstash)) return 1;
  if (cfg->stale_root && !b->stale) return 1;   // a reset env's first substep reads usv_reset's cached inputs
  // CaptureXY samples the potential field from its parts (SDF tiles, cost rows, constants)
  if (cfg->task_kind == USV_TASK_CAPTURE_XY && (!b->field || !b->sdf || !b->fnorm)) return 7;
  if (cfg->priv_dim != 4 && cfg->priv_dim != 8) return 3;
  if (cfg->task_kind != USV_TASK_CAPTURE_XY) {
    // GoToPose / TrackXYOVelocity: no potential field, so no split step
    const int kind = cfg->task_kind;
    if (part != 0 || ((kind == USV_TASK_GO_TO_POSE || kind == USV_TASK_TRACK_XYO) && !b->tgt_h)) return 1;
    if (step_has_dist(*cfg) && !b->dist) return 4;
    if (cfg->task_kind == USV_TASK_TRACK_XYO && !b->task_scratch) return 1;
    const StepK k = step_constants(*cfg);
    const int grid = (b->n + kBlock - 1) / kBlock;
    hipStream_t s = (hipStream_t)stream;
    const bool st = cfg->stats_on != 0;
    const TaskKern kern = task_kern(kind, st, u_inject != nullptr);
    if (!kern) return 1;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, s, StepCfg{*cfg, k}, *b, actions, lut_dev, action_bias, seed,
                       step, u_inject);
    if (kind == USV_TASK_TRACK_XYO) {
      USV_CHECK_LAUNCH();
      hipLaunchKernelGGL(st ? k_track_finish<true> : k_track_finish<false>, dim3(grid), dim3(kBlock), 0, s, *cfg, *b,
                         grid);
    }
    USV_CHECK_LAUNCH();
    return 0;
  }
  StepWin w{};
  const char *wbase = nullptr;
  const int rc = step_window(*cfg, *b, &wbase, &w);
  if (rc) return rc;
  const StepK k = step_constants(*cfg);
  const int grid = (b->n + kBlock - 1) / kBlock;
  hipStream_t s = (hipStream_t)stream;
  const bool dist = b->dist != nullptr;
  if (step_has_dist(*cfg) && !dist) return 4;   // a disturbance / water current is on: dist is required
  // the production shape (statistics on, in-kernel draws, no disturbance) on the canonical slab: constant offsets
  const int sh = fixed_slab_shift(*cfg, *b);
  if (sh >= 0 && cfg->stats_on && !u_inject && !dist) {
    const char *base = reinterpret_cast<const char *>(b->px);
#define USV_FIXED_CASE(S)                                                                                            \
  case S:                                                                                                            \
    hipLaunchKernelGGL((k_env_step<true, false, false, FixedWin<S>>), dim3(grid), dim3(kBlock), 0, s,                \
                       StepCfg{*cfg, k}, *b, FixedWin<S>{}, base, actions, lut_dev, action_bias, seed, step, u_inject,  \
                       part);                                                                                        \
    break;
    switch (sh) {
      USV_FIXED_CASE(13) USV_FIXED_CASE(14) USV_FIXED_CASE(15) USV_FIXED_CASE(16) USV_FIXED_CASE(17)
      USV_FIXED_CASE(18) USV_FIXED_CASE(19) USV_FIXED_CASE(20) USV_FIXED_CASE(21) USV_FIXED_CASE(22)
      default: return 6;
    }
#undef USV_FIXED_CASE
    USV_CHECK_LAUNCH();
    return 0;
  }
  auto kern = dist ? (cfg->stats_on ? (u_inject ? k_env_step<true, true, true, StepWin> : k_env_step<true, false, true, StepWin>)
                                    : (u_inject ? k_env_step<false, true, true, StepWin> : k_env_step<false, false, true, StepWin>))
                   : (cfg->stats_on ? (u_inject ? k_env_step<true, true, false, StepWin> : k_env_step<true, false, false, StepWin>)
                                    : (u_inject ? k_env_step<false, true, false, StepWin> : k_env_step<false, false, false, StepWin>));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, s, StepCfg{*cfg, k}, *b, w, wbase, actions, lut_dev, action_bias,
                     seed, step, u_inject, part);
  USV_CHECK_LAUNCH();
  return 0;
}

int usv_env_step_late(const usv_cfg_t *cfg, const usv_bufs_t *b, void *stream) {
  if (!cfg || !b || b->n <= 0 || !b->rstash || !b->field || !b->sdf || !b->fnorm ||
      cfg->task_kind != USV_TASK_CAPTURE_XY)
    return 1;
  // one-wave workgroups striding over the device reset count (~1% of the envs per step at the headline size)
  const int grid = (b->n + 63) / 64 < kLateGrid ? (b->n + 63) / 64 : kLateGrid;
  hipLaunchKernelGGL(k_env_reward_late, dim3(grid), dim3(64), 0, (hipStream_t)stream, *cfg, *b);
  USV_CHECK_LAUNCH();
  return 0;
}

int usv_env_step(const usv_cfg_t *cfg, const usv_bufs_t *b, const float *actions, const float *lut_dev,
                 float action_bias, uint64_t seed, uint64_t step, const float *u_inject, void *stream) {
  return usv_env_step_part(cfg, b, actions, lut_dev, action_bias, seed, step, u_inject, 0, stream);
}

int usv_forces(const usv_cfg_t *cfg, const usv_bufs_t *b, float *out, void *stream) {
  if (!cfg || !b || !out || b->n <= 0) return 1;
  hipLaunchKernelGGL(k_forces, dim3((b->n + 255) / 256), dim3(256), 0, (hipStream_t)stream, *cfg, *b, out);
  USV_CHECK_LAUNCH();
  return 0;
}

int usv_hydrostatics(const usv_hydro_t *h, int n, const float *quat, const float *root_z, float *volume,
                     float *euler, float *wrench, void *stream) {
  if (!h || !quat || !root_z || !volume || !euler || !wrench || n <= 0) return 1;
  hipLaunchKernelGGL(k_hydrostatics, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, *h, n, quat, root_z,
                     volume, euler, wrench);
  USV_CHECK_LAUNCH();
  return 0;
}

int usv_hip_version(void) { return 1; }

// Every integer #define, enumerator and ABI struct size / field offset of include/usv_hip.h (the generated
// list csrc/usv_layout_gen.h, in header order), folded with its name: see _abi.layout_key_of.
static unsigned long long fnv1a(const char *s) {
  unsigned long long h = 1469598103934665603ull;
  for (; *s; ++s) h = (h ^ (unsigned char)*s) * 1099511628211ull;
  return h;
}
long long usv_hip_layout_key(void) {
  unsigned long long k = 0;
#define USV_LAYOUT_FOLD(expr, name)                                    \
  k = k * 1000003ull + fnv1a(name);                                    \
  k = k * 1000003ull + (unsigned long long)(long long)(expr);
  USV_LAYOUT_ENTRIES(USV_LAYOUT_FOLD)
#undef USV_LAYOUT_FOLD
  return (long long)(k & 0x7fffffffffffffffull);
}

}  // extern "C"
