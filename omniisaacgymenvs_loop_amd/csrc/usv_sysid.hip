// SysID student distillation (include/usv_hip.h "sysid"): the StateHistoryEncoder(tsteps=50) forward /
// backward on windows that are views of a ring of frames, the frozen teacher's mass_encoder (z*) and
// action_mlp, Adam, and the update's diagnostics.  Float32 throughout (metrics in double).
//
// k_sy_net<GRAD>: one workgroup of 256 threads per tile of RT = 8 storage rows, thread (r, o) = (row of the
// tile, output channel).  The conv weights sit in LDS as [(k * 32 + c) * 33 + o]: lanes over o (forward) and
// lanes over c (backward-data) both hit distinct banks.  Activations per row: P [50][32] (the projection, read
// by conv 1 as [32][50]: the reference's raw reshape), A1 [32][11], A2 [32][7], A3 [32][3]; the frames of the
// window are staged in P's space first.  The backward pass overwrites each activation with the gradient of
// its pre-activation once the weight gradient that needs the activation has been taken, so nothing else is
// stored.  Weight gradients accumulate in registers over every tile of the workgroup (thread (o, cg) owns
// channels c = 4 cg .. 4 cg + 3 of output channel o) and are written once, as one partial row; k_sy_apply sums
// the rows in index order (bit-reproducible) and applies Adam.
//
// k_sy_play (sysid_play, the deployment step): the same forward on the matrix cores, described where it is defined.
#include "usv_device.h"

#include <cmath>

namespace {

constexpr int T = SY_T, C = SY_CH, L = SY_LAT, PRIV = SY_PRIV;
constexpr int K1 = SY_K1, S1 = SY_S1, L1 = SY_L1, K2 = SY_K2, L2 = SY_L2, L3 = SY_L3;
constexpr int FLAT = C * L3;                  // 96
constexpr int MAXD = LZ_MAX_OBS - PRIV;       // 28
constexpr int RT = 8, TB = 256;
constexpr int WPAD = C + 1;
constexpr float SLOPE = 0.01f;
constexpr int MAX_GROUPS = 256;        // gradient workgroups = partial rows (one per CU)
constexpr int MAX_FWD_GROUPS = 2048;   // forward workgroups; further tiles loop

struct Off {
  int w0, b0, w1, b1, w2, b2, w3, b3, wl, bl, n;
};
__host__ __device__ inline Off offsets(int D) {
  Off o;
  o.w0 = 0;
  o.b0 = o.w0 + C * D;
  o.w1 = o.b0 + C;
  o.b1 = o.w1 + C * C * K1;
  o.w2 = o.b1 + C;
  o.b2 = o.w2 + C * C * K2;
  o.w3 = o.b2 + C;
  o.b3 = o.w3 + C * C * K2;
  o.wl = o.b3 + C;
  o.bl = o.wl + L * FLAT;
  o.n = o.bl + L;
  return o;
}
// teacher (loopz actor architecture) offsets: mass_encoder 8-64-16-8, action_mlp (D + 8)-128-128-2
struct TOff {
  int e0w, e0b, e1w, e1b, e2w, e2b, a0w, a0b, a1w, a1b, a2w, a2b;
};
__host__ __device__ inline TOff toffsets(int D) {
  TOff o;
  o.e0w = 0;
  o.e0b = o.e0w + LZ_E1 * LZ_MASS;
  o.e1w = o.e0b + LZ_E1;
  o.e1b = o.e1w + LZ_E2 * LZ_E1;
  o.e2w = o.e1b + LZ_E2;
  o.e2b = o.e2w + LZ_LAT * LZ_E2;
  o.a0w = o.e2b + LZ_LAT;
  o.a0b = o.a0w + LZ_NH * (D + L);
  o.a1w = o.a0b + LZ_NH;
  o.a1b = o.a1w + LZ_NH * LZ_NH;
  o.a2w = o.a1b + LZ_NH;
  o.a2b = o.a2w + LZ_NA * LZ_NH;
  return o;
}

__device__ __forceinline__ float leaky(float x) { return x > 0.f ? x : SLOPE * x; }
// derivative from the activation's output (same sign as its input; 0 takes the slope, as torch does)
__device__ __forceinline__ float dleaky(float a) { return a > 0.f ? 1.f : SLOPE; }

struct Geo {
  int n, D, H, R, base;
};
__device__ __forceinline__ int ring_slot(const Geo &g, int s, int k) {
  int i = g.base + s + k;   // base < R, s + k < R
  return i >= g.R ? i - g.R : i;
}

// LDS layout (floats)
constexpr int LW1 = 0;
constexpr int LW2 = LW1 + K1 * C * WPAD;
constexpr int LW3 = LW2 + K2 * C * WPAD;
constexpr int LWL = LW3 + K2 * C * WPAD;
constexpr int LB = LWL + L * FLAT;             // b1 b2 b3 [32 each], bl [8]
constexpr int LP = LB + 3 * C + L;
constexpr int PROW = T * C;                    // 1600 >= T * MAXD
constexpr int LA1 = LP + RT * PROW;
constexpr int LA2 = LA1 + RT * C * L1;
constexpr int LA3 = LA2 + RT * C * L2;
constexpr int LDZ = LA3 + RT * C * L3;
constexpr int LRED = LDZ + RT * L;
constexpr int LDS_FLOATS = LRED + TB / 64 + 4;
constexpr int FR = 3;                          // rows of frames staged at a time for the projection's gradient
static_assert(FR * T * MAXD <= LDZ - LA1, "staged frames fit the space of A1..A3");
constexpr int LDS_INTS = 3 * RT;               // env, s, valid of the tile's rows
constexpr size_t LDS_BYTES = (size_t)(LDS_FLOATS + LDS_INTS) * 4;
static_assert(LDS_BYTES <= 160 * 1024, "k_sy_net LDS");
static_assert(LP % 4 == 0 && PROW % 4 == 0 && T % 2 == 0, "rows of P are read as float2");
static_assert(T * MAXD <= PROW, "frames are staged in the projection's space");

// LIN consecutive floats of LDS into registers; an even LIN starts 8-byte aligned (rows of 50 floats from a
// 16-byte aligned base) and is read two floats at a time: the convs are bound by LDS instructions, not bytes
template <int LIN>
__device__ __forceinline__ void load_row(const float *X, float (&x)[LIN]) {
  if constexpr (LIN % 2 == 0) {
    const float2 *X2 = reinterpret_cast<const float2 *>(X);
#pragma unroll
    for (int m = 0; m < LIN / 2; ++m) {
      const float2 v = X2[m];
      x[2 * m] = v.x;
      x[2 * m + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int m = 0; m < LIN; ++m) x[m] = X[m];
  }
}

// forward of one conv layer for thread (r, o): X [C][LIN] of row r -> leaky(conv) into Y [C][LOUT]
template <int K, int S, int LIN, int LOUT>
__device__ __forceinline__ void conv_fwd(const float *__restrict__ W, float bias, const float *X, float *Y, int o) {
  float acc[LOUT];
#pragma unroll
  for (int j = 0; j < LOUT; ++j) acc[j] = bias;
#pragma unroll 1
  for (int c = 0; c < C; ++c) {
    float x[LIN];
    load_row<LIN>(X + c * LIN, x);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float w = W[(k * C + c) * WPAD + o];
#pragma unroll
      for (int j = 0; j < LOUT; ++j) acc[j] = fmaf(w, x[S * j + k], acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < LOUT; ++j) Y[o * LOUT + j] = leaky(acc[j]);
}

// weight gradient of one conv layer for thread (o, cg): acc[4][K] += sum_rows sum_j dY[o][j] X[c][S j + k]
template <int K, int S, int LIN, int LOUT>
__device__ __forceinline__ void conv_bwd_w(const float *Xt, int xstride, const float *dYt, int ystride, int o, int cg,
                                           float (&acc)[4][K], float &accb) {
#pragma unroll 1
  for (int r = 0; r < RT; ++r) {
    float dy[LOUT];
#pragma unroll
    for (int j = 0; j < LOUT; ++j) dy[j] = dYt[r * ystride + o * LOUT + j];
    if (cg == 0) {
#pragma unroll
      for (int j = 0; j < LOUT; ++j) accb += dy[j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float x[LIN];
      load_row<LIN>(Xt + r * xstride + (cg * 4 + i) * LIN, x);
#pragma unroll
      for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int j = 0; j < LOUT; ++j) acc[i][k] = fmaf(dy[j], x[S * j + k], acc[i][k]);
      }
    }
  }
}

// data gradient of one conv layer for thread (r, c): dx[m] = sum_o sum_k W[o][c][k] dY[o][j], m = S j + k
template <int K, int S, int LIN, int LOUT>
__device__ __forceinline__ void conv_bwd_x(const float *__restrict__ W, const float *dY, int c, float (&dx)[LIN]) {
#pragma unroll
  for (int m = 0; m < LIN; ++m) dx[m] = 0.f;
#pragma unroll 1
  for (int o = 0; o < C; ++o) {
    float dy[LOUT];
#pragma unroll
    for (int j = 0; j < LOUT; ++j) dy[j] = dY[o * LOUT + j];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float w = W[(k * C + c) * WPAD + o];
#pragma unroll
      for (int j = 0; j < LOUT; ++j) dx[S * j + k] = fmaf(w, dy[j], dx[S * j + k]);
    }
  }
}

template <bool GRAD>
__global__ __launch_bounds__(TB) void k_sy_net(const float *__restrict__ enc, Geo g, int row0, int rows,
                                               const float *__restrict__ stream, const int32_t *__restrict__ valid_rows,
                                               const float *__restrict__ zstar, float *__restrict__ zhat,
                                               float *__restrict__ partials, int pstride) {
  extern __shared__ float lds[];
  int *rinfo = (int *)(lds + LDS_FLOATS);
  const int tid = threadIdx.x, o = tid & 31, r = tid >> 5, cg = r;
  const int D = g.D;
  const Off off = offsets(D);

  // weights -> LDS (conv weights as [(k * 32 + c) * 33 + o])
#pragma unroll 8
  for (int i = tid; i < C * C * K1; i += TB) {
    const int oo = i / (C * K1), c = (i / K1) % C, k = i % K1;
    lds[LW1 + (k * C + c) * WPAD + oo] = enc[off.w1 + i];
  }
#pragma unroll 4
  for (int i = tid; i < C * C * K2; i += TB) {
    const int oo = i / (C * K2), c = (i / K2) % C, k = i % K2;
    lds[LW2 + (k * C + c) * WPAD + oo] = enc[off.w2 + i];
    lds[LW3 + (k * C + c) * WPAD + oo] = enc[off.w3 + i];
  }
  for (int i = tid; i < L * FLAT; i += TB) lds[LWL + i] = enc[off.wl + i];
  if (tid < C) {
    lds[LB + tid] = enc[off.b1 + tid];
    lds[LB + C + tid] = enc[off.b2 + tid];
    lds[LB + 2 * C + tid] = enc[off.b3 + tid];
  }
  if (tid < L) lds[LB + 3 * C + tid] = enc[off.bl + tid];
  float w0[MAXD];
#pragma unroll
  for (int d = 0; d < MAXD; ++d) w0[d] = d < D ? enc[off.w0 + o * D + d] : 0.f;
  const float b0 = enc[off.b0 + o];

  // gradient accumulators (GRAD only; dead code otherwise)
  float gW1[4][K1], gW2[4][K2], gW3[4][K2], gW0[4], gWl[3], gb0 = 0.f, gb1 = 0.f, gb2 = 0.f, gb3 = 0.f, gbl = 0.f;
  float loss = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    gW0[i] = 0.f;
#pragma unroll
    for (int k = 0; k < K1; ++k) gW1[i][k] = 0.f;
#pragma unroll
    for (int k = 0; k < K2; ++k) gW2[i][k] = gW3[i][k] = 0.f;
  }
  gWl[0] = gWl[1] = gWl[2] = 0.f;
  const float gscale = 2.0f / ((float)rows * (float)L);

  float *P = lds + LP + r * PROW, *A1 = lds + LA1 + r * C * L1, *A2 = lds + LA2 + r * C * L2,
        *A3 = lds + LA3 + r * C * L3;
  const int ntiles = (rows + RT - 1) / RT;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();   // the previous tile's reads are done
    if (tid < RT) {
      const int lr = min(tile * RT + tid, rows - 1);   // rows past the end repeat the last one (never written)
      const int row = row0 + lr;
      rinfo[tid] = row % g.n;
      rinfo[RT + tid] = row / g.n;
      rinfo[2 * RT + tid] = valid_rows[row];
    }
    __syncthreads();
    // frames of the RT windows -> P's space, [T][D] per row
    if (o < D) {   // thread (r, d = o): frame k of row r, T independent loads
      const int env = rinfo[r], s = rinfo[RT + r], k0 = T - rinfo[2 * RT + r];
#pragma unroll 10
      for (int k = 0; k < T; ++k)
        P[k * D + o] = stream[((size_t)ring_slot(g, s, max(k, k0)) * g.n + env) * D + o];
    }
    __syncthreads();
    {  // projection: p[t] = leaky(W0[o] . frame_t + b0[o]), then P[t * 32 + o]
      float p[T];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        float acc = b0;
#pragma unroll
        for (int d = 0; d < MAXD; ++d)
          if (d < D) acc = fmaf(w0[d], P[t * D + d], acc);
        p[t] = leaky(acc);
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < T; ++t) P[t * C + o] = p[t];
    }
    __syncthreads();
    conv_fwd<K1, S1, T, L1>(lds + LW1, lds[LB + o], P, A1, o);
    __syncthreads();
    conv_fwd<K2, 1, L1, L2>(lds + LW2, lds[LB + C + o], A1, A2, o);
    __syncthreads();
    conv_fwd<K2, 1, L2, L3>(lds + LW3, lds[LB + 2 * C + o], A2, A3, o);
    __syncthreads();
    const int lrow = tile * RT + r;
    if (o < L) {
      float acc = lds[LB + 3 * C + o];
      for (int i = 0; i < FLAT; ++i) acc += lds[LWL + o * FLAT + i] * A3[i];
      const float z = leaky(acc);
      if (lrow < rows) {
        if (zhat) zhat[(size_t)lrow * L + o] = z;
        if (GRAD) {
          const float e = z - zstar[(size_t)(row0 + lrow) * L + o];
          loss += e * e;
          lds[LDZ + r * L + o] = gscale * e * dleaky(z);
        }
      } else if (GRAD) {
        lds[LDZ + r * L + o] = 0.f;
      }
    }
    if (!GRAD) continue;
    __syncthreads();
    {  // linear_output: weight gradient (3 elements per thread), then dY3 over A3
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int e = tid + TB * q, l = e / FLAT, i = e - l * FLAT;
#pragma unroll 1
        for (int rr = 0; rr < RT; ++rr) gWl[q] = fmaf(lds[LDZ + rr * L + l], lds[LA3 + rr * C * L3 + i], gWl[q]);
      }
      if (tid < L)
        for (int rr = 0; rr < RT; ++rr) gbl += lds[LDZ + rr * L + tid];
      float gf[L3];
#pragma unroll
      for (int j = 0; j < L3; ++j) {
        float a = 0.f;
#pragma unroll
        for (int l = 0; l < L; ++l) a += lds[LWL + l * FLAT + o * L3 + j] * lds[LDZ + r * L + l];
        gf[j] = a;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < L3; ++j) A3[o * L3 + j] = gf[j] * dleaky(A3[o * L3 + j]);
    }
    __syncthreads();
    {  // conv 3
      conv_bwd_w<K2, 1, L2, L3>(lds + LA2, C * L2, lds + LA3, C * L3, o, cg, gW3, gb3);
      float dx[L2];
      conv_bwd_x<K2, 1, L2, L3>(lds + LW3, A3, o, dx);
      __syncthreads();
#pragma unroll
      for (int m = 0; m < L2; ++m) A2[o * L2 + m] = dx[m] * dleaky(A2[o * L2 + m]);
    }
    __syncthreads();
    {  // conv 2
      conv_bwd_w<K2, 1, L1, L2>(lds + LA1, C * L1, lds + LA2, C * L2, o, cg, gW2, gb2);
      float dx[L1];
      conv_bwd_x<K2, 1, L1, L2>(lds + LW2, A2, o, dx);
      __syncthreads();
#pragma unroll
      for (int m = 0; m < L1; ++m) A1[o * L1 + m] = dx[m] * dleaky(A1[o * L1 + m]);
    }
    __syncthreads();
    {  // conv 1 (its input is P read as [32][50])
      conv_bwd_w<K1, S1, T, L1>(lds + LP, PROW, lds + LA1, C * L1, o, cg, gW1, gb1);
      float dx[T];
      conv_bwd_x<K1, S1, T, L1>(lds + LW1, A1, o, dx);
      __syncthreads();
#pragma unroll
      for (int m = 0; m < T; ++m) P[o * T + m] = dx[m] * dleaky(P[o * T + m]);
    }
    __syncthreads();
    // projection: dW0[o][d] += sum_t dP[t][o] frame_t[d], d = cg + 8 i.  The frames come from the stream again,
    // FR rows at a time through the space of A1..A3 (free now), thread (r, d = o) loading as above.
    for (int rb = 0; rb < RT; rb += FR) {
      const int nr = min(FR, RT - rb);
      float *F = lds + LA1;
      if (o < D) {
        for (int rl = 0; rl < nr; ++rl) {
          const int env = rinfo[rb + rl], s = rinfo[RT + rb + rl], k0 = T - rinfo[2 * RT + rb + rl];
#pragma unroll 7
          for (int k = r; k < T; k += RT)
            F[(rl * T + k) * D + o] = stream[((size_t)ring_slot(g, s, max(k, k0)) * g.n + env) * D + o];
        }
      }
      __syncthreads();
      for (int rl = 0; rl < nr; ++rl) {
        const float *dP = lds + LP + (rb + rl) * PROW, *f = F + rl * T * D;
#pragma unroll 2
        for (int t = 0; t < T; ++t) {
          const float dp = dP[t * C + o];
          if (cg == 0) gb0 += dp;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int d = cg + 8 * i;
            if (d < D) gW0[i] = fmaf(dp, f[t * D + d], gW0[i]);
          }
        }
      }
      __syncthreads();
    }
  }
  if (!GRAD) return;
  // one partial row per workgroup
  float *out = partials + (size_t)blockIdx.x * pstride;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = cg * 4 + i, d = cg + 8 * i;
    if (d < D) out[off.w0 + o * D + d] = gW0[i];
#pragma unroll
    for (int k = 0; k < K1; ++k) out[off.w1 + (o * C + c) * K1 + k] = gW1[i][k];
#pragma unroll
    for (int k = 0; k < K2; ++k) {
      out[off.w2 + (o * C + c) * K2 + k] = gW2[i][k];
      out[off.w3 + (o * C + c) * K2 + k] = gW3[i][k];
    }
  }
  if (cg == 0) {
    out[off.b0 + o] = gb0;
    out[off.b1 + o] = gb1;
    out[off.b2 + o] = gb2;
    out[off.b3 + o] = gb3;
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) out[off.wl + tid + TB * q] = gWl[q];
  if (tid < L) out[off.bl + tid] = gbl;
  // squared-error sum of the workgroup's rows, in a fixed order
  __syncthreads();
  const float ws = wave_sum(loss);
  if ((tid & 63) == 0) lds[LRED + (tid >> 6)] = ws;
  __syncthreads();
  if (tid == 0) out[off.n] = ((lds[LRED] + lds[LRED + 1]) + lds[LRED + 2]) + lds[LRED + 3];
}

// grad[p] = sum of the G partial rows in index order, then torch.optim.Adam (as k_lz_apply); thread np of the
// grid writes the minibatch loss
__global__ __launch_bounds__(256) void k_sy_apply(float *P, float *m, float *v, const float *__restrict__ partials,
                                                  int G, int pstride, int np, int rows, float lr, int adam_step,
                                                  int apply, float *grad, float *loss_out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p > np) return;
  float acc = 0.f;
  for (int b0 = 0; b0 < G; b0 += 8) {
    float x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = partials[(size_t)min(b0 + k, G - 1) * pstride + p];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (b0 + k < G) acc += x[k];
  }
  if (p == np) {
    if (loss_out) *loss_out = acc / ((float)rows * (float)L);
    return;
  }
  grad[p] = acc;
  if (!apply) return;
  // torch.optim.Adam's defaults as torch applies them to float32 tensors: the betas are Python doubles, rounded to
  // float where they scale a tensor (1 - beta taken in double first) and kept double in the bias corrections
  const double B1 = 0.9, B2 = 0.999;
  const float b2 = (float)B2, omb1 = (float)(1.0 - B1), omb2 = (float)(1.0 - B2), eps = 1e-8f;
  const double bc1 = 1.0 - pow(B1, (double)adam_step);
  const double bc2 = 1.0 - pow(B2, (double)adam_step);
  const float step_size = (float)((double)lr / bc1);
  const float bc2s = (float)sqrt(bc2);
  const float mi = m[p] + omb1 * (acc - m[p]);
  const float vi = v[p] * b2 + omb2 * acc * acc;
  const float denom = sqrtf(vi) / bc2s + eps;
  P[p] = P[p] - step_size * (mi / denom);
  m[p] = mi;
  v[p] = vi;
}

// one thread per env: frame -> ring, valid, z* = teacher mass_encoder(priv tail) (LeakyReLU after each layer)
__global__ __launch_bounds__(256) void k_sy_append(const float *__restrict__ obs, const int64_t *__restrict__ dones,
                                                   const float *__restrict__ teacher, Geo g, int obs_dim, int s,
                                                   int fill_mode, int fresh, float *__restrict__ stream,
                                                   int32_t *__restrict__ valid_rows, int32_t *__restrict__ valid_cur,
                                                   float *__restrict__ zstar) {
  const int env = blockIdx.x * 256 + threadIdx.x;
  if (env >= g.n) return;
  const float *x = obs + (size_t)env * obs_dim;
  float *f = stream + ((size_t)ring_slot(g, s, T - 1) * g.n + env) * g.D;
  for (int d = 0; d < g.D; ++d) f[d] = x[d];
  int v = T;
  if (fill_mode == SY_FILL_REPEAT) v = (fresh || (dones && dones[env] != 0)) ? 1 : min(valid_cur[env] + 1, T);
  valid_cur[env] = v;
  valid_rows[(size_t)s * g.n + env] = v;
  if (!teacher) return;
  const TOff to = toffsets(g.D);
  float in[LZ_MASS], h1[LZ_E1], h2[LZ_E2];
#pragma unroll
  for (int i = 0; i < LZ_MASS; ++i) in[i] = x[g.D + i];
#pragma unroll
  for (int j = 0; j < LZ_E1; ++j) {
    float a = teacher[to.e0b + j];
#pragma unroll
    for (int i = 0; i < LZ_MASS; ++i) a += teacher[to.e0w + j * LZ_MASS + i] * in[i];
    h1[j] = leaky(a);
  }
#pragma unroll
  for (int j = 0; j < LZ_E2; ++j) {
    float a = teacher[to.e1b + j];
#pragma unroll
    for (int i = 0; i < LZ_E1; ++i) a += teacher[to.e1w + j * LZ_E1 + i] * h1[i];
    h2[j] = leaky(a);
  }
  float *z = zstar + ((size_t)s * g.n + env) * L;
#pragma unroll
  for (int j = 0; j < L; ++j) {
    float a = teacher[to.e2b + j];
#pragma unroll
    for (int i = 0; i < LZ_E2; ++i) a += teacher[to.e2w + j * LZ_E2 + i] * h2[i];
    z[j] = leaky(a);
  }
}

// frozen action head on [cur | zhat]: RA rows per workgroup of 128 threads, thread j = hidden unit
constexpr int RA = 16, ATB = LZ_NH, AIN = MAXD + L;
__global__ __launch_bounds__(ATB) void k_sy_action(const float *__restrict__ teacher, Geo g, int s,
                                                   const float *__restrict__ stream, const float *__restrict__ zhat,
                                                   float *__restrict__ actions) {
  __shared__ float x[RA][AIN], h1[RA][LZ_NH], h2[RA][LZ_NH];
  const int j = threadIdx.x, in = g.D + L;
  const TOff to = toffsets(g.D);
  const int e0 = blockIdx.x * RA;
  const size_t cur = (size_t)ring_slot(g, s, T - 1) * g.n;
  for (int i = j; i < RA * in; i += ATB) {
    const int rr = i / in, d = i - rr * in, env = min(e0 + rr, g.n - 1);
    x[rr][d] = d < g.D ? stream[(cur + env) * g.D + d] : zhat[(size_t)env * L + (d - g.D)];
  }
  __syncthreads();
  float acc[RA];
  {
    const float b = teacher[to.a0b + j];
#pragma unroll
    for (int rr = 0; rr < RA; ++rr) acc[rr] = b;
    for (int i = 0; i < in; ++i) {
      const float w = teacher[to.a0w + j * in + i];
#pragma unroll
      for (int rr = 0; rr < RA; ++rr) acc[rr] += w * x[rr][i];
    }
#pragma unroll
    for (int rr = 0; rr < RA; ++rr) h1[rr][j] = leaky(acc[rr]);
  }
  __syncthreads();
  {
    const float b = teacher[to.a1b + j];
#pragma unroll
    for (int rr = 0; rr < RA; ++rr) acc[rr] = b;
    for (int i = 0; i < LZ_NH; ++i) {
      const float w = teacher[to.a1w + j * LZ_NH + i];
#pragma unroll
      for (int rr = 0; rr < RA; ++rr) acc[rr] += w * h1[rr][i];
    }
#pragma unroll
    for (int rr = 0; rr < RA; ++rr) h2[rr][j] = leaky(acc[rr]);
  }
  __syncthreads();
  if (j < RA * LZ_NA) {
    const int rr = j / LZ_NA, a = j - rr * LZ_NA, env = e0 + rr;
    float y = teacher[to.a2b + a];
    for (int i = 0; i < LZ_NH; ++i) y += teacher[to.a2w + a * LZ_NH + i] * h2[rr][i];
    if (env < g.n) actions[(size_t)env * LZ_NA + a] = tanhf(y);
  }
}

// ---- k_sy_play: the encoder forward on the matrix cores (sysid_play) ---------------------------------------------
// One workgroup of 4 waves per tile of RT = 8 windows; every product is a GEMM with N = 32 output channels on
// v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate): the A operand is the activation (row m = (window, output
// position), im2col addressing straight from the layer input in LDS), the B operand the weights, kept in LDS as
// [kidx][32] so that k-step s of lane l reads float 64 s + l (no bank conflict).  kidx = c * K + k (projection: d),
// and the accumulator starts at the bias: an f32 MFMA is a k-ordered fmaf chain, so every output is the chain
// k_sy_net's conv_fwd computes.  A wave owns whole 32-row tiles (projection 13 tiles, conv 1 / 2 / 3: 3 / 2 / 1);
// rows past the last one repeat it and are not written.  LDS: weights 79 KB, the projection of 8 windows 50 KB
// (rows padded to 1601 floats: the windows of a tile fall on different banks), A1..A3 21 KB.
namespace play {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NW = TB / 64;                  // waves
constexpr int DP = MAXD;                     // k extent of the projection (rows d >= D of W0 are zero)
constexpr int FS = DP + 1;                   // floats per staged frame (odd: conflict-free A reads)
constexpr int PROWM = T * C + 1;
constexpr int MW0 = 0;                       // [DP][32]
constexpr int MW1 = MW0 + DP * C;            // [C K1][32]
constexpr int MW2 = MW1 + C * K1 * C;        // [C K2][32]
constexpr int MW3 = MW2 + C * K2 * C;
constexpr int MWL = MW3 + C * K2 * C;        // [L][FLAT]
constexpr int MB = MWL + L * FLAT;           // b0 b1 b2 b3 [32 each], bl [8]
constexpr int MP = MB + 4 * C + L;
constexpr int MA1 = MP + RT * PROWM;
constexpr int MA2 = MA1 + RT * C * L1;
constexpr int MA3 = MA2 + RT * C * L2;
constexpr int M_FLOATS = MA3 + RT * C * L3;
constexpr size_t M_BYTES = (size_t)M_FLOATS * 4;
constexpr int PTILES = (RT * T + 31) / 32;   // 13
constexpr int PQ = (PTILES + NW - 1) / NW;   // projection tiles per wave
constexpr int MAX_PLAY_GROUPS = 256;       // one per CU (the LDS admits one): the weights are staged once
static_assert(M_BYTES <= 160 * 1024, "k_sy_play LDS");
static_assert(RT * T * FS <= RT * PROWM, "frames are staged in the projection's space");
static_assert(DP % 2 == 0 && (C * K1) % 2 == 0 && (C * K2) % 2 == 0, "two k per MFMA");
static_assert((RT * L1 + 31) / 32 <= NW && (RT * L2 + 31) / 32 <= NW && (RT * L3 + 31) / 32 <= NW, "one tile per wave");

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// one 32-row tile of a conv layer: rows m = (window w, position j) of the RT windows, X [RT][xstride] the layer
// input ([C][LIN] per window), Y [RT][C LOUT] its output ([C][LOUT] per window), WB [C K][32]
template <int K, int S, int LIN, int LOUT>
__device__ __forceinline__ void conv_tile(const float *WB, float bias, const float *X, int xstride, float *Y, int tile,
                                          int lane) {
  constexpr int M = RT * LOUT;
  const int i = lane & 31, h = lane >> 5;
  const int m = min(tile * 32 + i, M - 1);
  const int w = m / LOUT, j = m - w * LOUT;
  const float *xa = X + w * xstride + S * j;
  const float *wb = WB + lane;
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = bias;
  // kidx = 2 s + h = c K + k reads X at c LIN + k.  G k-steps cover a whole number CG of channels, so the offsets
  // of a group are per-lane constants and its 2 G operand reads do not depend on one another; the next group's
  // operands are read before this group's products
  constexpr int G = K % 2 == 0 ? K / 2 : K, CG = 2 * G / K, NG = C / CG;
  static_assert(C % CG == 0, "whole groups");
  int offq[G];
#pragma unroll
  for (int q = 0; q < G; ++q) offq[q] = ((2 * q + h) / K) * LIN + (2 * q + h) % K;
  float a[G], b[G], an[G], bn[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {
    a[q] = xa[offq[q]];
    b[q] = wb[64 * q];
  }
#pragma unroll 1
  for (int gi = 0; gi < NG; ++gi) {
    const int gn = min(gi + 1, NG - 1);   // the last group re-reads itself
#pragma unroll
    for (int q = 0; q < G; ++q) {
      an[q] = xa[gn * (CG * LIN) + offq[q]];
      bn[q] = wb[64 * (gn * G + q)];
    }
#pragma unroll
    for (int q = 0; q < G; ++q) acc = mfma(a[q], b[q], acc);
#pragma unroll
    for (int q = 0; q < G; ++q) {
      a[q] = an[q];
      b[q] = bn[q];
    }
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int mo = tile * 32 + acc_row(q, lane);
    if (mo < M) {
      const int wo = mo / LOUT, jo = mo - wo * LOUT;
      Y[wo * (C * LOUT) + i * LOUT + jo] = leaky(acc[q]);
    }
  }
}

__global__ __launch_bounds__(TB) void k_sy_play(const float *__restrict__ enc, Geo g, int row0, int rows,
                                                const float *__restrict__ stream,
                                                const int32_t *__restrict__ valid_rows, float *__restrict__ zhat) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, o = tid & 31, r = tid >> 5;
  const int D = g.D;
  const Off off = offsets(D);

  // weights -> LDS as [kidx][32]
  for (int i = tid; i < DP * C; i += TB) {
    const int d = i >> 5, oo = i & 31;
    lds[MW0 + i] = d < D ? enc[off.w0 + oo * D + d] : 0.f;
  }
#pragma unroll 8
  for (int i = tid; i < C * K1 * C; i += TB) lds[MW1 + i] = enc[off.w1 + (i & 31) * (C * K1) + (i >> 5)];
#pragma unroll 4
  for (int i = tid; i < C * K2 * C; i += TB) {
    lds[MW2 + i] = enc[off.w2 + (i & 31) * (C * K2) + (i >> 5)];
    lds[MW3 + i] = enc[off.w3 + (i & 31) * (C * K2) + (i >> 5)];
  }
  for (int i = tid; i < L * FLAT; i += TB) lds[MWL + i] = enc[off.wl + i];
  if (tid < C) {
    lds[MB + tid] = enc[off.b0 + tid];
    lds[MB + C + tid] = enc[off.b1 + tid];
    lds[MB + 2 * C + tid] = enc[off.b2 + tid];
    lds[MB + 3 * C + tid] = enc[off.b3 + tid];
  }
  if (tid < L) lds[MB + 4 * C + tid] = enc[off.bl + tid];

  float *F = lds + MP;   // staged frames [RT T][FS], then the projection [RT][PROWM]
  const int ntiles = (rows + RT - 1) / RT;
  // thread (r, d = o) owns column d of the T frames of window r.  The frames of the next tile are loaded into
  // registers before this tile's products and stored to LDS after them: T loads in flight per thread, their
  // latency under the matrix-core phases
  float fr[T];
  auto load_frames = [&](int tile) {
    const int lr = min(tile * RT + r, rows - 1);   // rows past the end repeat the last one (never written)
    const int row = row0 + lr, env = row % g.n, s = row / g.n, k0 = T - valid_rows[row];
    if (o < D) {
#pragma unroll
      for (int k = 0; k < T; ++k) fr[k] = stream[((size_t)ring_slot(g, s, max(k, k0)) * g.n + env) * D + o];
    }
  };
#pragma unroll
  for (int k = 0; k < T; ++k) fr[k] = 0.f;   // columns D <= d < DP stay zero
  if (blockIdx.x < ntiles) load_frames(blockIdx.x);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();   // the previous tile's reads are done (first pass: the weights are in place)
    if (o < DP) {
      float *f = F + r * T * FS + o;
#pragma unroll
      for (int k = 0; k < T; ++k) f[k * FS] = fr[k];
    }
    if (tile + (int)gridDim.x < ntiles) load_frames(tile + gridDim.x);
    __syncthreads();
    {  // projection: rows m = w T + t, K = DP
      f32x16 pacc[PQ];
      const float b0 = lds[MB + o];
#pragma unroll
      for (int q = 0; q < PQ; ++q) {
        const int tI = wave + NW * q;
#pragma unroll
        for (int x = 0; x < 16; ++x) pacc[q][x] = b0;
        if (tI < PTILES) {
          const int m = min(tI * 32 + o, RT * T - 1);
          const float *fa = F + m * FS + (lane >> 5), *wb = lds + MW0 + lane;
#pragma unroll
          for (int s = 0; s < DP / 2; ++s) pacc[q] = mfma(fa[2 * s], wb[64 * s], pacc[q]);
        }
      }
      __syncthreads();   // every wave has read its frames
#pragma unroll
      for (int q = 0; q < PQ; ++q) {
        const int tI = wave + NW * q;
        if (tI < PTILES) {
#pragma unroll
          for (int x = 0; x < 16; ++x) {
            const int m = tI * 32 + acc_row(x, lane);
            if (m < RT * T) {
              const int w = m / T, t = m - w * T;
              lds[MP + w * PROWM + t * C + o] = leaky(pacc[q][x]);
            }
          }
        }
      }
    }
    __syncthreads();
    if (wave < (RT * L1 + 31) / 32)
      conv_tile<K1, S1, T, L1>(lds + MW1, lds[MB + C + o], lds + MP, PROWM, lds + MA1, wave, lane);
    __syncthreads();
    if (wave < (RT * L2 + 31) / 32)
      conv_tile<K2, 1, L1, L2>(lds + MW2, lds[MB + 2 * C + o], lds + MA1, C * L1, lds + MA2, wave, lane);
    __syncthreads();
    if (wave < (RT * L3 + 31) / 32)
      conv_tile<K2, 1, L2, L3>(lds + MW3, lds[MB + 3 * C + o], lds + MA2, C * L2, lds + MA3, wave, lane);
    __syncthreads();
    const int lrow = tile * RT + r;
    if (o < L && lrow < rows) {   // linear_output as k_sy_net has it (N = 8: not worth a matrix-core tile)
      const float *A3 = lds + MA3 + r * C * L3;
      float acc = lds[MB + 4 * C + o];
      for (int i = 0; i < FLAT; ++i) acc += lds[MWL + o * FLAT + i] * A3[i];
      zhat[(size_t)lrow * L + o] = leaky(acc);
    }
  }
}

int launch(const float *enc, const Geo &g, int row0, int rows, const float *stream, const int32_t *valid_rows,
           float *zhat, hipStream_t s) {
  if (hipFuncSetAttribute((const void *)k_sy_play, hipFuncAttributeMaxDynamicSharedMemorySize, (int)M_BYTES) !=
      hipSuccess)
    return 90;
  const int nt = (rows + RT - 1) / RT;
  hipLaunchKernelGGL(k_sy_play, dim3(nt < MAX_PLAY_GROUPS ? nt : MAX_PLAY_GROUPS), dim3(TB), M_BYTES, s, enc, g, row0,
                     rows, stream, valid_rows, zhat);
  USV_CHECK_LAUNCH();
  return 0;
}

}  // namespace play

// diagnostics in double, two kernels, every sum in a fixed order.  k_sy_moments: block b, thread (q, l) = (tid / 8,
// tid % 8) sums rows b * 32 + q + 32 gridDim.x i of dimension l: z*, z*^2, z^, z^^2, (z^ - z*)^2; the 32 q's are
// folded in index order into moments[b][l][5].  k_sy_metrics folds the blocks in index order; the centred sums
// follow from the raw moments (doubles: the cancellation costs nothing that shows at 1e-5).
constexpr int MET_BLOCKS = 512;
__global__ __launch_bounds__(256) void k_sy_moments(const float *__restrict__ zstar, const float *__restrict__ zhat,
                                                    long long rows, double *__restrict__ moments) {
  __shared__ double red[5][256];
  const int tid = threadIdx.x, l = tid & 7, q = tid >> 3;
  double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long i = (long long)blockIdx.x * 32 + q; i < rows; i += 32LL * gridDim.x) {
    const double zs = (double)zstar[i * L + l], zh = (double)zhat[i * L + l];
    a[0] += zs;
    a[1] += zs * zs;
    a[2] += zh;
    a[3] += zh * zh;
    a[4] += (zh - zs) * (zh - zs);
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) red[k][tid] = a[k];
  __syncthreads();
  if (tid < L * 5) {
    const int ll = tid / 5, k = tid - ll * 5;
    double t = 0.0;
    for (int qq = 0; qq < 32; ++qq) t += red[k][qq * 8 + ll];
    moments[((size_t)blockIdx.x * L + ll) * 5 + k] = t;
  }
}

__global__ __launch_bounds__(64) void k_sy_metrics(const double *__restrict__ moments, int nblocks, long long rows,
                                                   const float *__restrict__ losses, int n_losses, int mini_batches,
                                                   double *__restrict__ out) {
  __shared__ double tot[L][5];
  const int tid = threadIdx.x;
  if (tid < L * 5) {
    const int ll = tid / 5, k = tid - ll * 5;
    double t = 0.0;
    for (int b = 0; b < nblocks; ++b) t += moments[((size_t)b * L + ll) * 5 + k];
    tot[ll][k] = t;
  }
  __syncthreads();
  if (tid == 0) {
    const double N = (double)rows;
    double e = 0.0, t = 0.0, h = 0.0, m = 0.0;
    for (int l = 0; l < L; ++l) {
      const double sse = tot[l][4];
      const double sst = fmax(tot[l][1] - tot[l][0] * tot[l][0] / N, 0.0);
      const double shh = fmax(tot[l][3] - tot[l][2] * tot[l][2] / N, 0.0);
      out[SY_MET_SSE + l] = sse;
      out[SY_MET_SST + l] = sst;
      out[SY_MET_R2_DIM + l] = 1.0 - sse / (sst + 1e-8);
      e += sse;
      t += sst;
      h += shh;
    }
    out[SY_MET_ZSTAR_VAR] = t / N / (double)L;
    out[SY_MET_ZHAT_VAR] = h / N / (double)L;
    out[SY_MET_R2_TOTAL] = 1.0 - e / (t + 1e-8);
    const int cnt = mini_batches < n_losses ? mini_batches : n_losses;
    for (int k = n_losses - cnt; k < n_losses; ++k) m += (double)losses[k];
    out[SY_MET_MSE] = cnt > 0 ? m / (double)cnt : 0.0;
  }
}

int check(int n, int obs_dim, int history_len, int horizon, int base) {
  if (history_len != SY_T || obs_dim < 33 || obs_dim > LZ_MAX_OBS) return 2;
  if (n <= 0 || horizon <= 0 || base < 0 || base >= SY_T - 1 + horizon) return 1;
  if ((long long)n * horizon > 0x7FFFFFFFLL / 64) return 1;   // row and float indices of the row tables fit an int
  return 0;
}
Geo geo(int n, int obs_dim, int horizon, int base) { return Geo{n, obs_dim - PRIV, horizon, T - 1 + horizon, base}; }

int groups(int rows) {
  const int nt = (rows + RT - 1) / RT;
  return nt < MAX_GROUPS ? nt : MAX_GROUPS;
}
int part_stride(int D) { return (offsets(D).n + 1 + 63) / 64 * 64; }

template <bool GRAD>
int launch_net(const float *enc, const Geo &g, int row0, int rows, const float *stream, const int32_t *valid_rows,
               const float *zstar, float *zhat, float *partials, int grid, hipStream_t s) {
  if (hipFuncSetAttribute((const void *)k_sy_net<GRAD>, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)LDS_BYTES) != hipSuccess)
    return 90;
  hipLaunchKernelGGL(k_sy_net<GRAD>, dim3(grid), dim3(TB), LDS_BYTES, s, enc, g, row0, rows, stream, valid_rows, zstar,
                     zhat, partials, part_stride(g.D));
  USV_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" {

int sysid_nparam(int obs_dim) { return obs_dim >= 33 && obs_dim <= LZ_MAX_OBS ? offsets(obs_dim - PRIV).n : -1; }

int sysid_partials_floats(int obs_dim, int rows) {
  if (sysid_nparam(obs_dim) <= 0 || rows <= 0) return -1;
  return groups(rows) * part_stride(obs_dim - PRIV);
}

int sysid_metrics_work_doubles(void) { return MET_BLOCKS * L * 5; }

int sysid_append(const float *obs, const int64_t *dones, const float *teacher, int n, int obs_dim, int history_len,
                 int horizon, int base, int s, int fill_mode, int fresh, float *stream, int32_t *valid_rows,
                 int32_t *valid_cur, float *zstar, void *stream_) {
  if (!obs || !stream || !valid_rows || !valid_cur || (teacher && !zstar)) return 1;
  if (const int rc = check(n, obs_dim, history_len, horizon, base)) return rc;
  if (s < 0 || s >= horizon || (fill_mode != SY_FILL_ZEROS && fill_mode != SY_FILL_REPEAT)) return 1;
  hipLaunchKernelGGL(k_sy_append, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream_, obs, dones, teacher,
                     geo(n, obs_dim, horizon, base), obs_dim, s, fill_mode, fresh, stream, valid_rows, valid_cur, zstar);
  USV_CHECK_LAUNCH();
  return 0;
}

int sysid_encode(const float *enc, int n, int obs_dim, int history_len, int horizon, int base, int row0, int rows,
                 const float *stream, const int32_t *valid_rows, float *zhat, void *stream_) {
  if (!enc || !stream || !valid_rows || !zhat) return 1;
  if (const int rc = check(n, obs_dim, history_len, horizon, base)) return rc;
  if (row0 < 0 || rows <= 0 || (long long)row0 + rows > (long long)n * horizon) return 1;
  const int nt = (rows + RT - 1) / RT;
  return launch_net<false>(enc, geo(n, obs_dim, horizon, base), row0, rows, stream, valid_rows, nullptr, zhat, nullptr,
                           nt < MAX_FWD_GROUPS ? nt : MAX_FWD_GROUPS, (hipStream_t)stream_);
}

int sysid_student_step(const float *enc, const float *teacher, int n, int obs_dim, int history_len, int horizon,
                       int base, int s, const float *stream, const int32_t *valid_rows, float *zhat, float *actions,
                       void *stream_) {
  if (!teacher || !actions || s < 0 || s >= horizon) return 1;
  if (const int rc = sysid_encode(enc, n, obs_dim, history_len, horizon, base, s * n, n, stream, valid_rows, zhat,
                                  stream_))
    return rc;
  hipLaunchKernelGGL(k_sy_action, dim3((n + RA - 1) / RA), dim3(ATB), 0, (hipStream_t)stream_, teacher,
                     geo(n, obs_dim, horizon, base), s, stream, zhat, actions);
  USV_CHECK_LAUNCH();
  return 0;
}

int sysid_play(const float *enc, const float *teacher, int n, int obs_dim, int history_len, int horizon, int base,
               int s, int flags, const float *stream, const int32_t *valid_rows, float *zhat, float *actions,
               void *stream_) {
  if (!teacher || !actions || !stream || !valid_rows || !zhat || s < 0 || s >= horizon) return 1;
  if (flags & ~(SY_PLAY_ZERO_LATENT | SY_PLAY_SCALAR)) return 1;
  if (const int rc = check(n, obs_dim, history_len, horizon, base)) return rc;
  if (flags & SY_PLAY_ZERO_LATENT) {
    if (hipMemsetAsync(zhat, 0, (size_t)n * L * sizeof(float), (hipStream_t)stream_) != hipSuccess) return 91;
  } else if (flags & SY_PLAY_SCALAR) {
    if (const int rc = sysid_encode(enc, n, obs_dim, history_len, horizon, base, s * n, n, stream, valid_rows, zhat,
                                    stream_))
      return rc;
  } else {
    if (!enc) return 1;
    if (const int rc = play::launch(enc, geo(n, obs_dim, horizon, base), s * n, n, stream, valid_rows, zhat,
                                    (hipStream_t)stream_))
      return rc;
  }
  hipLaunchKernelGGL(k_sy_action, dim3((n + RA - 1) / RA), dim3(ATB), 0, (hipStream_t)stream_, teacher,
                     geo(n, obs_dim, horizon, base), s, stream, zhat, actions);
  USV_CHECK_LAUNCH();
  return 0;
}

int sysid_minibatch(float *enc, float *adam_m, float *adam_v, int n, int obs_dim, int history_len, int horizon,
                    int base, int row0, int rows, float lr, int adam_step, int apply, const float *stream,
                    const int32_t *valid_rows, const float *zstar, float *partials, float *grad, float *loss_out,
                    void *stream_) {
  if (!enc || !stream || !valid_rows || !zstar || !partials || !grad) return 1;
  if (apply && (!adam_m || !adam_v || adam_step < 1)) return 1;
  if (const int rc = check(n, obs_dim, history_len, horizon, base)) return rc;
  if (row0 < 0 || rows <= 0 || (long long)row0 + rows > (long long)n * horizon) return 1;
  const Geo g = geo(n, obs_dim, horizon, base);
  const int G = groups(rows), np = offsets(g.D).n;
  if (const int rc = launch_net<true>(enc, g, row0, rows, stream, valid_rows, zstar, nullptr, partials, G,
                                      (hipStream_t)stream_))
    return rc;
  hipLaunchKernelGGL(k_sy_apply, dim3((np + 1 + 255) / 256), dim3(256), 0, (hipStream_t)stream_, enc, adam_m, adam_v,
                     partials, G, part_stride(g.D), np, rows, lr, adam_step, apply, grad, loss_out);
  USV_CHECK_LAUNCH();
  return 0;
}

int sysid_metrics(const float *enc, int n, int obs_dim, int history_len, int horizon, int base, const float *stream,
                  const int32_t *valid_rows, const float *zstar, const float *losses, int n_losses, int mini_batches,
                  float *zhat_work, double *work, double *out, void *stream_) {
  if (!zstar || !out || !zhat_work || !work || (n_losses > 0 && !losses) || n_losses < 0) return 1;
  if (const int rc = sysid_encode(enc, n, obs_dim, history_len, horizon, base, 0, n * horizon, stream, valid_rows,
                                  zhat_work, stream_))
    return rc;
  const long long rows = (long long)n * horizon;
  const int nb = (int)((rows + 31) / 32 < MET_BLOCKS ? (rows + 31) / 32 : MET_BLOCKS);
  hipLaunchKernelGGL(k_sy_moments, dim3(nb), dim3(256), 0, (hipStream_t)stream_, zstar, zhat_work, rows, work);
  USV_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_sy_metrics, dim3(1), dim3(64), 0, (hipStream_t)stream_, work, nb, rows, losses, n_losses,
                     mini_batches, out);
  USV_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
