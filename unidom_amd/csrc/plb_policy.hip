// PLB closed-loop policy: the reference's Taichi MLP (GenORM policy/pbm/plb/engine/nn/mlp.py:63-127) for B envs, float64, forward and
// adjoint.  Handle-free: the caller owns every buffer; nothing is allocated, nothing synchronises, no atomics.
//
//   h_0[b]   = observation, d_0 = 6 obs_num + 7 P:  x, v * velocity_weight of particles 0, obs_step, 2 obs_step, ...; then per primitive
//              its position and its rotation (w, x, y, z)                                            (input_particles / input_primitives)
//   h_{l+1}  = act(W_l h_l + b_l), W_l [d_{l+1}, d_l] row-major; act = relu / tanh, none on the last layer         (weights / bias)
//   action   = clamp(h_last, -1, 1)                                                                                    (set_action)
//   params   = W_0, b_0, W_1, b_1, ... flat (get_params); env b reads params + b * param_stride (0 = one policy for all envs)
//
// Tape (one row per env, doubles): h_0 | h_1 .. h_{L-1} after the activation | h_L before the clamp | d_1 words the backward hands from
// its first launch to its second.
//
// Launch plan and ownership (DESIGN.md "PLB policy").  Every output element is written by exactly one thread and every sum runs in an
// order fixed by the shapes alone, so two runs give the same bits.
//   forward, taped:   plb_policy_l0_fwd   grid (ceil(d_1 / 4), B) x 256: a wave owns output row i of layer 0, lanes run along j with four
//                                         accumulators each, one xor butterfly over the wave; workgroup 0 of an env also writes h_0
//                     plb_policy_tail_fwd grid (B) x 1024: layers 1 .. L-1 and the clamp, activations in LDS, same row sum
//   forward, no tape: plb_policy_tail_fwd alone from layer 0 (there is nowhere to put h_1 between two launches); same row sums, same bits
//   backward:         plb_policy_tail_bwd grid (B) x 1024 (L >= 2): clamp mask, then layers L-1 .. 1: thread (rg, c) owns column j = c of
//                                         rows i = rg mod 4: g_h[j] += W[i,j] g[i] and g_W[i,j] += g[i] h[j] in one pass over W; the four
//                                         row groups are summed ((0+1)+(2+3)); leaves g on layer 0's pre-activation in the tape row
//                     plb_policy_l0_bwd   grid (ceil(d_0 / 32), B) x 256: the same pass over a 32-column slab of W_0 with eight row groups,
//                                         then scatters g_h0 into g_x / g_v / g_prim_*; the zeros of the unobserved particles are
//                                         spread over the env's workgroups; workgroup 0 adds g_b0
// A row whose cotangent is exactly zero (a dead ReLU unit, a clamped output) is skipped in the backward passes: it would add +0 to
// g_h and to g_W, so only the traffic changes.
// Built with -ffp-contract=off like the rest of the f64 path: every product and sum below is rounded once.
#include "common.h"

namespace ud {

constexpr int POL_MAX_LAYERS = 4;       // 0 to 3 hidden layers
constexpr int POL_MAX_WIDTH = 1024;     // d_1 .. d_L
constexpr int POL_MAX_D0 = 4096;        // the observation
constexpr int POL_MAX_B = 65535;        // grid.y
constexpr int POL_L0F_ROWS = 4;         // rows (= waves) per workgroup of plb_policy_l0_fwd
constexpr int POL_L0B_COLS = 32, POL_L0B_RG = 8;   // plb_policy_l0_bwd: 32 columns x 8 row groups
constexpr int POL_TB_COLS = 256, POL_TB_RG = 4;    // plb_policy_tail_bwd: 256 columns x 4 row groups

struct PolDims {
  int n_layer, act, d[POL_MAX_LAYERS + 1];
  long woff[POL_MAX_LAYERS], boff[POL_MAX_LAYERS], n_params;   // a parameter row
  long hoff[POL_MAX_LAYERS + 1], goff, tstride;                 // a tape row
};

struct PolObs {
  int N, P, obs_step, obs_num;
  double vw;
};

// element k of env b's observation (mlp.py:68-86)
__device__ __forceinline__ double pol_obs(const PolObs& o, int b, int k, const double* __restrict__ x, const double* __restrict__ v,
                                          const double* __restrict__ pp, const double* __restrict__ pr) {
  const int np = 6 * o.obs_num;
  if (k < np) {
    const int i = k / 6, c = k - 6 * i;
    const long e = ((long)b * o.N + (long)i * o.obs_step) * 3;
    return c < 3 ? x[e + c] : v[e + c - 3] * o.vw;
  }
  const int q = k - np, p = q / 7, c = q - 7 * p;
  const long pi = (long)b * o.P + p;
  return c < 3 ? pp[pi * 3 + c] : pr[pi * 4 + c - 3];
}

// sum_j w[j] h[j] over one wave: lane l takes j = l, l + 64, ... into four accumulators (a tail of fewer than four into the first), then
// ((a0 + a1) + (a2 + a3)) and a xor butterfly 32, 16, .., 1 (a + b == b + a: every lane ends with the same bits)
__device__ __forceinline__ double pol_row_dot(const double* __restrict__ w, const double* h, int n, int lane) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int j = lane;
  for (; j + 192 < n; j += 256) {
    a0 += w[j] * h[j];
    a1 += w[j + 64] * h[j + 64];
    a2 += w[j + 128] * h[j + 128];
    a3 += w[j + 192] * h[j + 192];
  }
  for (; j < n; j += 64) a0 += w[j] * h[j];
  double s = (a0 + a1) + (a2 + a3);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  return s;
}

__device__ __forceinline__ double pol_act(int act, double pre) { return act == 1 ? tanh(pre) : (pre < 0.0 ? 0.0 : pre); }
// d act / d pre from the stored output h = act(pre): relu 1 where h > 0; tanh 1 - h^2
__device__ __forceinline__ double pol_dact(int act, double h) { return act == 1 ? 1.0 - h * h : (h > 0.0 ? 1.0 : 0.0); }
__device__ __forceinline__ double pol_clamp(double h) { return h < -1.0 ? -1.0 : (h > 1.0 ? 1.0 : h); }

// output i of layer l from its pre-activation: the tape entry, the action on the last layer; returns h_{l+1}[i]
__device__ __forceinline__ double pol_emit(const PolDims& D, int l, int i, double pre, double* trow, double* arow) {
  const bool last = l == D.n_layer - 1;
  const double h = last ? pre : pol_act(D.act, pre);
  if (trow) trow[D.hoff[l + 1] + i] = h;
  if (last) arow[i] = pol_clamp(h);
  return h;
}

__global__ void __launch_bounds__(256) plb_policy_l0_fwd(PolDims D, PolObs O, const double* __restrict__ x, const double* __restrict__ v,
                                                         const double* __restrict__ pp, const double* __restrict__ pr,
                                                         const double* __restrict__ params, long pstride, double* tape, double* action) {
  extern __shared__ double pol_lds[];
  double* h0 = pol_lds;
  const int b = blockIdx.y, tid = threadIdx.x, d0 = D.d[0], d1 = D.d[1];
  double* trow = tape + (long)b * D.tstride;
  for (int k = tid; k < d0; k += 256) {
    const double val = pol_obs(O, b, k, x, v, pp, pr);
    h0[k] = val;
    if (blockIdx.x == 0) trow[D.hoff[0] + k] = val;
  }
  __syncthreads();
  const int i = blockIdx.x * POL_L0F_ROWS + (tid >> 6), lane = tid & 63;
  if (i >= d1) return;
  const double* P = params + (long)b * pstride;
  const double pre = pol_row_dot(P + D.woff[0] + (long)i * d0, h0, d0, lane) + P[D.boff[0] + i];
  if (lane == 0) pol_emit(D, 0, i, pre, trow, action + (long)b * D.d[D.n_layer]);
}

// layers start .. L-1 of one env; start = 0 gathers the observation itself, start = 1 reads h_1 from the tape.  LDS: max(d_start, 1024) + 1024
__global__ void __launch_bounds__(1024) plb_policy_tail_fwd(PolDims D, PolObs O, int start, const double* __restrict__ x,
                                                            const double* __restrict__ v, const double* __restrict__ pp,
                                                            const double* __restrict__ pr, const double* __restrict__ params, long pstride,
                                                            double* tape, double* action) {
  extern __shared__ double pol_lds[];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  double* cur = pol_lds;
  double* nxt = pol_lds + (D.d[start] > POL_MAX_WIDTH ? D.d[start] : POL_MAX_WIDTH);
  double* trow = tape ? tape + (long)b * D.tstride : nullptr;
  double* arow = action + (long)b * D.d[D.n_layer];
  const double* P = params + (long)b * pstride;
  if (start == 0) {
    for (int k = tid; k < D.d[0]; k += 1024) {
      const double val = pol_obs(O, b, k, x, v, pp, pr);
      cur[k] = val;
      if (trow) trow[D.hoff[0] + k] = val;
    }
  } else {
    for (int k = tid; k < D.d[start]; k += 1024) cur[k] = trow[D.hoff[start] + k];
  }
  __syncthreads();
  for (int l = start; l < D.n_layer; ++l) {
    const int dk = D.d[l], dn = D.d[l + 1];
    for (int i = wave; i < dn; i += 16) {
      const double pre = pol_row_dot(P + D.woff[l] + (long)i * dk, cur, dk, lane) + P[D.boff[l] + i];
      if (lane == 0) nxt[i] = pol_emit(D, l, i, pre, trow, arow);
    }
    __syncthreads();
    double* t = cur;
    cur = nxt;
    nxt = t;
  }
}

// cotangent of the last layer's output behind the clamp: passes where |h| <= 1, equality included
__device__ __forceinline__ double pol_clamp_bwd(double h, double g) { return fabs(h) <= 1.0 ? g : 0.0; }

__global__ void __launch_bounds__(1024) plb_policy_tail_bwd(PolDims D, const double* __restrict__ params, long pstride, double* tape,
                                                            const double* __restrict__ g_action, double* g_params) {
  __shared__ double gbuf[2][POL_MAX_WIDTH], hl[POL_MAX_WIDTH], part[POL_TB_RG][POL_TB_COLS];
  const int b = blockIdx.x, tid = threadIdx.x, L = D.n_layer, dL = D.d[L];
  double* trow = tape + (long)b * D.tstride;
  const double* P = params + (long)b * pstride;
  double* G = g_params + (long)b * D.n_params;
  double* gA = gbuf[0];
  double* gB = gbuf[1];
  for (int i = tid; i < dL; i += 1024) gA[i] = pol_clamp_bwd(trow[D.hoff[L] + i], g_action[(long)b * dL + i]);
  __syncthreads();
  const int c = tid & (POL_TB_COLS - 1), rg = tid / POL_TB_COLS;
  for (int l = L - 1; l >= 1; --l) {
    const int dk = D.d[l], dn = D.d[l + 1];
    for (int j = tid; j < dk; j += 1024) hl[j] = trow[D.hoff[l] + j];
    for (int i = tid; i < dn; i += 1024) G[D.boff[l] + i] += gA[i];
    __syncthreads();
    const double* W = P + D.woff[l];
    double* GW = G + D.woff[l];
    for (int jb = 0; jb < dk; jb += POL_TB_COLS) {
      const int j = jb + c;
      double acc = 0.0;
      if (j < dk) {
        const double hj = hl[j];
#pragma unroll 4
        for (int i = rg; i < dn; i += POL_TB_RG) {
          const double gi = gA[i];
          if (gi == 0.0) continue;
          const long e = (long)i * dk + j;
          acc += W[e] * gi;
          GW[e] += gi * hj;
        }
      }
      part[rg][c] = acc;
      __syncthreads();
      if (rg == 0 && j < dk) gB[j] = ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) * pol_dact(D.act, hl[j]);
      __syncthreads();
    }
    double* t = gA;
    gA = gB;
    gB = t;
  }
  for (int i = tid; i < D.d[1]; i += 1024) trow[D.goff + i] = gA[i];
}

__global__ void __launch_bounds__(256) plb_policy_l0_bwd(PolDims D, PolObs O, const double* __restrict__ params, long pstride,
                                                         const double* __restrict__ tape, const double* __restrict__ g_action, double* g_x,
                                                         double* g_v, double* g_pp, double* g_pr, double* g_params) {
  __shared__ double g[POL_MAX_WIDTH], part[POL_L0B_RG][POL_L0B_COLS];
  const int b = blockIdx.y, tid = threadIdx.x, d0 = D.d[0], d1 = D.d[1];
  const double* trow = tape + (long)b * D.tstride;
  const double* P = params + (long)b * pstride;
  double* G = g_params + (long)b * D.n_params;
  if (D.n_layer == 1) {
    for (int i = tid; i < d1; i += 256) g[i] = pol_clamp_bwd(trow[D.hoff[1] + i], g_action[(long)b * d1 + i]);
  } else {
    for (int i = tid; i < d1; i += 256) g[i] = trow[D.goff + i];
  }
  __syncthreads();
  if (blockIdx.x == 0)
    for (int i = tid; i < d1; i += 256) G[D.boff[0] + i] += g[i];
  const int c = tid & (POL_L0B_COLS - 1), rg = tid / POL_L0B_COLS, j = blockIdx.x * POL_L0B_COLS + c;
  double acc = 0.0;
  if (j < d0) {
    const double hj = trow[D.hoff[0] + j];
#pragma unroll 4
    for (int i = rg; i < d1; i += POL_L0B_RG) {
      const double gi = g[i];
      if (gi == 0.0) continue;
      const long e = D.woff[0] + (long)i * d0 + j;
      acc += P[e] * gi;
      G[e] += gi * hj;
    }
  }
  part[rg][c] = acc;
  __syncthreads();
  if (rg == 0 && j < d0) {
    const double gh = ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) + ((part[4][c] + part[5][c]) + (part[6][c] + part[7][c]));
    const int np = 6 * O.obs_num;
    if (j < np) {
      const int i = j / 6, k = j - 6 * i;
      const long e = ((long)b * O.N + (long)i * O.obs_step) * 3;
      if (k < 3) g_x[e + k] = gh;
      else g_v[e + k - 3] = gh * O.vw;
    } else {
      const int q = j - np, p = q / 7, k = q - 7 * p;
      const long pi = (long)b * O.P + p;
      if (k < 3) g_pp[pi * 3 + k] = gh;
      else g_pr[pi * 4 + k - 3] = gh;
    }
  }
  // the unobserved particles' zeros, spread over the env's workgroups
  const long base = (long)b * O.N * 3;
  for (int e = blockIdx.x * 256 + tid; e < 3 * O.N; e += gridDim.x * 256) {
    const int n = e / 3;
    if (n % O.obs_step != 0 || n / O.obs_step >= O.obs_num) {
      g_x[base + e] = 0.0;
      g_v[base + e] = 0.0;
    }
  }
}

// the shape arguments of both calls: fills D; false (with the error text) when they are outside what the kernels cover
static bool pol_shapes(const char* who, int B, int N, int P, int obs_step, int obs_num, int n_layer, const int* dims, int activation,
                       PolDims& D) {
  if (!dims || n_layer < 1 || n_layer > POL_MAX_LAYERS) {
    set_error("%s: n_layer=%d outside [1, %d] (or dims is null)", who, n_layer, POL_MAX_LAYERS);
    return false;
  }
  if (B < 1 || B > POL_MAX_B || N < 1 || N > (1 << 28) || P < 0 || P > 64 || obs_num < 0 || (activation != 0 && activation != 1)) {
    set_error("%s: bad argument (B=%d in [1, %d], N=%d, P=%d in [0, 64], obs_num=%d, activation=%d in {0, 1})", who, B, POL_MAX_B, N, P, obs_num,
              activation);
    return false;
  }
  if (obs_step < 1) {
    set_error("%s: obs_step=%d below 1", who, obs_step);
    return false;
  }
  if (obs_num > 0 && (long)(obs_num - 1) * obs_step >= N) {
    set_error("%s: observed particle (obs_num - 1) * obs_step = %ld is outside N=%d", who, (long)(obs_num - 1) * obs_step, N);
    return false;
  }
  if (dims[0] < 1 || dims[0] > POL_MAX_D0) {
    set_error("%s: dims[0]=%d outside [1, %d]", who, dims[0], POL_MAX_D0);
    return false;
  }
  if ((long)dims[0] != 6L * obs_num + 7L * P) {
    set_error("%s: dims[0]=%d is not 6 obs_num + 7 P = %ld", who, dims[0], 6L * obs_num + 7L * P);
    return false;
  }
  for (int l = 1; l <= n_layer; ++l)
    if (dims[l] < 1 || dims[l] > POL_MAX_WIDTH) {
      set_error("%s: dims[%d]=%d outside [1, %d]", who, l, dims[l], POL_MAX_WIDTH);
      return false;
    }
  D.n_layer = n_layer;
  D.act = activation;
  long po = 0, to = 0;
  for (int l = 0; l <= n_layer; ++l) {
    D.d[l] = dims[l];
    D.hoff[l] = to;
    to += dims[l];
    if (l < n_layer) {
      D.woff[l] = po;
      po += (long)dims[l + 1] * dims[l];
      D.boff[l] = po;
      po += dims[l + 1];
    }
  }
  D.n_params = po;
  D.goff = to;
  D.tstride = to + dims[1];
  return true;
}

}  // namespace ud

using namespace ud;

extern "C" {

size_t ud_plb_policy_n_params(int n_layer, const int* dims) {
  if (!dims || n_layer < 1 || n_layer > POL_MAX_LAYERS) return 0;
  size_t n = 0;
  for (int l = 0; l < n_layer; ++l) {
    if (dims[l] < 1 || dims[l + 1] < 1) return 0;
    n += (size_t)dims[l + 1] * dims[l] + dims[l + 1];
  }
  return n;
}

size_t ud_plb_policy_tape_bytes(int B, int n_layer, const int* dims) {
  if (!dims || B < 1 || n_layer < 1 || n_layer > POL_MAX_LAYERS) return 0;
  size_t n = 0;
  for (int l = 0; l <= n_layer; ++l) {
    if (dims[l] < 1) return 0;
    n += dims[l];
  }
  return (size_t)B * (n + dims[1]) * sizeof(double);
}

int ud_plb_policy_fwd(int B, int N, int P, int obs_step, int obs_num, int n_layer, const int* dims, int activation, double velocity_weight,
                      const double* x, const double* v, const double* prim_pos, const double* prim_rot, const double* params,
                      long param_stride, double* action, void* tape, void* stream) {
  PolDims D;
  if (!pol_shapes("ud_plb_policy_fwd", B, N, P, obs_step, obs_num, n_layer, dims, activation, D)) return UD_ERR_INVALID;
  if (!x || !v || (P > 0 && (!prim_pos || !prim_rot)) || !params || !action || (param_stride != 0 && param_stride < D.n_params)) {
    set_error("ud_plb_policy_fwd: bad argument (x, v, prim_pos, prim_rot, params and action must not be null; param_stride=%ld is 0 or >= %ld)",
              param_stride, D.n_params);
    return UD_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const PolObs O{N, P, obs_step, obs_num, velocity_weight};
  int start = 0;
  if (tape) {
    hipLaunchKernelGGL(plb_policy_l0_fwd, dim3((unsigned)((D.d[1] + POL_L0F_ROWS - 1) / POL_L0F_ROWS), B), dim3(256),
                       (size_t)D.d[0] * sizeof(double), st, D, O, x, v, prim_pos, prim_rot, params, param_stride, (double*)tape, action);
    start = 1;
  }
  if (start < n_layer) {
    const size_t lds = (size_t)((D.d[start] > POL_MAX_WIDTH ? D.d[start] : POL_MAX_WIDTH) + POL_MAX_WIDTH) * sizeof(double);
    hipLaunchKernelGGL(plb_policy_tail_fwd, dim3(B), dim3(1024), lds, st, D, O, start, x, v, prim_pos, prim_rot, params, param_stride,
                       (double*)tape, action);
  }
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

int ud_plb_policy_bwd(int B, int N, int P, int obs_step, int obs_num, int n_layer, const int* dims, int activation, double velocity_weight,
                      const double* params, long param_stride, void* tape, const double* g_action, double* g_x, double* g_v,
                      double* g_prim_pos, double* g_prim_rot, double* g_params, void* stream) {
  PolDims D;
  if (!pol_shapes("ud_plb_policy_bwd", B, N, P, obs_step, obs_num, n_layer, dims, activation, D)) return UD_ERR_INVALID;
  if (!params || !tape || !g_action || !g_x || !g_v || (P > 0 && (!g_prim_pos || !g_prim_rot)) || !g_params ||
      (param_stride != 0 && param_stride < D.n_params)) {
    set_error("ud_plb_policy_bwd: bad argument (no pointer may be null; param_stride=%ld is 0 or >= %ld)", param_stride, D.n_params);
    return UD_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const PolObs O{N, P, obs_step, obs_num, velocity_weight};
  if (n_layer > 1) hipLaunchKernelGGL(plb_policy_tail_bwd, dim3(B), dim3(1024), 0, st, D, params, param_stride, (double*)tape, g_action, g_params);
  hipLaunchKernelGGL(plb_policy_l0_bwd, dim3((unsigned)((D.d[0] + POL_L0B_COLS - 1) / POL_L0B_COLS), B), dim3(256), 0, st, D, O, params,
                     param_stride, (const double*)tape, g_action, g_x, g_v, g_prim_pos, g_prim_rot, g_params);
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

}  // extern "C"
