// Default cloth forward for gfx950: operation order "v2" -- the reference's formulas re-associated into far fewer
// IEEE operations (1 division + 1 sqrt per link instead of 6 + 1) and compiled WITHOUT FMA contraction, so that
// it is bit-identical to the CPU restatement of the same order (oracle/csrc/cloth_oracle.hpp::cloth_substep_fwd_v2)
// over a whole 2000-substep step_diff, including the discrete grasp sets.  Against the reference's
// literal order (cloth.hip, mode 1) it differs by f32 round-off per substep -- see DESIGN.md "Numerical sensitivity".
// Same mapping as the other cloth kernels: one workgroup per env, one particle per lane, float4 positions
// double-buffered in LDS, one barrier per substep, per-substep checkpoints to HBM.  Bodies of 257-512 padded particles run two waves per
// SIMD: there the later-dispatched wave of each SIMD changes its issue priority inside every substep (WavePrio, cloth_common.h).
#include <type_traits>
#include "cloth_v2_force.h"

namespace ud {

constexpr int UD_V2_MAXP = 1024 + 1;   // LDS plane stride (floats; the kernels refuse Pp > 1024).  Odd, as in the adjoint: a stride that is a multiple
                                       // of 64 lets the compiler fuse the x and y reads of a neighbour into ds_read2st64, whose results then need
                                       // register moves to regroup them by link pair (24 single reads and 10 moves against 16 reads and 22 moves)

typedef __attribute__((address_space(1))) float* gfptr;
typedef __attribute__((address_space(1))) uint8_t* gbptr;
// base[off / 4] = val for a uniform base and a loop-invariant 32-bit lane offset in bytes: the "SGPR base + VGPR offset" form of
// the global store, no address arithmetic.  The empty asm keeps the offset 32 bits wide inside the loop; hoisted out of it,
// its 64-bit extension costs a v_lshl_add_u64 per store and substep instead.
__device__ __forceinline__ void st_lane(gfptr base, unsigned off, float val) {
  asm volatile("" : "+v"(off));
  *(gfptr)((__attribute__((address_space(1))) char*)base + off) = val;
}

// x, from here on in a vector register (opaque to the compiler, which would otherwise keep a uniform value in a scalar one)
__device__ __forceinline__ void vreg(float& x) { asm volatile("" : "+v"(x)); }

template <typename G, typename T>
__device__ __forceinline__ G uniform_ptr(T* p) {
  const unsigned long long u = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((int)(unsigned)u), hi = __builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
  return (G)(((unsigned long long)hi << 32) | lo);
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// CKPT / GRASP: the call records checkpoints (ClothFwdArgs::ckpt) / grasp sets (::grasp); chosen by the launch function, so a
// forward-only call carries neither block.  The substep loop is unrolled by two: with the parity of the LDS double buffer a
// compile-time constant, buffer and plane offsets are immediates of the ds instructions and a neighbour's address is one
// loop-invariant register.
// ISV: the launch's constants passed cloth_isv_consts_ok, so isV comes from exact_math.h's select-free 1 / sqrt; the launch function runs
// the `_anyc` kernels (the compiler's own 1.0f / sqrtf) where they do not.
template <bool CKPT, bool GRASP, bool ISV>
__device__ __forceinline__ void cloth_rollout_fwd_v2_body(const ClothFwdArgs& a) {
  extern __shared__ float ldsf[];  // Xs[2][3][UD_V2_MAXP], double-buffered by substep parity
  const ClothConst c = a.c;
  const int i = threadIdx.x, b = blockIdx.x;
  const int P = c.P, Pp = c.Pp, S = c.S, B = a.B, T = a.T;
  const bool live = i < P;
  int nbs[8];
#pragma unroll
  for (int l = 0; l < 8; ++l) { const int j = a.nbr[l * Pp + i]; nbs[l] = j >= 0 ? j : i; }
  float x[3] = {0.f, 0.f, 0.f}, v[3] = {0.f, 0.f, 0.f};
  if (live) {
#pragma unroll
    for (int d = 0; d < 3; ++d) { x[d] = a.x[((size_t)b * P + i) * 3 + d]; v[d] = a.v[((size_t)b * P + i) * 3 + d]; }
  }
  float ps[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) ps[d] = a.prim[b * 8 + d];
  float k = a.k[b], mu = a.mu[b];
  float kLs = k / c.Ls, kLd = k / c.Ld;   // k / L0 with the rest lengths of cloth_simulator.py:61-63
  // The stiffness and the friction coefficient multiply per-lane values in the link code: there a scalar operand costs a second
  // issue slot at 2 waves/SIMD, so they live in vector registers for the whole launch.  Measured: -1.8 % of the kernel.
  // The same for dt / damp / max_v / g or for the bounds of the |r|^2 clip made it slower (profiles/r09_ablation.txt).
  vreg(k); vreg(mu); vreg(kLs); vreg(kLd);
  const f2 kL2 = {kLs, kLd};
  GraspThr th0, th1;
  th0.init(ps[3]); th1.init(ps[7]);
  float thr0 = th0.first, thr1 = th1.first;   // loop-carried: `rest` from the second substep on, instead of a select per substep
  const size_t rec = cloth_rec_floats(Pp);
  // records and grasp sets are addressed as a uniform base, moved once per substep, plus loop-invariant lane offsets (bytes)
  gfptr rp = CKPT ? uniform_ptr<gfptr>(a.ckpt + (size_t)b * cloth_env_records(T, S) * rec) : nullptr;
  gbptr gp = GRASP ? uniform_ptr<gbptr>(a.grasp + (size_t)b * 2 * P) : nullptr;
  const size_t gstride = (size_t)B * 2 * P;
  unsigned ox[3], ov[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) { ox[d] = 4u * (unsigned)(d * Pp + i); ov[d] = 4u * (unsigned)((3 + d) * Pp + i); }
  float act[8];
  WavePrio wp;
  wp.init(Pp);
  // one substep on LDS buffer PAR; LOSE: this wave loses the SIMD's arbitration to its partner (wave-uniform, decided once below)
  auto substep = [&](auto par, auto lose) {
    constexpr int PAR = decltype(par)::value;
    constexpr bool LOSE = decltype(lose)::value;
    float* Xs = ldsf + PAR * (3 * UD_V2_MAXP);
    Xs[i] = x[0]; Xs[UD_V2_MAXP + i] = x[1]; Xs[2 * UD_V2_MAXP + i] = x[2];
    if (CKPT) {
#pragma unroll
      for (int d = 0; d < 3; ++d) { st_lane(rp, ox[d], x[d]); st_lane(rp, ov[d], v[d]); }
      if (i == 0) {
#pragma unroll
        for (int d = 0; d < 8; ++d) rp[6 * Pp + d] = ps[d];
      }
      rp += rec;
    }
    // everything that needs no neighbour goes between the LDS write and the barrier, where it hides the write
    // latency and the arrival skew of the other waves
    float vv[3], x2[3];
    bool m0, m1;
    grip_own(x, ps, act, thr0, thr1, m0, m1, x2);
    thr0 = th0.rest; thr1 = th1.rest;
    const float sV = v[0] * v[0] + v[2] * v[2] + c.eps;
    const float isV = ISV ? rcp_sqrt_rn_rsq(sV) : 1.0f / sqrtf(sV);
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int d = 0; d < 4; ++d) ps[g * 4 + d] = clipf(ps[g * 4 + d] + (d < 3 ? act[g * 4 + d] : 0.f), 0.f, 1.f);  // :322-323
    if (LOSE) wp.up();
    __syncthreads();
    force_v2<UD_V2_MAXP>(c, nbs, Xs, k, kL2, mu, x, v, isV, vv);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      vv[d] = m0 ? act[3] * vv[d] : vv[d];
      vv[d] = m1 ? act[7] * vv[d] : vv[d];
    }
    if (GRASP) {
      if (live) { gp[i] = m0; gp[P + i] = m1; }
      gp += gstride;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {   // :326-329
      const float vc = clipf(vv[d], -c.max_v, c.max_v);
      x[d] = clipf(x2[d], 0.f, 1.f) + c.dt * vc;
      v[d] = vc;
    }
    // the hand-over: the force and the update are done, the partner wave takes the SIMD while this one writes the next substep's
    // positions and record and runs its own-particle block (the best of six places tried, profiles/r10_ablation.txt)
    if (LOSE) wp.drop();
  };
  auto rollout = [&](auto lose) {
    for (int t = 0; t < T; ++t) {
      macro_action_f(a.actions + ((size_t)t * B + b) * 8, act);
      int s = 0;
      for (; s + 1 < S; s += 2) {
        substep(std::integral_constant<int, 0>(), lose);
        substep(std::integral_constant<int, 1>(), lose);
      }
      if (s < S) {   // odd S: the next macro step starts on buffer 0 again, whose readers of this substep must be done first
        substep(std::integral_constant<int, 0>(), lose);
        __syncthreads();
      }
      if (live) {
        const size_t o = (((size_t)t * B + b) * P + i) * 3;
        if (a.x_list) { a.x_list[o] = x[0]; a.x_list[o + 1] = x[1]; a.x_list[o + 2] = x[2]; }
        if (a.v_list) { a.v_list[o] = v[0]; a.v_list[o + 1] = v[1]; a.v_list[o + 2] = v[2]; }
      }
      if (a.prim_list && i == 0) {
#pragma unroll
        for (int d = 0; d < 8; ++d) a.prim_list[((size_t)t * B + b) * 8 + d] = ps[d];
      }
    }
  };
  // two copies of the loop, chosen per wave: every wave passes the same barriers in either
  if (wp.lose) rollout(std::true_type()); else rollout(std::false_type());
  if (live) {
    const size_t o = ((size_t)b * P + i) * 3;
#pragma unroll
    for (int d = 0; d < 3; ++d) { a.x_out[o + d] = x[d]; a.v_out[o + d] = v[d]; }
  }
  if (i == 0) {
#pragma unroll
    for (int d = 0; d < 8; ++d) a.prim_out[b * 8 + d] = ps[d];
  }
  if (CKPT) {   // rp has reached the last record
#pragma unroll
    for (int d = 0; d < 3; ++d) { rp[d * Pp + i] = x[d]; rp[(3 + d) * Pp + i] = v[d]; }
    if (i == 0) {
#pragma unroll
      for (int d = 0; d < 8; ++d) rp[6 * Pp + d] = ps[d];
    }
  }
}


// One kernel per variant, each under a plain name (profiles and counter passes are keyed by kernel name): the training forward
// (checkpoints, no grasp sets) keeps the name it always had.
__global__ void __launch_bounds__(512) cloth_rollout_fwd_v2_kernel(ClothFwdArgs a) { cloth_rollout_fwd_v2_body<true, false, true>(a); }
__global__ void __launch_bounds__(512) cloth_rollout_fwd_v2_eval_kernel(ClothFwdArgs a) { cloth_rollout_fwd_v2_body<false, false, true>(a); }
__global__ void __launch_bounds__(512) cloth_rollout_fwd_v2_grasp_kernel(ClothFwdArgs a) { cloth_rollout_fwd_v2_body<false, true, true>(a); }
__global__ void __launch_bounds__(512) cloth_rollout_fwd_v2_ckpt_grasp_kernel(ClothFwdArgs a) { cloth_rollout_fwd_v2_body<true, true, true>(a); }
// the same four for constants outside cloth_isv_consts_ok
__global__ void __launch_bounds__(512) cloth_rollout_fwd_v2_anyc_kernel(ClothFwdArgs a) { cloth_rollout_fwd_v2_body<true, false, false>(a); }
__global__ void __launch_bounds__(512) cloth_rollout_fwd_v2_eval_anyc_kernel(ClothFwdArgs a) { cloth_rollout_fwd_v2_body<false, false, false>(a); }
__global__ void __launch_bounds__(512) cloth_rollout_fwd_v2_grasp_anyc_kernel(ClothFwdArgs a) { cloth_rollout_fwd_v2_body<false, true, false>(a); }
__global__ void __launch_bounds__(512) cloth_rollout_fwd_v2_ckpt_grasp_anyc_kernel(ClothFwdArgs a) { cloth_rollout_fwd_v2_body<true, true, false>(a); }

void cloth_launch_fwd_v2(const ClothFwdArgs& a, hipStream_t stream) {
  const size_t shmem = (size_t)2 * 3 * UD_V2_MAXP * sizeof(float);
  auto* kern = a.ckpt ? (a.grasp ? cloth_rollout_fwd_v2_ckpt_grasp_kernel : cloth_rollout_fwd_v2_kernel)
                      : (a.grasp ? cloth_rollout_fwd_v2_grasp_kernel : cloth_rollout_fwd_v2_eval_kernel);
  if (!cloth_isv_consts_ok(a.c))
    kern = a.ckpt ? (a.grasp ? cloth_rollout_fwd_v2_ckpt_grasp_anyc_kernel : cloth_rollout_fwd_v2_anyc_kernel)
                  : (a.grasp ? cloth_rollout_fwd_v2_grasp_anyc_kernel : cloth_rollout_fwd_v2_eval_anyc_kernel);
  hipLaunchKernelGGL(kern, dim3(a.B), dim3(a.c.Pp), shmem, stream, a);
}

}  // namespace ud
