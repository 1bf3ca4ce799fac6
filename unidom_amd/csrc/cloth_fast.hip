// Fast cloth rollout kernels for gfx950: mode 2's forward here, the one-workgroup adjoint of modes 0, 2 and 3 in cloth_fast_bwd.hip
// (the reference-operation-order kernels are in cloth.hip).
//
// Same mapping as cloth.hip (one workgroup per env, one particle per lane, whole T x substeps rollout in one
// launch, per-substep checkpoints in HBM) but the arithmetic is restructured for the CU, not for bit-identity:
//   forward   the spring force is evaluated as  f = r * (k/L0 - k/|r|)  (= k r/|r| (|r|-L0)/L0 of
//             cloth_simulator.py:267-268) with v_rsq_f32, i.e. 1 transcendental + 4 FMAs per link and component
//             triple instead of 6 IEEE divisions + 1 IEEE sqrt; x is staged as float4 in LDS (one ds_read_b128
//             per neighbour); the dead static-friction branch (:293-306, never taken because
//             sqrt(.+small_num) > small_num) is dropped; FMA contraction is on.
//   backward  the reference normalises cotangents six times per substep (norm_grad, :189-194, applied at
//             :223-224 twice and :331-334).  Every map between two normalisations is linear, so all six norms
//             are functions of NINE block-wide sums of the incoming cotangent that can be taken BEFORE the
//             stencil barrier: |gx|^2, |gv|^2, |Dx gx|^2, |Dv gv|^2, <Dv gv, Dv gx>, |Dv gx|^2 and the last three
//             restricted to the particles gripper 1 holds (Dx, Dv = the clip masks of :326-327; Dv is read off
//             the NEXT checkpoint record, whose v is clip(v5)).  That turns 3 dependent reduction rounds + 6
//             barriers per substep into 1 round + 2 barriers.
// Results agree with the reference-order kernels / the CPU oracle to f32 round-off (tests/test_cloth_gpu.py,
// tolerances written there); the discrete grasp test |x - pos| <= radius keeps its exact form.
#include "cloth_fast_adj.h"

namespace ud {

struct FastInter {
  float F1, cF, muF, xV, yV, isV, tf;   // friction block
  float r0[8], r1[8], r2[8];            // link vectors (reused by the spring adjoint)
  float w[8];                           // 1/L0 - 1/|r|            (spring coefficient / k)
  float c2k[8];                         // k / |r|^3, or 0 where clip(|r|^2, 1e-12) is active
};

// spring + gravity + ground friction + damping: (x, v, neighbours in X4) -> v3 ; keeps the adjoint's inputs
template <bool KEEP>
// nbs[l] = neighbour index, or the particle itself where the lattice has no neighbour: then r == 0 exactly and the
// (finite) coefficient multiplies zeros, so neither the force nor its adjoint needs a select.
__device__ __forceinline__ void force_fast(const ClothConst& c, const int* nbs, const float4* X4, float k, float iLs,
                                           float iLd, float mu, const float* x, const float* v, float* v3, FastInter* in) {
  float F0 = 0.f, F1 = 0.f, F2 = 0.f;
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const float4 xj = X4[nbs[l]];
    const float r0 = xj.x - x[0], r1 = xj.y - x[1], r2 = xj.z - x[2];
    const float s2 = r0 * r0 + r1 * r1 + r2 * r2;
    const float inv = rsq(fmaxf(s2, 1e-12f));
    const float w = ((l < 4) ? iLs : iLd) - inv;
    const float coef = k * w;
    F0 += coef * r0; F1 += coef * r1; F2 += coef * r2;
    if (KEEP) {
      in->r0[l] = r0; in->r1[l] = r1; in->r2[l] = r2; in->w[l] = w;
      in->c2k[l] = (s2 > 1e-12f) ? k * inv * inv * inv : 0.f;
    }
  }
  F1 -= c.g;                                        // :278
  const float v1y = v[1] - c.gdt;                   // :259
  const bool fm = x[1] <= c.eps;                    // :281
  const float cF = fminf(F1, 0.f);
  const float muF = -(mu * cF);                     // :282
  const float xV = v[0], yV = v[2];
  const float isV = rsq(xV * xV + yV * yV + c.eps); // :285
  const float tf = fm ? muF * isV : 0.f;            // :288-290 (sV > small_num always holds)
  const float Ax = F0 - tf * xV, Az = F2 - tf * yV;
  v3[0] = (xV + Ax * c.dt) * c.damp;                // :308-309
  v3[1] = (v1y + F1 * c.dt) * c.damp;
  v3[2] = (yV + Az * c.dt) * c.damp;
  if (KEEP) { in->F1 = F1; in->cF = cF; in->muF = muF; in->xV = xV; in->yV = yV; in->isV = isV; in->tf = tf; }
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(512) cloth_rollout_fwd_fast_kernel(ClothFwdArgs a) {
  extern __shared__ float4 lds4[];  // [2][Pp]
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
  const float k = a.k[b], mu = a.mu[b];
  const float iLs = 1.f / c.Ls, iLd = 1.f / c.Ld;
  GraspThr th0, th1;
  th0.init(ps[3]); th1.init(ps[7]);
  const size_t rec = cloth_rec_floats(Pp);
  float* ckb = a.ckpt ? a.ckpt + (size_t)b * cloth_env_records(T, S) * rec : nullptr;
  unsigned step = 0;
  for (int t = 0; t < T; ++t) {
    float act[8];
    macro_action_f(a.actions + ((size_t)t * B + b) * 8, act);
    for (int s = 0; s < S; ++s, ++step) {
      float4* X4 = lds4 + (step & 1u) * Pp;
      X4[i] = make_float4(x[0], x[1], x[2], 0.f);
      if (ckb) {
        float* r = ckb + (size_t)step * rec;
#pragma unroll
        for (int d = 0; d < 3; ++d) { r[d * Pp + i] = x[d]; r[(3 + d) * Pp + i] = v[d]; }
        if (i == 0) {
#pragma unroll
          for (int d = 0; d < 8; ++d) r[6 * Pp + d] = ps[d];
        }
      }
      __syncthreads();
      float vv[3], x2[3];
      bool m0, m1;
      FastInter dummy;
      force_fast<false>(c, nbs, X4, k, iLs, iLd, mu, x, v, vv, &dummy);
      grip_own(x, ps, act, th0.at(step == 0), th1.at(step == 0), m0, m1, x2);
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        vv[d] = m0 ? act[3] * vv[d] : vv[d];
        vv[d] = m1 ? act[7] * vv[d] : vv[d];
      }
      if (a.grasp && live) {
        uint8_t* g = a.grasp + ((((size_t)t * S + s) * B + b) * 2) * P;
        g[i] = m0; g[P + i] = m1;
      }
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int d = 0; d < 4; ++d) ps[g * 4 + d] = clipf(ps[g * 4 + d] + (d < 3 ? act[g * 4 + d] : 0.f), 0.f, 1.f);  // :322-323
#pragma unroll
      for (int d = 0; d < 3; ++d) {   // :326-329
        const float vc = clipf(vv[d], -c.max_v, c.max_v);
        x[d] = clipf(x2[d], 0.f, 1.f) + c.dt * vc;
        v[d] = vc;
      }
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
  if (live) {
    const size_t o = ((size_t)b * P + i) * 3;
#pragma unroll
    for (int d = 0; d < 3; ++d) { a.x_out[o + d] = x[d]; a.v_out[o + d] = v[d]; }
  }
  if (i == 0) {
#pragma unroll
    for (int d = 0; d < 8; ++d) a.prim_out[b * 8 + d] = ps[d];
  }
  if (ckb) {
    float* r = ckb + (size_t)T * S * rec;
#pragma unroll
    for (int d = 0; d < 3; ++d) { r[d * Pp + i] = x[d]; r[(3 + d) * Pp + i] = v[d]; }
    if (i == 0) {
#pragma unroll
      for (int d = 0; d < 8; ++d) r[6 * Pp + d] = ps[d];
    }
  }
}

void cloth_launch_fwd_fast(const ClothFwdArgs& a, hipStream_t stream) {
  const size_t shmem = (size_t)2 * a.c.Pp * sizeof(float4);
  hipLaunchKernelGGL(cloth_rollout_fwd_fast_kernel, dim3(a.B), dim3(a.c.Pp), shmem, stream, a);
}

}  // namespace ud
