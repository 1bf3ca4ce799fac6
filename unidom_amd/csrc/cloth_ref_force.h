// The mode-3 force block with in-range exact divide / sqrt sequences (design and operand windows: cloth_ref.hip's header), shared by the
// one-workgroup kernel (cloth_ref.hip, LDS planes of UD_REF_MAXP floats) and the several-workgroups-per-env kernel (cloth_cluster_ref.hip,
// planes of CL_STRIDE floats).  Every including file is compiled with -ffp-contract=off and correctly rounded f32 divide / sqrt.
#pragma once
#include "cloth_common.h"
#include "exact_math.h"

namespace ud {

// frexp exponents (0 for +-0) of the values seen so far.  inf and NaN also give exponent 0; inf shows in `amax` / `dmax`, NaN does NOT
// (fmaxf drops it): a lane whose operands hold a NaN stays on the fast path and returns NaN there
struct RefTrack {
  int rmin, rmax;     // link components
  int amin, amax_e;   // friction numerators
  float amax, dmax;   // |numerators| and |denominators| as floats: inf shows here
  __device__ __forceinline__ void init() { rmin = 0; rmax = 0; amin = 0; amax_e = 0; amax = 0.f; dmax = 0.f; }
  __device__ __forceinline__ void link(float r0, float r1, float r2) {
    const int e0 = __builtin_amdgcn_frexp_expf(r0), e1 = __builtin_amdgcn_frexp_expf(r1), e2 = __builtin_amdgcn_frexp_expf(r2);
    rmin = min(rmin, min(e0, min(e1, e2)));
    rmax = max(rmax, max(e0, max(e1, e2)));
    amax = fmaxf(amax, fmaxf(__builtin_fabsf(r0), fmaxf(__builtin_fabsf(r1), __builtin_fabsf(r2))));
  }
  __device__ __forceinline__ void num(float a) {
    const int e = __builtin_amdgcn_frexp_expf(a);
    amin = min(amin, e); amax_e = max(amax_e, e); amax = fmaxf(amax, __builtin_fabsf(a));
  }
  __device__ __forceinline__ void den(float d) { dmax = fmaxf(dmax, __builtin_fabsf(d)); }
  // link components: 0 or 2^-36 <= |r| < 2^8 (frexp exponent -35 .. 8); friction numerators: 0 or 2^-100 <= |a| < 2^100;
  // friction denominators sqrt(. + small_num): >= sqrt(small_num) >= 2^-24 by the per-launch check, here only < 2^24
  __device__ __forceinline__ bool bad() const {
    return rmin < -35 || rmax > 8 || amin < -99 || amax_e > 100 || !(amax < 0x1p100f) || !(dmax < 0x1p24f);
  }
};

// per-launch constants of the fast path
struct RefConst { float rLs, rLd; };   // div_prep(Ls), div_prep(Ld)

// One forward substep of a particle from own x, v and the neighbours' x in the LDS planes X (plane stride STRIDE floats; force, friction,
// damping: v -> v3); the grippers and the clip / advect are the caller's (they need no neighbour).  nbs[l] = the neighbour's index in
// the planes, or the particle's own where the lattice has none.  Same operations in the same order as substep_fwd (cloth_ref_order.h),
// each with the same correctly rounded result.  Returns false when a tracked operand left its window.
template <int STRIDE>
__device__ __forceinline__ bool force_ref(const ClothConst& c, const RefConst& rc, const int* nbs, const float* X, float k, float mu,
                                          const float* x, const float* v, float* v3) {
  RefTrack t;
  t.init();
  const float INF = INFINITY;
  float F[3] = {0.f, 0.f, 0.f};
  float r0[8], r1[8], r2[8], len[8], rl[8];
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const int j = nbs[l];
    r0[l] = X[j] - x[0]; r1[l] = X[STRIDE + j] - x[1]; r2[l] = X[2 * STRIDE + j] - x[2];
    t.link(r0[l], r1[l], r2[l]);
  }
#pragma unroll
  for (int l = 0; l < 8; ++l) {     // all eight roots and reciprocals before the first quotient: independent chains fill each other's latency
    const float s = r0[l] * r0[l] + r1[l] * r1[l] + r2[l] * r2[l];
    len[l] = sqrt_rn_inrange(clipf(s, 1e-12f, INF));
    rl[l] = div_prep(len[l]);
  }
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const float L = (l < 4) ? c.Ls : c.Ld, rL = (l < 4) ? rc.rLs : rc.rLd;
    const float dl = len[l] - L;
    // k * r / len * (len - L) / L, left to right (:267-268)
    const float f0 = div_rn_prepped_nz(div_rn_prepped_nz(k * r0[l], len[l], rl[l]) * dl, L, rL);
    const float f1 = div_rn_prepped_nz(div_rn_prepped_nz(k * r1[l], len[l], rl[l]) * dl, L, rL);
    const float f2 = div_rn_prepped_nz(div_rn_prepped_nz(k * r2[l], len[l], rl[l]) * dl, L, rL);
    F[0] += f0; F[1] += f1; F[2] += f2;
  }
  const float v1[3] = {v[0], v[1] - c.gdt, v[2]};     // :259
  F[1] += -c.g;                                       // :278
  const bool fm = x[1] <= c.eps;                      // :281
  const float cF = clipf(F[1], -INF, 0.f);
  const float muF = mu * cF * -1.0f;                  // :282
  const float xV = v1[0], yV = v1[2];
  const float sV = sqrt_rn_inrange(xV * xV + yV * yV + c.eps);
  const float dm = (fm && sV > c.eps) ? 1.f : 0.f;
  const float rsV = div_prep(sV);
  const float nx = dm * muF * xV, nz_ = dm * muF * yV;
  t.num(nx); t.num(nz_); t.den(sV);
  const float Ax = F[0] - div_rn_prepped_nz(nx, sV, rsV);
  const float Az = F[2] - div_rn_prepped_nz(nz_, sV, rsV);
  const bool st = fm && (sV <= c.eps);
  const float sF = sqrt_rn_inrange(Ax * Ax + Az * Az + c.eps);
  const float zm = (st && muF > sF) ? 1.f : 0.f;
  const float Bx = 0.f + (1.f - zm) * Ax, Bz = 0.f + (1.f - zm) * Az;
  const float nz = (st && muF <= sF) ? 1.f : 0.f;
  t.num(muF); t.den(sF);
  const float R = 1.f - div_rn_prepped_nz(muF, sF, div_prep(sF));
  const float Cx = (R * Ax) * nz + Bx * (1.f - nz);
  const float Cz = (R * Az) * nz + Bz * (1.f - nz);
  const float Ff[3] = {Cx, F[1], Cz};
#pragma unroll
  for (int a = 0; a < 3; ++a) v3[a] = (v1[a] + Ff[a] * c.dt) * c.damp;
  return !t.bad();
}

}  // namespace ud
