// Mode-3 cloth forward for gfx950: the reference's LITERAL operation order (cloth_simulator.py:257-337 as written -- spring force
// k * r / len * (len - L0) / L0 per component, the whole friction block :281-306, gravity twice) with the SAME bits as
// cloth_ref_order.h::substep_fwd and the CPU restatement of that order (oracle/csrc/cloth_oracle.hpp::cloth_substep_fwd), at about
// two thirds of the instructions.
//
// What the literal kernel spends its time on is 51 IEEE divisions and 12 IEEE square roots per particle-substep: hipcc expands each
// division into v_div_scale x2, v_rcp, five FMAs, v_div_fmas, v_div_fixup (11 instructions) and each sqrt into ~15.  Here
//   * a division is exact_math.h's div_rn_prepped_nz: the compiler's own sequence minus its exponent scaling and fix-up (5 instructions),
//     with the refined reciprocal shared by the numerators of one denominator -- the three components of a link share 1 / len, and
//     1 / L0 is one of two per-launch constants (straight / diagonal rest length);
//   * a sqrt is sqrt_rn_inrange (v_sqrt + two residual FMAs + two selects);
//   * the two grasp tests compare squared distances with the exact thresholds of cloth_common.h (same booleans as the sqrt form);
//   * a missing neighbour points at the particle itself: r = 0 exactly, the force component is -0 and adding it changes no bit
//     (F starts at +0 and can never become -0), so the per-link selects go.
// Those sequences return the correctly rounded result only inside operand windows (tools/check_exact_math.hip,
// tools/check_exact_div.hip: |a| in [2^-100, 2^100), |d| in [2^-24, 2^24), sqrt arguments >= 2^-96).  The windows are not assumed:
// every lane tracks the frexp exponents of its 24 link components (0, or 2^-36 <= |r| < 2^8 -- with the per-launch checks on k, L0 and
// small_num that puts every numerator and denominator of the spring block inside) and of the three friction numerators, and a wave
// in which ANY lane left a window repeats the substep for its 64 particles with the literal code (wave-uniform branch; a lane's
// result depends on its own arithmetic only).  A launch whose constants are outside the per-launch checks runs the literal kernel.
// So: bit-identical to the literal order for any NaN-free input, fast for every input a cloth produces (positions in [0, 1],
// |v| <= max_v).  A NaN operand is not caught by the tracking (cloth_ref_force.h): its lane stays on the fast path and returns NaN.
// The tracking and the force block live in cloth_ref_force.h, shared with the several-workgroup kernel (cloth_cluster_ref.hip).
#include <cmath>

#include "cloth_ref_force.h"
#include "cloth_ref_order.h"
#include "cloth_v2_force.h"

namespace ud {

constexpr int UD_REF_MAXP = 512;   // LDS plane stride (floats); this kernel serves Pp <= 512

__global__ void __launch_bounds__(512) cloth_rollout_fwd_ref_kernel(ClothFwdArgs a) {
  extern __shared__ float ldsf[];  // Xs[2][3][UD_REF_MAXP], double-buffered by substep parity
  const ClothConst c = a.c;
  const int i = threadIdx.x, b = blockIdx.x;
  const int P = c.P, Pp = c.Pp, S = c.S, B = a.B, T = a.T;
  const bool live = i < P;
  int nbs[8], nb[8];
  float L0[8];
#pragma unroll
  for (int l = 0; l < 8; ++l) { nb[l] = a.nbr[l * Pp + i]; nbs[l] = nb[l] >= 0 ? nb[l] : i; L0[l] = (l < 4) ? c.Ls : c.Ld; }
  float x[3] = {0.f, 0.f, 0.f}, v[3] = {0.f, 0.f, 0.f};
  if (live) {
#pragma unroll
    for (int d = 0; d < 3; ++d) { x[d] = a.x[((size_t)b * P + i) * 3 + d]; v[d] = a.v[((size_t)b * P + i) * 3 + d]; }
  }
  float ps[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) ps[d] = a.prim[b * 8 + d];
  const float k = a.k[b], mu = a.mu[b];
  const RefConst rc = {div_prep(c.Ls), div_prep(c.Ld)};
  // per-env constants of the fast path: 2^-8 <= |k| < 2^24 puts k r, k r / len and (k r / len)(len - L) inside the division's windows for
  // every tracked r (cloth_ref.hip header); otherwise this env runs the literal code throughout (block-uniform)
  const bool k_ok = __builtin_fabsf(k) >= 0x1p-8f && __builtin_fabsf(k) < 0x1p24f;
  GraspThr th0, th1;
  th0.init(ps[3]); th1.init(ps[7]);
  const size_t rec = cloth_rec_floats(Pp);
  float* ckb = a.ckpt ? a.ckpt + (size_t)b * cloth_env_records(T, S) * rec : nullptr;
  unsigned step = 0;
  for (int t = 0; t < T; ++t) {
    float act[8];
    macro_action_f(a.actions + ((size_t)t * B + b) * 8, act);
    for (int s = 0; s < S; ++s, ++step) {
      float* Xs = ldsf + (step & 1u) * (3 * UD_REF_MAXP);
      Xs[i] = x[0]; Xs[UD_REF_MAXP + i] = x[1]; Xs[2 * UD_REF_MAXP + i] = x[2];
      if (ckb) {
        float* r = ckb + (size_t)step * rec;
#pragma unroll
        for (int d = 0; d < 3; ++d) { r[d * Pp + i] = x[d]; r[(3 + d) * Pp + i] = v[d]; }
        if (i == 0) {
#pragma unroll
          for (int d = 0; d < 8; ++d) r[6 * Pp + d] = ps[d];
        }
      }
      // no neighbour needed: grasp tests, displaced position, primitive update -- between the LDS write and the barrier
      float vv[3], x2[3];
      bool m0, m1;
      grip_own(x, ps, act, th0.at(step == 0), th1.at(step == 0), m0, m1, x2);
      float po[8];
      prim_update(ps, act, po);
      __syncthreads();
      bool ok = k_ok && force_ref<UD_REF_MAXP>(c, rc, nbs, Xs, k, mu, x, v, vv);
      if (__builtin_amdgcn_ballot_w64(!ok) != 0) {
        // a lane of this wave left an operand window (or the env's k is outside its check): the literal substep, grippers and clip
        // included, for the whole wave -- its outputs replace what the fast path computed
        float xo[3], vo[3];
        Inter in;
        substep_fwd<false>(c, i, nb, L0, Xs, k, mu, x, v, ps, act, xo, vo, &in, UD_REF_MAXP);
        if (a.grasp && live) {
          uint8_t* g = a.grasp + ((((size_t)t * S + s) * B + b) * 2) * P;
          g[i] = in.m0; g[P + i] = in.m1;
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) { x[d] = xo[d]; v[d] = vo[d]; }
      } else {
#pragma unroll
        for (int d = 0; d < 3; ++d) {           // grippers 0 then 1 (:313-314): v <- suction * v where grasped
          vv[d] = m0 ? act[3] * vv[d] : vv[d];
          vv[d] = m1 ? act[7] * vv[d] : vv[d];
        }
        if (a.grasp && live) {
          uint8_t* g = a.grasp + ((((size_t)t * S + s) * B + b) * 2) * P;
          g[i] = m0; g[P + i] = m1;
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {           // :326-329
          const float vc = clipf(vv[d], -c.max_v, c.max_v);
          x[d] = clipf(x2[d], 0.f, 1.f) + c.dt * vc;
          v[d] = vc;
        }
      }
#pragma unroll
      for (int d = 0; d < 8; ++d) ps[d] = po[d];
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

// The per-launch constants the fast path relies on (header): rest lengths in [2^-20, 2^4], small_num >= 2^-48 (so that
// sqrt(. + small_num) >= 2^-24), dt / damp / gravity finite.  Shared with the several-workgroup kernel (cloth_cluster_ref.hip), which
// runs every wave on the literal code when they fail.
bool cloth_ref_consts_ok(const ClothConst& c) {
  auto in = [](float v, float lo, float hi) { return v >= lo && v <= hi; };
  return in(c.Ls, 0x1p-20f, 0x1p4f) && in(c.Ld, 0x1p-20f, 0x1p4f) && in(c.eps, 0x1p-48f, 0x1p20f) &&
         std::isfinite(c.dt) && std::isfinite(c.damp) && std::isfinite(c.g) && std::isfinite(c.gdt) && std::isfinite(c.max_v);
}

// This kernel's launch condition: the constants above and a body that fits its LDS planes.  false -> the caller launches the literal kernel.
bool cloth_ref_fast_ok(const ClothConst& c) { return c.Pp <= UD_REF_MAXP && cloth_ref_consts_ok(c); }

void cloth_launch_fwd_ref(const ClothFwdArgs& a, hipStream_t stream) {
  const size_t shmem = (size_t)2 * 3 * UD_REF_MAXP * sizeof(float);
  hipLaunchKernelGGL(cloth_rollout_fwd_ref_kernel, dim3(a.B), dim3(a.c.Pp), shmem, stream, a);
}

}  // namespace ud
