// Mode-3 cloth forward for bodies of more than 1024 particles on several workgroups per env: the reference's LITERAL operation
// order (cloth_simulator.py:257-337 as written), bit-identical to the CPU restatement of that order (oracle cloth_substep_fwd,
// ClothOracle(order=1)) whatever the number of parts.
//   skeleton    cloth_cluster_fwd.hip unchanged: the same parts, LDS window, position hand-off through the step-parity XE buffer,
//               checkpoint records, halo poll and dead path (protocol: cloth_cluster.h).  The hand-off moves positions only, so
//               it does not depend on the operation order.
//   per particle  cloth_ref.hip's kernel: force_ref (cloth_ref_force.h) on the in-range exact divide / sqrt sequences, every
//               operand tracked; a wave in which any live lane left a window (or whose env's k, or whose launch's constants, are
//               outside the checks) repeats the substep for its 64 particles with the literal substep_fwd (cloth_ref_order.h).
//               That branch is wave-uniform, not workgroup-uniform, so it holds no barrier; every neighbour it reads is already in
//               the LDS window.
// Padding lanes (gi >= P: the ragged last part) never send their wave to the literal code; no output and no live particle uses them.
#include <cmath>

#include "cloth_cluster.h"
#include "cloth_ref_force.h"
#include "cloth_ref_order.h"
#include "cloth_v2_force.h"

namespace ud {

__global__ void __launch_bounds__(CL_T) cloth_cluster_fwd_ref_kernel(ClothFwdArgs a, ClusterArgs q, int fast) {
  extern __shared__ float ldsf[];  // Xs[2][3][CL_STRIDE], double-buffered by substep parity | bail[2]
  int bl, w;
  cl_decode(q.W, bl, w);
  if (bl >= q.Bl) return;
  const int b = q.b0 + bl;
  const ClothConst c = a.c;
  const int P = c.P, Pp = c.Pp, S = c.S, B = a.B, T = a.T;
  const int i = threadIdx.x, base = w * CL_T, gi = base + i;
  const bool inp = gi < Pp, live = gi < P;
  const int lo = max(0, base - q.H), hi = min(Pp, base + CL_T + q.H);   // LDS window = particles [lo, hi)
  const int nlo = base - lo, nhi = max(0, hi - (base + CL_T));            // halo entries below / above the part
  const int li = gi - lo;
  const bool hl = i < nlo + nhi;                                          // this lane fetches one halo particle
  const int hidx = i < nlo ? lo + i : base + CL_T + (i - nlo);
  int* bail = (int*)(ldsf + 6 * CL_STRIDE);
  if (i < 2) bail[i] = 0;
  // window indices; a missing neighbour is the particle itself (force_ref: r = 0, adds -0).  The literal fallback wants -1 there
  // instead -- a particle is never its own neighbour, so it derives that table from this one where it needs it.
  int nbs[8];
  float L0[8];
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const int j = inp ? a.nbr[l * Pp + gi] : -1;
    nbs[l] = (j >= 0 ? j : gi) - lo;
    L0[l] = (l < 4) ? c.Ls : c.Ld;
  }
  float x[3] = {0.f, 0.f, 0.f}, v[3] = {0.f, 0.f, 0.f};
  if (live) {
#pragma unroll
    for (int d = 0; d < 3; ++d) { x[d] = a.x[((size_t)b * P + gi) * 3 + d]; v[d] = a.v[((size_t)b * P + gi) * 3 + d]; }
  }
  float ps[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) ps[d] = a.prim[b * 8 + d];
  const float k = a.k[b], mu = a.mu[b];
  const RefConst rc = {div_prep(c.Ls), div_prep(c.Ld)};
  // fast: the launch's constants passed cloth_ref_consts_ok; k_ok: this env's stiffness is inside the window (cloth_ref.hip).  Either
  // false -> every wave of the env runs the literal code
  const bool k_ok = fast && __builtin_fabsf(k) >= 0x1p-8f && __builtin_fabsf(k) < 0x1p24f;
  GraspThr th0, th1;
  th0.init(ps[3]); th1.init(ps[7]);
  const size_t rec = cloth_rec_floats(Pp);
  float* ckb = a.ckpt ? a.ckpt + (size_t)b * cloth_env_records(T, S) * rec : nullptr;
  cl_granule* ar = q.arena + (size_t)bl * cl_env_granules(Pp, q.W);   // XE[2][3][Pp] first
  __syncthreads();
  unsigned step = 0;
  bool dead = false;
  for (int t = 0; t < T && !dead; ++t) {
    float act[8];
    macro_action_f(a.actions + ((size_t)t * B + b) * 8, act);
    for (int s = 0; s < S; ++s, ++step) {
      const unsigned tag = step + 1u;
      float* Xs = ldsf + (step & 1u) * (3 * CL_STRIDE);
      Xs[li] = x[0]; Xs[CL_STRIDE + li] = x[1]; Xs[2 * CL_STRIDE + li] = x[2];
      // XE is double-buffered by step parity (cloth_cluster_fwd.hip)
      cl_granule* xe = ar + (size_t)(step & 1u) * 3 * Pp;
      if (inp) { cl_put(xe + gi, x[0], tag); cl_put(xe + Pp + gi, x[1], tag); cl_put(xe + 2 * (size_t)Pp + gi, x[2], tag); }
      if (ckb && inp) {
        float* r = ckb + (size_t)step * rec;
#pragma unroll
        for (int d = 0; d < 3; ++d) { r[d * Pp + gi] = x[d]; r[(3 + d) * Pp + gi] = v[d]; }
        if (gi == 0) {
#pragma unroll
          for (int d = 0; d < 8; ++d) r[6 * Pp + d] = ps[d];
        }
      }
      // no neighbour needed: grasp tests, displaced position, primitive update (out of place: a wave that falls back tests its
      // grippers against this substep's primitives) -- while the halo travels
      float vv[3] = {0.f, 0.f, 0.f}, x2[3];
      bool m0, m1;
      grip_own(x, ps, act, th0.at(step == 0), th1.at(step == 0), m0, m1, x2);
      float po[8];
      prim_update(ps, act, po);
      if (__builtin_amdgcn_ballot_w64(hl) != 0) {   // waves that hold halo lanes (the first (nlo + nhi) / 64 of the part)
        float h[3];
        const bool ok = cl_poll3(xe + hidx, (size_t)Pp, tag, hl, h);
        if (hl) { Xs[hidx - lo] = h[0]; Xs[CL_STRIDE + hidx - lo] = h[1]; Xs[2 * CL_STRIDE + hidx - lo] = h[2]; }
        if (!ok) bail[step & 1u] = 1;
      }
      __syncthreads();
      if (bail[step & 1u]) { dead = true; break; }
      const bool ok = (k_ok && force_ref<CL_STRIDE>(c, rc, nbs, Xs, k, mu, x, v, vv)) || !live;
      if (__builtin_amdgcn_ballot_w64(!ok) != 0) {
        // a live lane of this wave left an operand window (or the env / launch is outside its checks): the literal substep, grippers
        // and clip included, for the whole wave -- its outputs replace what the fast path computed
        int nbw[8];
#pragma unroll
        for (int l = 0; l < 8; ++l) nbw[l] = nbs[l] == li ? -1 : nbs[l];
        float xo[3], vo[3];
        Inter in;
        substep_fwd<false>(c, li, nbw, L0, Xs, k, mu, x, v, ps, act, xo, vo, &in, CL_STRIDE);
        if (a.grasp && live) {
          uint8_t* g = a.grasp + ((((size_t)t * S + s) * B + b) * 2) * P;
          g[gi] = in.m0; g[P + gi] = in.m1;
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
          g[gi] = m0; g[P + gi] = m1;
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
    if (dead) break;
    if (live) {
      const size_t o = (((size_t)t * B + b) * P + gi) * 3;
      if (a.x_list) { a.x_list[o] = x[0]; a.x_list[o + 1] = x[1]; a.x_list[o + 2] = x[2]; }
      if (a.v_list) { a.v_list[o] = v[0]; a.v_list[o + 1] = v[1]; a.v_list[o + 2] = v[2]; }
    }
    if (a.prim_list && gi == 0) {
#pragma unroll
      for (int d = 0; d < 8; ++d) a.prim_list[((size_t)t * B + b) * 8 + d] = ps[d];
    }
  }
  if (dead) {   // a part of this env never showed up: make it loud
    if (i == 0 && q.timeouts) atomicAdd(q.timeouts, 1);
#pragma unroll
    for (int d = 0; d < 3; ++d) { x[d] = NAN; v[d] = NAN; }
#pragma unroll
    for (int d = 0; d < 8; ++d) ps[d] = NAN;
  }
  if (live) {
    const size_t o = ((size_t)b * P + gi) * 3;
#pragma unroll
    for (int d = 0; d < 3; ++d) { a.x_out[o + d] = x[d]; a.v_out[o + d] = v[d]; }
  }
  if (gi == 0) {
#pragma unroll
    for (int d = 0; d < 8; ++d) a.prim_out[b * 8 + d] = ps[d];
  }
  if (ckb && inp) {
    float* r = ckb + (size_t)T * S * rec;
#pragma unroll
    for (int d = 0; d < 3; ++d) { r[d * Pp + gi] = x[d]; r[(3 + d) * Pp + gi] = v[d]; }
    if (gi == 0) {
#pragma unroll
      for (int d = 0; d < 8; ++d) r[6 * Pp + d] = ps[d];
    }
  }
}

void cloth_launch_fwd_cluster_ref(const ClothFwdArgs& a, const ClusterArgs& q, int fast, hipStream_t stream) {
  const size_t shmem = (size_t)(6 * CL_STRIDE + 2) * sizeof(float);
  hipLaunchKernelGGL(cloth_cluster_fwd_ref_kernel, dim3(cl_grid(q.Bl, q.W)), dim3(CL_T), shmem, stream, a, q, fast);
}

}  // namespace ud
