// The one-workgroup cloth adjoint of the fast path (see cloth_fast.hip for the restructuring: nine block sums, two barriers per
// substep).  It lives in a translation unit of its own because its roundings are part of its contract:
//
//   EVERY multiply-add of this file is written out.  The file is compiled with FMA contraction OFF (the pragma below and
//   -ffp-contract=off on the command line, which also covers the helpers of the headers), a fused multiply-add is a
//   __builtin_fmaf / fma2 call, and everything else is rounded operation by operation in the association the source gives.  So
//   the bits of every cotangent are the source's, whatever the vectoriser, the scheduler or a later compiler make of the code.
//
// The choices themselves are those the compiler made for the build this file was split from (contraction on, SLP vectoriser on),
// read off its ISA (tools/isa_dataflow.py) and pinned by tests/test_cloth_adjoint_bits_gpu.py: they look arbitrary in places
// (sm[3] and sm[5] unfused, sm[4] half fused, the nm sum of the norm chain fused differently from n2v) because they were.
#include <type_traits>
#include "cloth_fast_adj.h"

#pragma clang fp contract(off)

namespace ud {

// clip_grad_lt(x, 0, 1) from the sign of p = x (1 - x): two compares instead of four.  p > 0 exactly for 0 < x < 1 (1 - x >= 2^-24 there
// and the product of a positive float with it is positive, denormals kept); p = +-0 exactly on either bound (x = -0 included);
// p < 0 outside, -inf for +-inf, NaN for NaN: 1 / 0.5 / 0 as clip_grad_lt gives them.
__device__ __forceinline__ float clip_grad_01(float x) {
  const float p = x * (1.f - x);
  return p > 0.f ? 1.0f : (p == 0.f ? 0.5f : 0.0f);
}

__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
// a0 b0 + a1 b1 + a2 b2 as  fma(a2, b2, fma(a0, b0, a1 b1)):  the middle product is the one that is rounded
__device__ __forceinline__ float dot3_m(float a0, float a1, float a2, float b0, float b1, float b2) {
  return __builtin_fmaf(a2, b2, __builtin_fmaf(a0, b0, a1 * b1));
}

// force_pairs of cloth_fast_adj.h with its roundings written out (that one stays as it is for cloth_cluster_bwd.hip, whose file is
// compiled with contraction on)
template <int STRIDE>
__device__ __forceinline__ void force_pairs_x(const ClothConst& c, const int* nbs, const float* Xs, float k, f2 iL2, float mu,
                                              const float* x, const float* v, float* v3, PairInter* in) {
  f2 F0 = {0.f, 0.f}, F1 = {0.f, 0.f}, F2 = {0.f, 0.f};
  f2 q0[4], q1[4], q2[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {   // all 24 LDS reads in flight before the first use
    const int ja = nbs[p], jb = nbs[p + 4];
    q0[p] = f2{Xs[ja], Xs[jb]};
    q1[p] = f2{Xs[STRIDE + ja], Xs[STRIDE + jb]};
    q2[p] = f2{Xs[2 * STRIDE + ja], Xs[2 * STRIDE + jb]};
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const f2 r0 = q0[p] - x[0], r1 = q1[p] - x[1], r2 = q2[p] - x[2];
    const f2 s2 = fma2(r2, r2, fma2(r0, r0, r1 * r1));
    const f2 inv = {rsq(fmaxf(s2.x, 1e-12f)), rsq(fmaxf(s2.y, 1e-12f))};
    const f2 w = iL2 - inv;
    F0 = fma2(r0, w, F0); F1 = fma2(r1, w, F1); F2 = fma2(r2, w, F2);
    const f2 c3 = (k * inv) * (inv * inv);
    in->r0[p] = r0; in->r1[p] = r1; in->r2[p] = r2; in->w[p] = w;
    in->c2k[p] = f2{s2.x > 1e-12f ? c3.x : 0.f, s2.y > 1e-12f ? c3.y : 0.f};
  }
  const float S0 = F0.x + F0.y, S1 = F1.x + F1.y, S2 = F2.x + F2.y;
  const float Fy = k * S1 - c.g;                    // :278
  const float v1y = v[1] - c.gdt;                   // :259
  const bool fm = x[1] <= c.eps;                    // :281
  const float cF = fminf(Fy, 0.f);
  const float muF = mu * -cF;                       // :282
  const float xV = v[0], yV = v[2];
  const float isV = rsq((xV * xV + yV * yV) + c.eps); // :285
  const float tf = fm ? muF * isV : 0.f;            // :288-290 (sV > small_num always holds)
  const float Ax = __builtin_fmaf(S0, k, -(xV * tf)), Az = __builtin_fmaf(S2, k, -(yV * tf));   // k S - tf v: the force itself is never rounded
  v3[0] = __builtin_fmaf(Ax, c.dt, xV) * c.damp;    // :308-309
  v3[1] = __builtin_fmaf(Fy, c.dt, v1y) * c.damp;
  v3[2] = __builtin_fmaf(Az, c.dt, yV) * c.damp;
  in->S0 = S0; in->S1 = S1; in->S2 = S2;
  in->F1 = Fy; in->cF = cF; in->muF = muF; in->xV = xV; in->yV = yV; in->isV = isV; in->tf = tf;
}

constexpr int UD_CLOTH_MAXP = 1024 + 1;   // LDS plane stride (floats; the kernels refuse Pp > 1024).  Odd on purpose: a stride that is a
                                          // multiple of 64 lets the compiler fuse the x and y reads of one neighbour into ds_read2st64,
                                          // which then needs register moves to regroup them by link pair

// NORM = ClothBwdArgs::normalize as a compile-time switch: between barrier 1 and barrier 2 the substep is one basic block (no
// branch on `normalize`, and the primitive cotangent's pieces run in every wave -- it is zero outside lanes 0-7 of wave 0 and stays
// zero), so the scheduler can start the position reads of force_pairs_x under the norm chain.
// FULL = the body fills its waves (P == Pp, fold_cloth1's 512 particles): no padding lane, so `live` is a constant and its selects go.
// DEC = the substep's discrete decisions (grasp masks, the clip factors of x2, of v5 and of the primitives) come from the checkpoint's
// decision words (cloth_common.h; cloth_decisions_kernel below computes them with the functions the DEC = false code calls in its loop)
// and not from grip_own / clip_grad_01 / the compare with max_v: one word per lane-substep, fetched one substep ahead like nx / nv.
// Every operation on a cotangent is the same in both; a select against zero becomes an AND with an all-ones / zero mask (same bits).
__device__ __forceinline__ float and_mask(float x, int m) { return __builtin_bit_cast(float, __builtin_bit_cast(int, x) & m); }
// m ? x : y for an all-ones / zero mask (v_bfi_b32)
__device__ __forceinline__ float sel_mask(int m, float x, float y) {
  return __builtin_bit_cast(float, (__builtin_bit_cast(int, x) & m) | (__builtin_bit_cast(int, y) & ~m));
}

template <bool NORM, bool FULL, bool DEC>
__device__ __forceinline__ void cloth_rollout_bwd_fast(const ClothBwdArgs& a, float* ldsf) {
  // ldsf: Xs[3][MAXP] | Gs[3][MAXP] | red[2][16][UD_RSTR] | mac[16*8]
  const ClothConst c = a.c;
  const int i = threadIdx.x, b = blockIdx.x;
  const int P = c.P, Pp = c.Pp, S = c.S, B = a.B, T = a.T;
  const int nw = Pp >> 6, lane = i & 63, wv = i >> 6;
  const bool live = FULL || i < P;
  // single-buffered: every X read sits between barrier 1 and barrier 2 and the next X write comes after barrier 2;
  // every G read sits between barrier 2 and the next barrier 1 and the next G write comes after that barrier
  float* Xs = ldsf;
  float* Gs = ldsf + 3 * UD_CLOTH_MAXP;
  float* red = ldsf + 6 * UD_CLOTH_MAXP;
  float* mac = red + 2 * 16 * UD_RSTR;
  int nbs[8];
#pragma unroll
  for (int l = 0; l < 8; ++l) { const int j = a.nbr[l * Pp + i]; nbs[l] = j >= 0 ? j : i; }
  float gx[3] = {0.f, 0.f, 0.f}, gv[3] = {0.f, 0.f, 0.f};
  if (live) {
#pragma unroll
    for (int d = 0; d < 3; ++d) { gx[d] = a.g_x[((size_t)b * P + i) * 3 + d]; gv[d] = a.g_v[((size_t)b * P + i) * 3 + d]; }
  }
  // primitive cotangent: component d lives in lane d of wave 0 (lanes 0-3 gripper 0, 4-7 gripper 1)
  float gpl = (i < 8) ? a.g_prim[b * 8 + i] : 0.f;
  const bool pm3 = (i < 8) && ((i & 3) < 3);
  const float inm = 1.f / c.n_mask;
  const float k = a.k[b], mu = a.mu[b];
  const float Ls = c.Ls, Ld = c.Ld;
  const f2 iL2 = {1.f / Ls, 1.f / Ld};
  float gk = 0.f, gmu = 0.f;
  const size_t rec = cloth_rec_floats(Pp);
  const float* ck = a.ckpt + (size_t)b * cloth_env_records(T, S) * rec;
  GraspThr th0, th1;   // from record 0 = the rollout's input primitives, exactly what the forward derived them from
  if (!DEC) { th0.init(ck[6 * Pp + 3]); th1.init(ck[6 * Pp + 7]); }
  // records: `cur` = input of the substep being reversed, `vnext` = v of the record after it (= clip(v5))
  // The primitive rows of the records are read through the constant address space (scalar loads into SGPRs: the
  // checkpoints are read-only for this kernel), one substep ahead like the particle rows (`nps`, handed to `ps` after barrier 2).
  typedef const __attribute__((address_space(4))) float* cfptr;
  float vnext[3], nx[3], nv[3], ps[8], psl, nps[8], npsl;   // n* = the record the loop consumes next, fetched one substep ahead
  // DEC: this env's decision words [T*S][Pp]; `ndw` = the word of the substep the loop reverses next (vnext, ps, psl and their n* stay unused)
  const unsigned* const dw0 = (const unsigned*)(a.ckpt + (size_t)B * cloth_env_records(T, S) * rec) + (size_t)b * T * S * Pp;
  const unsigned* dp = dw0 + ((size_t)T * S - 1) * Pp;
  unsigned ndw = 0;
  {
    const float* r = ck + (size_t)T * S * rec;
    if (!DEC) {
#pragma unroll
      for (int d = 0; d < 3; ++d) vnext[d] = r[(3 + d) * Pp + i];
    }
    r = ck + ((size_t)T * S - 1) * rec;
#pragma unroll
    for (int d = 0; d < 3; ++d) { nx[d] = r[d * Pp + i]; nv[d] = r[(3 + d) * Pp + i]; }
    if (!DEC) {
#pragma unroll
      for (int d = 0; d < 8; ++d) ps[d] = ((cfptr)r)[6 * Pp + d];
      psl = r[6 * Pp + (i & 7)];
    } else {
      ndw = dp[i];
    }
  }
  for (int q = i; q < 2 * 16 * UD_RSTR; q += Pp) red[q] = 0.f;   // slots of waves this launch does not have are read as zeros
  __syncthreads();
  unsigned step = 0;
  const float* rp = ck + ((size_t)T * S - 1) * rec;   // record held in nx/nv/nps
  // Two waves per SIMD (WavePrio, cloth_common.h): the wave that loses the SIMD's arbitration enters both barrier intervals of the substep
  // at priority 1 and drops to 0 after force_pairs_x in the one, at the end of the spring adjoint in the other.  Either hand-over alone only moves the older
  // wave's wait to the other barrier (no gain); both together: -7 % of the kernel (profiles/r10_ablation.txt).
  WavePrio wp;
  wp.init(Pp);
  auto sweep = [&](auto lose) {
  constexpr bool LOSE = decltype(lose)::value;
  for (int t = T - 1; t >= 0; --t) {
    if (live) {
      const size_t o = (((size_t)t * B + b) * P + i) * 3;
      if (a.g_x_list) { gx[0] += a.g_x_list[o]; gx[1] += a.g_x_list[o + 1]; gx[2] += a.g_x_list[o + 2]; }
      if (a.g_v_list) { gv[0] += a.g_v_list[o]; gv[1] += a.g_v_list[o + 1]; gv[2] += a.g_v_list[o + 2]; }
    }
    if (a.g_prim_list && i < 8) gpl += a.g_prim_list[((size_t)t * B + b) * 8 + i];
    const float* a8 = a.actions + ((size_t)t * B + b) * 8;
    float act[8], ga[8];
    macro_action_f(a8, act);
#pragma unroll
    for (int d = 0; d < 8; ++d) ga[d] = 0.f;
    const float addl = pm3 ? clipf(a8[i & 7], -2.0f, 2.0f) * (1.0f / 50.0f) : 0.f;   // this lane's component of the primitive move
    const float oms1 = __builtin_fmaf(-act[7], act[7], 1.f);   // 1 - s1^2 of the gripper-1 norm
    float gaP = 0.f;
    for (int s = S - 1; s >= 0; --s, ++step) {
      float x[3], v[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) { x[d] = nx[d]; v[d] = nv[d]; }
      {  // prefetch the record this loop consumes next
        rp = (rp != ck) ? rp - rec : rp;            // uniform; the last iteration re-reads record 0 and ignores it
        const float* r = rp;
#pragma unroll
        for (int d = 0; d < 3; ++d) { nx[d] = r[(unsigned)(d * Pp + i)]; nv[d] = r[(unsigned)((3 + d) * Pp + i)]; }
        if (!DEC) {
#pragma unroll
          for (int d = 0; d < 8; ++d) nps[d] = ((cfptr)r)[6 * Pp + d];
          npsl = r[(unsigned)(6 * Pp + (i & 7))];
        }
      }
      const unsigned dw = ndw;
      if (DEC) {
        dp = (dp != dw0) ? dp - Pp : dp;
        ndw = dp[i];
      }
      const unsigned par = step & 1u;
      float* rd = red + par * 16 * UD_RSTR;
      Xs[i] = x[0]; Xs[UD_CLOTH_MAXP + i] = x[1]; Xs[2 * UD_CLOTH_MAXP + i] = x[2];
      // ---- own-particle forward pieces and the nine sums (no neighbour data needed) ----
      bool m0 = false, m1 = false;
      int M0 = 0, M1 = 0;   // DEC: the masks as all ones / zero (a padding lane's word is 0, so `live` is in them)
      float av[3], bv[3], bx[3];
      if (DEC) {
        M0 = (int)(dw << (31 - UD_DEC_M0)) >> 31;
        M1 = (int)(dw << (31 - UD_DEC_M1)) >> 31;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const float Dx = (float)((dw >> (8 * d)) & 0xFFu) * 0.5f;
          const float Dv = (float)((dw >> (UD_DEC_DV + d)) & 1u);
          av[d] = Dx * gx[d]; bv[d] = Dv * gv[d]; bx[d] = Dv * gx[d];
        }
      } else {
        float x2[3];
        grip_own(x, ps, act, th0.at(t == 0 && s == 0), th1.at(t == 0 && s == 0), m0, m1, x2);
        m0 = m0 && live; m1 = m1 && live;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const float Dx = clip_grad_01(x2[d]);
          const float Dv = (fabsf(vnext[d]) < c.max_v) ? 1.f : 0.f;
          av[d] = Dx * gx[d]; bv[d] = Dv * gv[d]; bx[d] = Dv * gx[d];
        }
      }
      float sm[UD_NSUM];
      sm[0] = dot3_m(gx[0], gx[1], gx[2], gx[0], gx[1], gx[2]);
      sm[1] = dot3_m(gv[0], gv[1], gv[2], gv[0], gv[1], gv[2]);
      sm[2] = dot3_m(av[0], av[1], av[2], av[0], av[1], av[2]);
      sm[3] = (bv[0] * bv[0] + bv[1] * bv[1]) + bv[2] * bv[2];                      // three rounded products
      sm[4] = __builtin_fmaf(bv[1], bx[1], bv[0] * bx[0]) + bv[2] * bx[2];
      sm[5] = (bx[0] * bx[0] + bx[1] * bx[1]) + bx[2] * bx[2];
      if (DEC) { sm[6] = and_mask(sm[3], M1); sm[7] = and_mask(sm[4], M1); sm[8] = and_mask(sm[5], M1); m1 = M1 != 0; }
      else { sm[6] = m1 ? sm[3] : 0.f; sm[7] = m1 ? sm[4] : 0.f; sm[8] = m1 ? sm[5] : 0.f; }
      if (NORM) {
        const float sm8[8] = {sm[0], sm[1], sm[2], sm[3], sm[4], sm[5], sm[6], sm[7]};
        const float w8 = wave_sum8_t(sm8, lane);
        if ((lane & 0x2C) == 0) rd[wv * UD_RSTR + (((lane >> 2) & 4) | (lane & 3))] = w8;
        if (__builtin_amdgcn_ballot_w64(m1) != 0) {   // wave-uniform: gripper 1 holds something in this wave
          const float w = wave_sum_l63(sm[8]);
          if (lane == 63) rd[wv * UD_RSTR + 8] = w;
        } else if (lane == 63) {
          rd[wv * UD_RSTR + 8] = 0.f;
        }
      }
      if (LOSE) wp.up();
      __syncthreads();   // barrier 1: X4 and the wave partials are visible
      float sx = 1.f, sv = 1.f, sA = 1.f, sB = 1.f, s3x = 1.f, s3v = 1.f;   // cumulative scale factors
      if (NORM) {
        // row g of the wave adds the partials of waves g, g+4, g+8, g+12 (slots of absent waves stay zero), then the
        // four rows are added position by position: one LDS round trip instead of a dependent read per wave
        float tot = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) tot += rd[((lane >> 4) + 4 * m) * UD_RSTR + (lane & 15)];
        tot = rows_sum4(tot);
        float T_[UD_NSUM];
#pragma unroll
        for (int q = 0; q < UD_NSUM; ++q) T_[q] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, tot), q));
        sx = inv_norm(T_[0], inm);                                   // :331
        sv = inv_norm(T_[1], inm);                                   // :332
        const float cx = c.dt * sx;
        const float svv = sv * sv, svx = (sv + sv) * cx, cxx = cx * cx;
        const float n2x = (sx * sx) * T_[2];                              // |g_x2|^2
        const float n2v = __builtin_fmaf(cxx, T_[5], __builtin_fmaf(svx, T_[4], svv * T_[3]));
        sA = inv_norm(n2x, inm);                                     // :223 (gripper 1)
        sB = inv_norm(n2v, inm);                                     // :224
        const float n3x = n2x * (sA * sA);
        const float nm = __builtin_fmaf(svx, T_[7], svv * T_[6]) + cxx * T_[8];
        const float n3v = (n2v - nm * oms1) * (sB * sB);
        s3x = inv_norm(n3x, inm);                                    // :223 (gripper 0)
        s3v = inv_norm(fmaxf(n3v, 0.f), inm);                        // :224
        // primitives (:333-334): 4-vector norms, uniform; only lanes 0-7 of wave 0 carry a primitive cotangent, the rest compute on zeros
        float n2 = __builtin_fmaf(gpl, gpl, dpp_f<0xB1>(gpl * gpl));   // the neighbour's product is rounded, the lane's own is not
        n2 += dpp_f<0x4E>(n2);   // quad total = this gripper's 4-vector norm^2
        gpl *= inv_norm(n2, inm);
      }
      // ---- neighbour-dependent forward recompute ----
      float v3[3], v4[3];
      PairInter in;
      force_pairs_x<UD_CLOTH_MAXP>(c, nbs, Xs, k, iL2, mu, x, v, v3, &in);
      if (LOSE) wp.drop();
#pragma unroll
      for (int d = 0; d < 3; ++d) v4[d] = v3[d] * (DEC ? sel_mask(M0, act[3], 1.f) : (m0 ? act[3] : 1.f));   // the suction as a factor (sc0 of the gripper-0 block below): x * 1 = x bit for bit
      // ---- reverse: clip (:326-329) and the two grippers (:313-314) with their normalisations folded in ----
      float gx2n[3], gv5n[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        gx2n[d] = (av[d] * sx) * sA;
        gv5n[d] = __builtin_fmaf(bv[d], sv, (c.dt * sx) * bx[d]) * sB;
      }
      {  // gripper 1, branch-free: masks as 0/1 factors
        const float s1 = act[7], m1f = DEC ? and_mask(1.f, M1) : (m1 ? 1.f : 0.f), sc1 = DEC ? sel_mask(M1, s1, 1.f) : (m1 ? s1 : 1.f), h1 = (1.f - s1) * m1f;
        const float dotv = __builtin_fmaf(gv5n[2], v4[2], __builtin_fmaf(gv5n[1], v4[1], gv5n[0] * v4[0]));
        const float dotx = __builtin_fmaf(act[6], gx2n[2], __builtin_fmaf(act[4], gx2n[0], act[5] * gx2n[1]));
        ga[7] = __builtin_fmaf(dotv - dotx, m1f, ga[7]);
#pragma unroll
        for (int d = 0; d < 3; ++d) { ga[4 + d] = __builtin_fmaf(h1, gx2n[d], ga[4 + d]); gv5n[d] *= sc1; }
      }
      float gxd[3], gv3[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) { gxd[d] = gx2n[d] * s3x; gv3[d] = gv5n[d] * s3v; }
      {  // gripper 0
        const float s0 = act[3], m0f = DEC ? and_mask(1.f, M0) : (m0 ? 1.f : 0.f), sc0 = DEC ? sel_mask(M0, s0, 1.f) : (m0 ? s0 : 1.f), h0 = (1.f - s0) * m0f;
        const float dotv = dot3_m(v3[0], v3[1], v3[2], gv3[0], gv3[1], gv3[2]);
        const float dotx = dot3_m(act[0], act[1], act[2], gxd[0], gxd[1], gxd[2]);
        ga[3] = __builtin_fmaf(dotv - dotx, m0f, ga[3]);
#pragma unroll
        for (int d = 0; d < 3; ++d) { ga[d] = __builtin_fmaf(h0, gxd[d], ga[d]); gv3[d] *= sc0; }
      }
      // primitives (:322-323), uniform; counted once (lane 0) in the action accumulators
      gpl *= DEC ? (float)((dw >> UD_DEC_PRIM) & 3u) * 0.5f : clip_grad_01(psl + addl);
      gaP += pm3 ? gpl : 0.f;
      // ---- v3 = (v1 + F dt) damp ; ground friction (:281-290) ----
      float gF[3];
      {
        const float g2x = gv3[0] * c.damp, g2y = gv3[1] * c.damp, g2z = gv3[2] * c.damp;
        const float gAx = g2x * c.dt, gFy = g2y * c.dt, gAz = g2z * c.dt;
        // the cotangent of tf enters with its sign flipped (ngt = -gt, and -0 where the particle is off the ground), which
        // saves the negations: g_muF = -ngmuF, g_isV = -ngisV
        const float ngt = in.xV * gAx + in.yV * gAz;
        const bool fm = x[1] <= c.eps;
        const float ngmuF = fm ? ngt * in.isV : -0.f;
        const float ngisV = fm ? ngt * in.muF : -0.f;
        const float gq = (((0.5f * in.isV) * in.isV) * in.isV) * ngisV;
        const float gxV = __builtin_fmaf(in.xV + in.xV, gq, -(gAx * in.tf)), gyV = __builtin_fmaf(in.yV + in.yV, gq, -(gAz * in.tf));
        gmu += live ? in.cF * ngmuF : 0.f;
        const float gcF = mu * ngmuF;
        const float cfm = (in.F1 < 0.f) ? 1.f : ((in.F1 == 0.f) ? 0.5f : 0.f);
        gF[0] = live ? gAx : 0.f;
        gF[1] = live ? gFy + gcF * cfm : 0.f;
        gF[2] = live ? gAz : 0.f;
        gv[0] = g2x + gxV; gv[1] = g2y; gv[2] = g2z + gyV;   // v1 = v - (0, g dt, 0)
      }
      Gs[i] = gF[0]; Gs[UD_CLOTH_MAXP + i] = gF[1]; Gs[2 * UD_CLOTH_MAXP + i] = gF[2];
      if (LOSE) wp.up();
      __syncthreads();   // barrier 2: Gs visible
      if (!DEC) {
#pragma unroll
        for (int d = 0; d < 8; ++d) ps[d] = nps[d];   // next substep's primitives
        psl = npsl;
      }
      // ---- spring adjoint, gather form: g_x_i = gxd + sum_l J_il (gF_j - gF_i) ----
      f2 A0 = {gxd[0], 0.f}, A1 = {gxd[1], 0.f}, A2 = {gxd[2], 0.f};
      f2 h0[4], h1[4], h2[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {   // all 24 LDS reads in flight before the first use
        const int ja = nbs[p], jb = nbs[p + 4];       // a missing neighbour reads gF itself: d = 0 and r = 0
        h0[p] = f2{Gs[ja], Gs[jb]};
        h1[p] = f2{Gs[UD_CLOTH_MAXP + ja], Gs[UD_CLOTH_MAXP + jb]};
        h2[p] = f2{Gs[2 * UD_CLOTH_MAXP + ja], Gs[2 * UD_CLOTH_MAXP + jb]};
      }
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const f2 d0 = h0[p] - gF[0], d1 = h1[p] - gF[1], d2 = h2[p] - gF[2];
        const f2 r0 = in.r0[p], r1 = in.r1[p], r2 = in.r2[p];
        const f2 rd_ = fma2(d2, r2, fma2(d0, r0, d1 * r1));
        const f2 c1 = k * in.w[p];
        const f2 c2 = in.c2k[p] * rd_;
        A0 += fma2(d0, c1, r0 * c2); A1 += fma2(d1, c1, r1 * c2); A2 += fma2(d2, c1, r2 * c2);
      }
      const float ax0 = A0.x + A0.y, ax1 = A1.x + A1.y, ax2 = A2.x + A2.y;
      gk += __builtin_fmaf(in.S2, gF[2], __builtin_fmaf(in.S0, gF[0], in.S1 * gF[1]));   // sum_l w_l (r_l . gF) = gF . S
      gx[0] = ax0; gx[1] = ax1; gx[2] = ax2;
      if (!DEC) {
#pragma unroll
        for (int d = 0; d < 3; ++d) vnext[d] = v[d];   // this substep's input v is the previous substep's clip(v5)
      }
      if (LOSE) wp.drop();
    }
    // macro-step boundary: robot_step's action transform (:168-169)
    {
      __syncthreads();
      {
        const float w8 = wave_sum8_t(ga, lane);
        if ((lane & 0x2C) == 0) mac[wv * 8 + (((lane >> 2) & 4) | (lane & 3))] = w8;
      }
      __syncthreads();
      if (i < 8) {
        float tot = 0.f;
        for (int q = 0; q < nw; ++q) tot += mac[q * 8 + i];
        tot += gaP;
        const int d = i & 3;
        a.g_actions[((size_t)t * B + b) * 8 + i] = (d < 3) ? tot * (1.0f / 50.0f) * clip_grad(a8[i], -2.0f, 2.0f) : tot;
      }
    }
  }
  };
  // two copies of the sweep, chosen per wave: every wave passes the same barriers in either
  if (wp.lose) sweep(std::true_type()); else sweep(std::false_type());
  if (live) {
    const size_t o = ((size_t)b * P + i) * 3;
#pragma unroll
    for (int d = 0; d < 3; ++d) { a.g_x0[o + d] = gx[d]; a.g_v0[o + d] = gv[d]; }
  }
  __syncthreads();
  {
    const float w0 = wave_sum_l63(gk), w1 = wave_sum_l63(gmu);
    if (lane == 63) { mac[wv * 2] = w0; mac[wv * 2 + 1] = w1; }
  }
  __syncthreads();
  if (i < 8) a.g_prim0[b * 8 + i] = gpl;
  if (i == 0) {
    float t0 = 0.f, t1 = 0.f;
    for (int q = 0; q < nw; ++q) { t0 += mac[q * 2]; t1 += mac[q * 2 + 1]; }
    a.g_k[b] = t0;
    a.g_mu[b] = t1;
  }
}

// One kernel per variant under a plain name (profiles and counter passes are keyed by kernel name).  The training default -- normalised
// cotangents, a body that fills its waves -- keeps the name it always had; `_ragged` = a body with padding lanes in its last wave.
__global__ void __launch_bounds__(512) cloth_rollout_bwd_fast_ragged_kernel(ClothBwdArgs a) {
  extern __shared__ float ldsf[];
  cloth_rollout_bwd_fast<true, false, false>(a, ldsf);
}

__global__ void __launch_bounds__(512) cloth_rollout_bwd_fast_ragged_raw_kernel(ClothBwdArgs a) {
  extern __shared__ float ldsf[];
  cloth_rollout_bwd_fast<false, false, false>(a, ldsf);
}

__global__ void __launch_bounds__(512) cloth_rollout_bwd_fast_kernel(ClothBwdArgs a) {
  extern __shared__ float ldsf[];
  cloth_rollout_bwd_fast<true, true, false>(a, ldsf);
}

__global__ void __launch_bounds__(512) cloth_rollout_bwd_fast_raw_kernel(ClothBwdArgs a) {
  extern __shared__ float ldsf[];
  cloth_rollout_bwd_fast<false, true, false>(a, ldsf);
}

// the same four with the decisions read from the checkpoint's words (DEC)
__global__ void __launch_bounds__(512) cloth_rollout_bwd_dec_ragged_kernel(ClothBwdArgs a) {
  extern __shared__ float ldsf[];
  cloth_rollout_bwd_fast<true, false, true>(a, ldsf);
}

__global__ void __launch_bounds__(512) cloth_rollout_bwd_dec_ragged_raw_kernel(ClothBwdArgs a) {
  extern __shared__ float ldsf[];
  cloth_rollout_bwd_fast<false, false, true>(a, ldsf);
}

__global__ void __launch_bounds__(512) cloth_rollout_bwd_dec_kernel(ClothBwdArgs a) {
  extern __shared__ float ldsf[];
  cloth_rollout_bwd_fast<true, true, true>(a, ldsf);
}

__global__ void __launch_bounds__(512) cloth_rollout_bwd_dec_raw_kernel(ClothBwdArgs a) {
  extern __shared__ float ldsf[];
  cloth_rollout_bwd_fast<false, true, true>(a, ldsf);
}

void cloth_launch_bwd_fast(const ClothBwdArgs& a, hipStream_t stream) {
  const size_t shmem = (size_t)(6 * UD_CLOTH_MAXP + 2 * 16 * UD_RSTR + 16 * 8) * sizeof(float);
  auto* kern = a.c.P == a.c.Pp ? (a.normalize ? cloth_rollout_bwd_fast_kernel : cloth_rollout_bwd_fast_raw_kernel)
                               : (a.normalize ? cloth_rollout_bwd_fast_ragged_kernel : cloth_rollout_bwd_fast_ragged_raw_kernel);
  if (a.dec)
    kern = a.c.P == a.c.Pp ? (a.normalize ? cloth_rollout_bwd_dec_kernel : cloth_rollout_bwd_dec_raw_kernel)
                           : (a.normalize ? cloth_rollout_bwd_dec_ragged_kernel : cloth_rollout_bwd_dec_ragged_raw_kernel);
  hipLaunchKernelGGL(kern, dim3(a.B), dim3(a.c.Pp), shmem, stream, a);
}

// The pre-pass: the decision words of all T*S substeps of all envs at once, on the whole chip, from the records the forward has just
// written.  It calls what the DEC = false sweep calls per substep -- macro_action_f, GraspThr from record 0 (the first-substep threshold
// for record 0), grip_own, clip_grad_01, the compare of record n + 1's v with max_v, and in lanes 0-7 clip_grad_01 of the moved primitive
// component -- in this translation unit (contraction off), so the booleans are that sweep's by construction.
// One workgroup of Pp lanes per (env, UD_DEC_RECS consecutive records): the two thresholds (a walk over IEEE square roots) are derived once
// per workgroup, not once per word.
constexpr int UD_DEC_RECS = 8;
__global__ void __launch_bounds__(512) cloth_decisions_kernel(ClothConst c, int B, int T, float* ckpt, const float* actions) {
  const int i = threadIdx.x, b = blockIdx.y;
  const int P = c.P, Pp = c.Pp, S = c.S, TS = T * S;
  const size_t rec = cloth_rec_floats(Pp);
  const float* ck = ckpt + (size_t)b * cloth_env_records(T, S) * rec;
  unsigned* words = (unsigned*)(ckpt + (size_t)B * cloth_env_records(T, S) * rec) + (size_t)b * TS * Pp;
  GraspThr th0, th1;
  th0.init(ck[6 * Pp + 3]); th1.init(ck[6 * Pp + 7]);
  const bool live = i < P;
  const bool pm3 = (i < 8) && ((i & 3) < 3);
  const int n0 = blockIdx.x * UD_DEC_RECS, n1 = min(n0 + UD_DEC_RECS, TS);
  for (int n = n0; n < n1; ++n) {
    const float* r = ck + (size_t)n * rec;
    const float* a8 = actions + ((size_t)(n / S) * B + b) * 8;
    float act[8], x[3], ps[8], x2[3];
    macro_action_f(a8, act);
#pragma unroll
    for (int d = 0; d < 3; ++d) x[d] = r[d * Pp + i];
#pragma unroll
    for (int d = 0; d < 8; ++d) ps[d] = r[6 * Pp + d];
    bool m0, m1;
    grip_own(x, ps, act, th0.at(n == 0), th1.at(n == 0), m0, m1, x2);
    unsigned w = 0;
    if (live) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        w |= (unsigned)(2.f * clip_grad_01(x2[d])) << (8 * d);
        w |= (fabsf(r[rec + (3 + d) * Pp + i]) < c.max_v ? 1u : 0u) << (UD_DEC_DV + d);
      }
      w |= (m0 ? 1u : 0u) << UD_DEC_M0 | (m1 ? 1u : 0u) << UD_DEC_M1;
    }
    if (i < 8) {
      const float addl = pm3 ? clipf(a8[i & 7], -2.0f, 2.0f) * (1.0f / 50.0f) : 0.f;
      w |= (unsigned)(2.f * clip_grad_01(r[6 * Pp + (i & 7)] + addl)) << UD_DEC_PRIM;
    }
    words[(size_t)n * Pp + i] = w;
  }
}

void cloth_launch_decisions(const ClothConst& c, int B, int T, float* ckpt, const float* actions, hipStream_t stream) {
  hipLaunchKernelGGL(cloth_decisions_kernel, dim3((T * c.S + UD_DEC_RECS - 1) / UD_DEC_RECS, B), dim3(c.Pp), 0, stream, c, B, T, ckpt, actions);
}

}  // namespace ud
