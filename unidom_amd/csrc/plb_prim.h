// Primitive contact of the PlasticineLab-style f64 MLS-MPM grid op beyond the sticky Sphere: the base class's model
// (GenORM/policy/pbm/plb/engine/primitive/primive_base.py:57-115 -- signed distance in the primitive's frame, rotated analytic
// normal, soft influence, Coulomb friction) for the Capsule (primitives.py:55-73), one cell against one primitive, and its
// hand-derived adjoint.  f64, plain C++; the orientation is a handle constant (action.dim = 3: w = 0, rotation[f + 1] = rotation[f]).
// Differentiable in the primitive's positions P_f (through the local point: distance, normal, influence, collider velocity) and
// P_{f+1} (collider velocity) and in the incoming cell velocity; the branches (active, flag) are held constant, the sub-gradients
// of min / max / clamp at equality are torch's (the checker is torch.autograd through tests/plb_prim_twin.py).
#pragma once
#include <hip/hip_runtime.h>

namespace ud {

// per-primitive constants of a handle with a general primitive; kind 0 = sticky Sphere, 1 = Capsule
struct PlbPrim {
  int kind[2];
  double h[2], mu[2];
  double q[2][4];    // rotation (w, x, y, z) as given: qrot(q, .) takes the primitive's frame to the world
  double qi[2][4];   // conj(q) / |q|: inv_trans (utils.py:43-47)
};
// What the kernels of a handle take beside PlbArgs: nothing on a Sphere-only handle (the kernels it runs are the GEN = false
// instantiations, which hold no general code at all), the constants above otherwise.  Chosen at create.
template <bool GEN> struct PlbPrimArg {};
template <> struct PlbPrimArg<true> { PlbPrim p; };

__device__ __forceinline__ void plb_cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
// utils.py:7-13: v + 2 (w (qv x v) + qv x (qv x v)); linear in v, and for any rot (unit or not) its transpose is the same map with conj(rot)
__device__ __forceinline__ void plb_qrot(const double* rot, const double* v, double* o) {
  double uv[3], uuv[3];
  plb_cross(rot + 1, v, uv);
  plb_cross(rot + 1, uv, uuv);
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = v[k] + 2 * (rot[0] * uv[k] + uuv[k]);
}
__device__ __forceinline__ void plb_qrot_t(const double* rot, const double* g, double* o) {
  const double cj[4] = {rot[0], -rot[1], -rot[2], -rot[3]};
  plb_qrot(cj, g, o);
}

// Capsule._sdf / _normal (primitives.py:61-73) behind inv_trans: d = point - position.  pl = the point in the primitive's frame, p = the vector
// from the nearest point of the axis segment, len = sqrt(p.p + 1e-14) (primitives.py's length); the distance is len - r, the local normal p / len.
// pass_y: 1 where p.y moves with pl.y (beyond the segment's ends), 0 alongside it.
__device__ __forceinline__ double plb_capsule_local(const PlbPrim& pr, int pi, const double* d, double* pl, double* p, double& pass_y) {
  plb_qrot(pr.qi[pi], d, pl);
  const double py = pl[1] + pr.h[pi] / 2;
  p[0] = pl[0]; p[2] = pl[2];
  p[1] = py - fmin(fmax(py, 0.0), pr.h[pi]);
  pass_y = (py >= 0.0 && py <= pr.h[pi]) ? 0.0 : 1.0;
  return sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + 1e-14);
}
// cotangents (glen of len, gnl of the local normal p / len, gpl of pl directly) -> cotangent of d
__device__ __forceinline__ void plb_capsule_local_adj(const PlbPrim& pr, int pi, const double* p, double len, double pass_y, double glen, const double* gnl,
                                                      const double* gpl, double* gd) {
  const double il = 1.0 / len;
  const double gl = glen - (gnl[0] * p[0] + gnl[1] * p[1] + gnl[2] * p[2]) * il * il;
  double g[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] = gnl[k] * il + gl * p[k] * il;
  g[1] *= pass_y;
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] += gpl[k];
  plb_qrot_t(pr.qi[pi], g, gd);
}

// everything Primitive.collide (primive_base.py:91-115) computes for one cell, kept for the adjoint
struct PlbCollide {
  bool active, flag;
  double pl[3], p[3], pass_y, len, dist, D[3], e, infl, cv[3], w[3], nc, mn, t[3], tn, arg, ts[3];
};
// gp: cell position, P0 / P1: the primitive's position at substeps f / f + 1, sf: softness, u: the cell velocity so far
__device__ __forceinline__ void plb_collide_eval(const PlbPrim& pr, int pi, double radius, double dt, const double* gp, const double* P0, const double* P1,
                                                 double sf, const double* u, PlbCollide& k) {
  const double d[3] = {gp[0] - P0[0], gp[1] - P0[1], gp[2] - P0[2]};
  k.len = plb_capsule_local(pr, pi, d, k.pl, k.p, k.pass_y);
  k.dist = k.len - radius;
  k.e = exp(-k.dist * sf);
  k.infl = fmin(k.e, 1.0);
  k.active = (sf > 0 && k.infl > 0.1) || k.dist <= 0;       // no 0.001 and no trailing `and softness > 0`: those are the Sphere override's
  k.flag = false;
  if (!k.active) return;
  const double nl[3] = {k.p[0] / k.len, k.p[1] / k.len, k.p[2] / k.len};
  plb_qrot(pr.q[pi], nl, k.D);
  double back[3];
  plb_qrot(pr.q[pi], k.pl, back);                            // rotation[f + 1] = rotation[f]
#pragma unroll
  for (int i = 0; i < 3; ++i) { k.cv[i] = (back[i] + P1[i] - gp[i]) / dt; k.w[i] = u[i] - k.cv[i]; }
  k.nc = k.w[0] * k.D[0] + k.w[1] * k.D[1] + k.w[2] * k.D[2];
  k.mn = fmin(k.nc, 0.0);
#pragma unroll
  for (int i = 0; i < 3; ++i) k.t[i] = k.w[i] - k.mn * k.D[i];
  const double tt = k.t[0] * k.t[0] + k.t[1] * k.t[1] + k.t[2] * k.t[2];
  k.tn = sqrt(tt + 1e-8);                                    // utils.py's length
  k.arg = k.tn + k.nc * pr.mu[pi];
  k.flag = k.nc < 0 && sqrt(tt) > 1e-30;
  const double s = fmax(0.0, k.arg);
#pragma unroll
  for (int i = 0; i < 3; ++i) k.ts[i] = k.flag ? k.t[i] / k.tn * s : k.t[i];
}
// u <- collide(u); returns whether the primitive acted on the cell
__device__ __forceinline__ bool plb_collide(const PlbPrim& pr, int pi, double radius, double dt, const double* gp, const double* P0, const double* P1, double sf,
                                            double* u) {
  PlbCollide k;
  plb_collide_eval(pr, pi, radius, dt, gp, P0, P1, sf, u, k);
  if (!k.active) return false;
#pragma unroll
  for (int i = 0; i < 3; ++i) u[i] = k.cv[i] + k.w[i] * (1 - k.infl) + k.ts[i] * k.infl;
  return true;
}
// adjoint of an ACTIVE collide: G = cotangent of u_out (in), cotangent of u_in (out, may alias nothing of the inputs); g0 / g1 = cotangents of P_f / P_{f+1}
__device__ __forceinline__ void plb_collide_adj(const PlbPrim& pr, int pi, double dt, const PlbCollide& k, double sf, const double* G, double* gu, double* g0,
                                                double* g1) {
  double gcv[3], gw[3], gt[3], gD[3];
  double ginfl = 0, gnc = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    gcv[i] = G[i]; gw[i] = G[i] * (1 - k.infl); gt[i] = G[i] * k.infl;
    ginfl += G[i] * (k.ts[i] - k.w[i]);
  }
  if (k.flag) {                                              // ts = t * (s / tn), s = max(0, tn + nc mu)
    const double s = fmax(0.0, k.arg), ratio = s / k.tn;
    const double gr = gt[0] * k.t[0] + gt[1] * k.t[1] + gt[2] * k.t[2];
    double gtn = -gr * s / (k.tn * k.tn);
    if (k.arg >= 0) { gtn += gr / k.tn; gnc += gr / k.tn * pr.mu[pi]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) gt[i] = gt[i] * ratio + gtn * k.t[i] / k.tn;
  }
  // t = w - min(nc, 0) D
  const double gmn = -(gt[0] * k.D[0] + gt[1] * k.D[1] + gt[2] * k.D[2]);
  if (k.nc <= 0) gnc += gmn;
#pragma unroll
  for (int i = 0; i < 3; ++i) { gw[i] += gt[i]; gD[i] = -k.mn * gt[i]; }
  // nc = w . D
#pragma unroll
  for (int i = 0; i < 3; ++i) { gw[i] += gnc * k.D[i]; gD[i] += gnc * k.w[i]; }
  // w = u - cv
#pragma unroll
  for (int i = 0; i < 3; ++i) { gu[i] = gw[i]; gcv[i] -= gw[i]; }
  // influence = min(exp(-dist softness), 1)
  const double glen = (k.e <= 1.0) ? -sf * k.e * ginfl : 0.0;
  // cv = (qrot(q, pl) + P1 - g) / dt, D = qrot(q, p / len)
  double gback[3], gpl[3], gnl[3], gd[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { gback[i] = gcv[i] / dt; g1[i] = gback[i]; }
  plb_qrot_t(pr.q[pi], gback, gpl);
  plb_qrot_t(pr.q[pi], gD, gnl);
  plb_capsule_local_adj(pr, pi, k.p, k.len, k.pass_y, glen, gnl, gpl, gd);
#pragma unroll
  for (int i = 0; i < 3; ++i) g0[i] = -gd[i];                // d = g - P_f
}

}  // namespace ud
