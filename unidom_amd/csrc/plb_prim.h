// Primitive contact of the PlasticineLab-style f64 MLS-MPM grid op beyond the sticky Sphere: the base class's model
// (GenORM/policy/pbm/plb/engine/primitive/primive_base.py:57-115 -- signed distance in the primitive's frame, rotated analytic
// normal, soft influence, Coulomb friction) for the Capsule (primitives.py:55-73), one cell against one primitive, and its
// hand-derived adjoint.  f64, plain C++.  The orientation is a handle constant (action.dim = 3: w = 0, rotation[f + 1] = rotation[f]) or, on a
// rot_state handle, per-env state: every function below is a template on ROT -- false (the default) reads the handle's constants pr.q / pr.qi exactly
// as before, true takes q_f, conj(q_f) / |q_f| and q_{f+1} as pointers (one geometry, two instantiations) and its adjoint also returns the cotangents
// of q_f and q_{f+1}.
// Differentiable in the primitive's positions P_f (through the local point: distance, normal, influence, collider velocity) and
// P_{f+1} (collider velocity) and in the incoming cell velocity; the branches (active, flag) are held constant, the sub-gradients
// of min / max / clamp at equality are torch's (the checker is torch.autograd through tests/plb_prim_twin.py).
#pragma once
#include <hip/hip_runtime.h>

namespace ud {

// per-primitive constants of a handle with a general primitive; kind 0 = sticky Sphere, 1 = Capsule (the RollingPin's contact is the Capsule's: kind 1 here)
struct PlbPrim {
  int kind[2];
  double h[2], mu[2];
  double q[2][4];    // rotation (w, x, y, z) as given: qrot(q, .) takes the primitive's frame to the world
  double qi[2][4];   // conj(q) / |q|: inv_trans (utils.py:43-47)
};
// What the kernels of a handle take beside PlbArgs: nothing on a Sphere-only handle (the kernels it runs are the GEN = 0
// instantiations, which hold no general code at all), the constants above otherwise.  Chosen at create.
// On a rot_state handle (GEN = 2) also the rotation trajectory of this step and its cotangent, and the kinematics of primitive 0.
struct PlbRot {
  double* rot;      // [B][S+1][np][4] (w, x, y, z): handle arena, or the caller's checkpoint; the loss kernels: the caller's prim_rot [B][np][4]
  double* grot;     // [B][S+1][np][4] cotangent (adjoint only); the loss adjoint: the caller's g_prim_rot [B][np][4] (may be null)
  double* ext;      // the caller's [B][np][4] array of this launch: prim_rot (pack), prim_rot_out (unpack), g_prim_rot (adjoint pack; may be null)
  int kin;          // kinematics of primitive 0: 1 = Primitive.forward_kinematics, 2 = RollingPin's, 3 = Chopsticks' (plb_gap_step, plb_qstep_right below)
  int adim;         // action dimensions: 3 or 6 (7 on a Chopsticks handle)
  double sw[3];     // action.scale[3:6]
};
template <int GEN> struct PlbPrimArg {};
template <> struct PlbPrimArg<1> { PlbPrim p; };
template <> struct PlbPrimArg<2> { PlbPrim p; PlbRot r; };
// Shape constants of a handle with a Box, a Cylinder or a Torus (PlbPrim.kind 3 / 4 / 5): Box size (three half extents), Cylinder (h, r, -),
// Torus (tx, ty, -).  Such a handle runs instantiations of its own (GEN = 3: constant orientation, 4: rot_state), whose general code goes
// through the shape layer below with the primitive's kind read at run time (a Capsule may sit beside a new shape); PlbPrim is laid out as
// before, so the kernels of every other handle take the arguments they always took.
struct PlbShape { double c[2][3]; };
template <> struct PlbPrimArg<3> { PlbPrim p; PlbShape s; };
template <> struct PlbPrimArg<4> { PlbPrim p; PlbRot r; PlbShape s; };
// A handle with a Chopsticks (PlbPrim.kind 6, primitive 0 only, always on rot_state; GEN = 5): the one kind whose shape is state.  Its opening
// `gap` changes once per substep, so the trajectory of this step and its cotangent sit beside the rotation's.  The shape layer takes the gap
// of the substep where the other kinds take their constants: a pointer to it stands in for PlbShape.c[pi] (plb_shape_consts).
struct PlbGap {
  double* gap;      // [B][S+1][np]: handle arena, or the caller's checkpoint; the loss kernels: the caller's prim_gap [B][np]
  double* ggap;     // [B][S+1][np] cotangent (adjoint only); the loss adjoint: the caller's g_prim_gap [B][np] (may be null)
  double* ext;      // the caller's [B][np] array of this launch: prim_gap (pack), g_prim_gap (adjoint pack; may be null)
  double* ext_out;  // the forward pack: prim_gap_out [B][np]
  double mingap[2]; // minimal_gap
  double sg;        // action.scale[6]
};
template <> struct PlbPrimArg<5> { PlbPrim p; PlbRot r; PlbShape s; PlbGap g; };
// which kinds take Primitive.collide: the Capsule alone in the instantiations of before, every kind but the sticky Sphere on a shape handle.
// SH is 0 (no shape layer), 1 (Box, Cylinder, Torus, Capsule) or 2 (a Chopsticks handle: kind 6 as well; gap = the env's gaps [np] of the substep)
template <int SH> __device__ __forceinline__ bool plb_general(int kind) {
  if constexpr (SH != 0) return kind != 0; else return kind == 1;
}
// the constants the shape layer reads for primitive pi: the handle's, or for a Chopsticks its gap of this substep
template <int SH> __device__ __forceinline__ const double* plb_shape_consts(const PlbPrim& pr, const PlbShape& sh, int pi, const double* gap) {
  if constexpr (SH == 2) { if (pr.kind[pi] == 6) return gap + pi; }
  return sh.c[pi];
}
// the extra argument of the pack / unpack kernels: nothing, or the above
template <bool ROT> struct PlbRotArg {};
template <> struct PlbRotArg<true> { PlbRot r; };

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

// adjoint of plb_qrot in its rotation argument: g = cotangent of qrot(rot, v) -> grot (w, x, y, z), assigned
__device__ __forceinline__ void plb_qrot_adj_rot(const double* rot, const double* v, const double* g, double* grot) {
  double a[3], vg[3], ag[3], gu[3], vgu[3];
  plb_cross(rot + 1, v, a);
  plb_cross(v, g, vg);
  plb_cross(a, g, ag);
  plb_cross(g, rot + 1, gu);
  plb_cross(v, gu, vgu);
  grot[0] = 2 * (g[0] * a[0] + g[1] * a[1] + g[2] * a[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) grot[1 + k] = 2 * (rot[0] * vg[k] + ag[k] + vgu[k]);
}
// utils.py:19-27: the Hamilton product q r, normalised
__device__ __forceinline__ void plb_qmul(const double* q, const double* r, double* o) {
  const double w = r[0] * q[0] - r[1] * q[1] - r[2] * q[2] - r[3] * q[3];
  const double x = r[0] * q[1] + r[1] * q[0] - r[2] * q[3] + r[3] * q[2];
  const double y = r[0] * q[2] + r[1] * q[3] + r[2] * q[0] - r[3] * q[1];
  const double z = r[0] * q[3] - r[1] * q[2] + r[2] * q[1] + r[3] * q[0];
  const double n = sqrt(w * w + x * x + y * y + z * z);
  o[0] = w / n; o[1] = x / n; o[2] = y / n; o[3] = z / n;
}
// its adjoint: o = plb_qmul(q, r) again, go its cotangent; gq / gr are ADDED to
__device__ __forceinline__ void plb_qmul_adj(const double* q, const double* r, const double* go, double* gq, double* gr) {
  const double w = r[0] * q[0] - r[1] * q[1] - r[2] * q[2] - r[3] * q[3];
  const double x = r[0] * q[1] + r[1] * q[0] - r[2] * q[3] + r[3] * q[2];
  const double y = r[0] * q[2] + r[1] * q[3] + r[2] * q[0] - r[3] * q[1];
  const double z = r[0] * q[3] - r[1] * q[2] + r[2] * q[1] + r[3] * q[0];
  const double n = sqrt(w * w + x * x + y * y + z * z);
  const double o[4] = {w / n, x / n, y / n, z / n};
  const double dot = go[0] * o[0] + go[1] * o[1] + go[2] * o[2] + go[3] * o[3];
  const double gw = (go[0] - dot * o[0]) / n, gx = (go[1] - dot * o[1]) / n, gy = (go[2] - dot * o[2]) / n, gz = (go[3] - dot * o[3]) / n;
  gq[0] += gw * r[0] + gx * r[1] + gy * r[2] + gz * r[3];
  gq[1] += -gw * r[1] + gx * r[0] - gy * r[3] + gz * r[2];
  gq[2] += -gw * r[2] + gx * r[3] + gy * r[0] - gz * r[1];
  gq[3] += -gw * r[3] - gx * r[2] + gy * r[1] + gz * r[0];
  gr[0] += gw * q[0] + gx * q[1] + gy * q[2] + gz * q[3];
  gr[1] += -gw * q[1] + gx * q[0] + gy * q[3] - gz * q[2];
  gr[2] += -gw * q[2] - gx * q[3] + gy * q[0] + gz * q[1];
  gr[3] += -gw * q[3] + gx * q[2] - gy * q[1] + gz * q[0];
}
// utils.py:29-41: axis-angle -> quaternion; the identity when |w| <= 1e-9
__device__ __forceinline__ void plb_w2quat(const double* w, double* o) {
  const double n = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  o[0] = 1.0; o[1] = 0.0; o[2] = 0.0; o[3] = 0.0;
  if (n > 1e-9) {
    const double s = sin(n / 2);
    o[0] = cos(n / 2); o[1] = w[0] / n * s; o[2] = w[1] / n * s; o[3] = w[2] / n * s;
  }
}
// its adjoint, assigned; on the identity arm the cotangent of w is DEFINED as 0 (taichi's reverse mode would form 0 * inf there)
__device__ __forceinline__ void plb_w2quat_adj(const double* w, const double* go, double* gw) {
  const double n = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  gw[0] = 0.0; gw[1] = 0.0; gw[2] = 0.0;
  if (n > 1e-9) {
    const double s = sin(n / 2), c = cos(n / 2);
    const double gs = (go[1] * w[0] + go[2] * w[1] + go[3] * w[2]) / n;      // v = (w / n) s
    const double gn = gs * c / 2 - go[0] * s / 2 - (go[1] * w[0] + go[2] * w[1] + go[3] * w[2]) * s / (n * n);
#pragma unroll
    for (int k = 0; k < 3; ++k) gw[k] = go[1 + k] * s / n + gn * w[k] / n;
  }
}
// conj(q) / |q| (inv_trans, utils.py:43-47) and its adjoint (gq ADDED to)
__device__ __forceinline__ void plb_qinv(const double* q, double* qi) {
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  qi[0] = q[0] / n; qi[1] = -q[1] / n; qi[2] = -q[2] / n; qi[3] = -q[3] / n;
}
__device__ __forceinline__ void plb_qinv_adj(const double* q, const double* qi, const double* gqi, double* gq) {
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double dot = gqi[0] * qi[0] + gqi[1] * qi[1] + gqi[2] * qi[2] + gqi[3] * qi[3];
  gq[0] += (gqi[0] - dot * qi[0]) / n;
#pragma unroll
  for (int k = 1; k < 4; ++k) gq[k] -= (gqi[k] - dot * qi[k]) / n;
}
// Chopsticks.forward_kinematics (primitives.py:113-117) beside the base class's: the rotation step multiplies on the RIGHT, rot[f+1] =
// qmul(rot[f], w2quat(w)) (a turn about the body's own axes; the base class has w2quat(w) on the left), and the opening closes against a floor,
// gap[f+1] = max(gap[f] - gap_vel, minimal_gap).  Adjoints: gq / gdq / ggap / ggv are ADDED to; the arm of max is held constant -- the cotangent
// passes where gap - gap_vel > minimal_gap and is zero where it is smaller; at exact equality it is unspecified (here: zero).
__device__ __forceinline__ void plb_qstep_right(const double* q, const double* dq, double* q1) { plb_qmul(q, dq, q1); }
__device__ __forceinline__ void plb_qstep_right_adj(const double* q, const double* dq, const double* gq1, double* gq, double* gdq) { plb_qmul_adj(q, dq, gq1, gq, gdq); }
__device__ __forceinline__ double plb_gap_step(double gap, double gv, double mingap) { return fmax(gap - gv, mingap); }
__device__ __forceinline__ void plb_gap_step_adj(double gap, double gv, double mingap, double g1, double& ggap, double& ggv) {
  if (gap - gv > mingap) { ggap += g1; ggv -= g1; }
}

// the orientation a ROT = false instantiation reads (the handle's constant) or a ROT = true one is given
template <bool ROT> __device__ __forceinline__ const double* plb_sel(const double* of_handle, const double* given) {
  if constexpr (ROT) return given; else return of_handle;
}

// Capsule._sdf / _normal (primitives.py:61-73) behind inv_trans: d = point - position.  pl = the point in the primitive's frame, p = the vector
// from the nearest point of the axis segment, len = sqrt(p.p + 1e-14) (primitives.py's length); the distance is len - r, the local normal p / len.
// pass_y: 1 where p.y moves with pl.y (beyond the segment's ends), 0 alongside it.
template <bool ROT = false>   // qi: conj(q_f) / |q_f| (ROT)
__device__ __forceinline__ double plb_capsule_local(const PlbPrim& pr, int pi, const double* d, double* pl, double* p, double& pass_y, const double* qi = nullptr) {
  plb_qrot(plb_sel<ROT>(pr.qi[pi], qi), d, pl);
  const double py = pl[1] + pr.h[pi] / 2;
  p[0] = pl[0]; p[2] = pl[2];
  p[1] = py - fmin(fmax(py, 0.0), pr.h[pi]);
  pass_y = (py >= 0.0 && py <= pr.h[pi]) ? 0.0 : 1.0;
  return sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + 1e-14);
}
// cotangents (glen of len, gnl of the local normal p / len, gpl of pl directly) -> cotangent of d; ROT: also gpl_all, the whole cotangent of pl
template <bool ROT = false>
__device__ __forceinline__ void plb_capsule_local_adj(const PlbPrim& pr, int pi, const double* p, double len, double pass_y, double glen, const double* gnl,
                                                      const double* gpl, double* gd, const double* qi = nullptr, double* gpl_all = nullptr) {
  const double il = 1.0 / len;
  const double gl = glen - (gnl[0] * p[0] + gnl[1] * p[1] + gnl[2] * p[2]) * il * il;
  double g[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] = gnl[k] * il + gl * p[k] * il;
  g[1] *= pass_y;
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] += gpl[k];
  plb_qrot_t(plb_sel<ROT>(pr.qi[pi], qi), g, gd);
  if constexpr (ROT) { gpl_all[0] = g[0]; gpl_all[1] = g[1]; gpl_all[2] = g[2]; }
}

// ---- shape layer: (kind, constants, pl = the point in the primitive's frame) -> signed distance and local normal, and the adjoint from their
// cotangents to pl's.  Restated from primitives.py: Capsule :61-73, Cylinder :176-202, Torus :211-231, Box :241-269; length(x) = sqrt(x.x + 1e-14)
// throughout (:8-14).  Constants of the adjoint: indicators, signs and the arm abs / min / max took.  The Box normal is the reference's central
// difference of its own _sdf (d = 1e-4), and its adjoint the exact derivative of that formula: the analytic sdf gradient at the six samples.
#define PLB_BOX_D 1e-4
__device__ __forceinline__ double plb_sgn(double a) { return a > 0.0 ? 1.0 : (a < 0.0 ? -1.0 : 0.0); }
// Box._sdf (:251-256) at y; grad (may be null): its gradient
__device__ __forceinline__ double plb_box_sdf(const double* sz, const double* y, double* grad = nullptr) {
  const double q[3] = {fabs(y[0]) - sz[0], fabs(y[1]) - sz[1], fabs(y[2]) - sz[2]};
  const double m[3] = {fmax(q[0], 0.0), fmax(q[1], 0.0), fmax(q[2], 0.0)};
  const double len = sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2] + 1e-14);
  const double mx = fmax(q[0], fmax(q[1], q[2]));
  if (grad) {
    const int am = (q[0] >= q[1] && q[0] >= q[2]) ? 0 : (q[1] >= q[2] ? 1 : 2);
#pragma unroll
    for (int i = 0; i < 3; ++i) grad[i] = plb_sgn(y[i]) * (m[i] / len + ((mx <= 0.0 && am == i) ? 1.0 : 0.0));
  }
  return len + fmin(mx, 0.0);
}
// Chopsticks._sdf / _normal (primitives.py:130-147): two Capsules of the primitive's (h, r) side by side.  With p = pl + (0, h/2, 0) and delta =
// (gap/2, 0, 0) stick a is the Capsule's _sdf at p - delta, stick b at p + delta, and that _sdf shifts y by h/2 AGAIN before it takes off
// clamp(y, 0, h): both axis segments span local y in [-h, 0], at x = -+gap/2 -- the primitive's position is the sticks' top end, as the reference
// has it.  sdf = min(a, b); the normal is stick a's where a <= b (a tie takes a for both), else stick b's.  Both sticks are evaluated here, once,
// for the distance, the normal and the adjoint: p = the selected stick's vector from its axis segment (the sticks differ in p[0] alone), len =
// length(p), pass_y as in plb_capsule_local, half = d p[0] / d gap (-1/2 for stick a, +1/2 for stick b).  The selection is a constant of the adjoint.
__device__ __forceinline__ double plb_chop_pick(double gap, double ch, const double* pl, double* p, double& pass_y, double& half) {
  const double py = (pl[1] + ch / 2) + ch / 2;
  p[1] = py - fmin(fmax(py, 0.0), ch); p[2] = pl[2];
  pass_y = (py >= 0.0 && py <= ch) ? 0.0 : 1.0;
  const double xa = pl[0] - gap / 2, xb = pl[0] + gap / 2;
  const double rest = p[1] * p[1] + p[2] * p[2] + 1e-14;
  const double la = sqrt(xa * xa + rest), lb = sqrt(xb * xb + rest);
  const bool a = la <= lb;                                   // a - r <= b - r
  p[0] = a ? xa : xb; half = a ? -0.5 : 0.5;
  return a ? la : lb;
}
// the distance alone (all a cell outside the shell, and the contact loss, need)
template <int SH = 1>
__device__ __forceinline__ double plb_shape_sdf(int kind, const double* sc, double ch, double radius, const double* pl) {
  if constexpr (SH == 2) {
    if (kind == 6) {                                         // Chopsticks: sc[0] = the gap of this substep (plb_shape_consts)
      double p[3], pass_y, half;
      return plb_chop_pick(sc[0], ch, pl, p, pass_y, half) - radius;
    }
  }
  if (kind == 3) return plb_box_sdf(sc, pl);
  if (kind == 4) {                                           // Cylinder: sc = (h, r), h the radial half extent and r the axial one
    const double l = sqrt(pl[0] * pl[0] + pl[2] * pl[2] + 1e-14);
    const double d0 = l - sc[0], d1 = fabs(pl[1]) - sc[1];
    const double m0 = fmax(d0, 0.0), m1 = fmax(d1, 0.0);
    return fmin(fmax(d0, d1), 0.0) + sqrt(m0 * m0 + m1 * m1 + 1e-14);
  }
  if (kind == 5) {                                           // Torus: sc = (tx, ty)
    const double q0 = sqrt(pl[0] * pl[0] + pl[2] * pl[2] + 1e-14) - sc[0];
    return sqrt(q0 * q0 + pl[1] * pl[1] + 1e-14) - sc[1];
  }
  const double py = pl[1] + ch / 2;                          // Capsule, as plb_capsule_local
  const double p1 = py - fmin(fmax(py, 0.0), ch);
  return sqrt(pl[0] * pl[0] + p1 * p1 + pl[2] * pl[2] + 1e-14) - radius;
}
// n / length(n) and its adjoint (gn assigned)
__device__ __forceinline__ void plb_normalize3(const double* n, double* o) {
  const double il = 1.0 / sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2] + 1e-14);
  o[0] = n[0] * il; o[1] = n[1] * il; o[2] = n[2] * il;
}
__device__ __forceinline__ void plb_normalize3_adj(const double* n, const double* go, double* gn) {
  const double il = 1.0 / sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2] + 1e-14);
  const double s = (go[0] * n[0] + go[1] * n[1] + go[2] * n[2]) * il * il * il;
#pragma unroll
  for (int k = 0; k < 3; ++k) gn[k] = go[k] * il - s * n[k];
}
// the local normal (_normal of the kind)
template <int SH = 1>
__device__ __forceinline__ void plb_shape_normal(int kind, const double* sc, double ch, const double* pl, double* nl) {
  if constexpr (SH == 2) {
    if (kind == 6) {                                         // Chopsticks: the selected stick's p / len
      double p[3], pass_y, half;
      const double il = 1.0 / plb_chop_pick(sc[0], ch, pl, p, pass_y, half);
      nl[0] = p[0] * il; nl[1] = p[1] * il; nl[2] = p[2] * il;
      return;
    }
  }
  if (kind == 3) {                                           // Box: central differences of _sdf, normalised (:259-269)
    double n[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double inc[3] = {pl[0], pl[1], pl[2]}, dec[3] = {pl[0], pl[1], pl[2]};
      inc[i] += PLB_BOX_D; dec[i] -= PLB_BOX_D;
      n[i] = (0.5 / PLB_BOX_D) * (plb_box_sdf(sc, inc) - plb_box_sdf(sc, dec));
    }
    plb_normalize3(n, nl);
  } else if (kind == 4) {                                    // Cylinder (:189-202)
    const double l = sqrt(pl[0] * pl[0] + pl[2] * pl[2] + 1e-14);
    const double d0 = l - sc[0], d1 = fabs(pl[1]) - sc[1];
    const double f = d0 > d1 ? 1.0 : 0.0, in = fmax(d0, d1) <= 0.0 ? 1.0 : 0.0;
    const double n20 = fmax(d0, 0.0) + in * f, n21 = fmax(d1, 0.0) + in * (1 - f);
    const double l2 = sqrt(n20 * n20 + n21 * n21 + 1e-14);
    const double sy = pl[1] >= 0.0 ? 1.0 : -1.0;
    const double n3[3] = {pl[0] / l * (n20 / l2), n21 / l2 * sy, pl[2] / l * (n20 / l2)};
    plb_normalize3(n3, nl);
  } else if (kind == 5) {                                    // Torus (:223-231)
    const double l = sqrt(pl[0] * pl[0] + pl[2] * pl[2] + 1e-14);
    const double q0 = l - sc[0], q1 = pl[1];
    const double lq = sqrt(q0 * q0 + q1 * q1 + 1e-14);
    const double n3[3] = {pl[0] / l * (q0 / lq), q1 / lq, pl[2] / l * (q0 / lq)};
    plb_normalize3(n3, nl);
  } else {                                                   // Capsule: p / len
    const double py = pl[1] + ch / 2;
    const double p1 = py - fmin(fmax(py, 0.0), ch);
    const double il = 1.0 / sqrt(pl[0] * pl[0] + p1 * p1 + pl[2] * pl[2] + 1e-14);
    nl[0] = pl[0] * il; nl[1] = p1 * il; nl[2] = pl[2] * il;
  }
}
// cotangents (gdist of the distance, gnl of the local normal) -> cotangent of pl (assigned); the intermediates are formed again from pl.
// SH == 2: also ggap (assigned), the cotangent of the gap -- that of the selected stick's local point in x times -+1/2; 0 for every other kind
template <int SH = 1>
__device__ __forceinline__ void plb_shape_adj(int kind, const double* sc, double ch, const double* pl, double gdist, const double* gnl, double* g,
                                              double* ggap = nullptr) {
  if constexpr (SH == 2) {
    *ggap = 0.0;
    if (kind == 6) {                                         // Chopsticks: the Capsule's adjoint at the selected stick
      double p[3], pass_y, half;
      const double il = 1.0 / plb_chop_pick(sc[0], ch, pl, p, pass_y, half);
      const double gl = gdist - (gnl[0] * p[0] + gnl[1] * p[1] + gnl[2] * p[2]) * il * il;
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] = gnl[k] * il + gl * p[k] * il;
      g[1] *= pass_y;
      *ggap = half * g[0];
      return;
    }
  }
  if (kind == 3) {
    double n[3], dg[3][3], gn[3], gs[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {                            // n_i = (0.5 / d) (sdf(pl + d e_i) - sdf(pl - d e_i)): each sample once, value and gradient
      double inc[3] = {pl[0], pl[1], pl[2]}, dec[3] = {pl[0], pl[1], pl[2]}, gi[3], gd[3];
      inc[i] += PLB_BOX_D; dec[i] -= PLB_BOX_D;
      n[i] = (0.5 / PLB_BOX_D) * (plb_box_sdf(sc, inc, gi) - plb_box_sdf(sc, dec, gd));
#pragma unroll
      for (int k = 0; k < 3; ++k) dg[i][k] = gi[k] - gd[k];
    }
    plb_normalize3_adj(n, gnl, gn);
    plb_box_sdf(sc, pl, gs);
    g[0] = gdist * gs[0]; g[1] = gdist * gs[1]; g[2] = gdist * gs[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double w = gn[i] * (0.5 / PLB_BOX_D);
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] += w * dg[i][k];
    }
  } else if (kind == 4) {
    const double l = sqrt(pl[0] * pl[0] + pl[2] * pl[2] + 1e-14);
    const double d0 = l - sc[0], d1 = fabs(pl[1]) - sc[1];
    const double f = d0 > d1 ? 1.0 : 0.0, in = fmax(d0, d1) <= 0.0 ? 1.0 : 0.0;
    const double m0 = fmax(d0, 0.0), m1 = fmax(d1, 0.0);
    const double n20 = m0 + in * f, n21 = m1 + in * (1 - f);
    const double l2 = sqrt(n20 * n20 + n21 * n21 + 1e-14);
    const double sy = pl[1] >= 0.0 ? 1.0 : -1.0;
    const double a0 = n20 / l2, a1 = n21 / l2, px = pl[0] / l, pz = pl[2] / l;
    const double n3[3] = {px * a0, a1 * sy, pz * a0};
    double gn3[3];
    plb_normalize3_adj(n3, gnl, gn3);
    const double gpx = gn3[0] * a0, gpz = gn3[2] * a0;
    const double ga0 = gn3[0] * px + gn3[2] * pz, ga1 = gn3[1] * sy;
    const double s2 = (ga0 * n20 + ga1 * n21) / (l2 * l2 * l2);        // a = n2 / length(n2)
    const double gn20 = ga0 / l2 - s2 * n20, gn21 = ga1 / l2 - s2 * n21;
    // the distance: min(max(d0, d1), 0) + length(max(d, 0))
    const double ls = sqrt(m0 * m0 + m1 * m1 + 1e-14);
    const double gd0 = (d0 > 0.0 ? gn20 : 0.0) + gdist * (m0 / ls + (in * f)), gd1 = (d1 > 0.0 ? gn21 : 0.0) + gdist * (m1 / ls + in * (1 - f));
    const double gl = gd0 - (gpx * pl[0] + gpz * pl[2]) / (l * l);      // d0 = l - h, p / l
    g[0] = gpx / l + gl * pl[0] / l; g[2] = gpz / l + gl * pl[2] / l;
    g[1] = gd1 * plb_sgn(pl[1]);
  } else if (kind == 5) {
    const double l = sqrt(pl[0] * pl[0] + pl[2] * pl[2] + 1e-14);
    const double q0 = l - sc[0], q1 = pl[1];
    const double lq = sqrt(q0 * q0 + q1 * q1 + 1e-14);
    const double a0 = q0 / lq, a1 = q1 / lq, px = pl[0] / l, pz = pl[2] / l;
    const double n3[3] = {px * a0, a1, pz * a0};
    double gn3[3];
    plb_normalize3_adj(n3, gnl, gn3);
    const double gpx = gn3[0] * a0, gpz = gn3[2] * a0;
    const double ga0 = gn3[0] * px + gn3[2] * pz, ga1 = gn3[1];
    const double s2 = (ga0 * q0 + ga1 * q1) / (lq * lq * lq);
    const double gq0 = ga0 / lq - s2 * q0 + gdist * a0, gq1 = ga1 / lq - s2 * q1 + gdist * a1;
    const double gl = gq0 - (gpx * pl[0] + gpz * pl[2]) / (l * l);
    g[0] = gpx / l + gl * pl[0] / l; g[2] = gpz / l + gl * pl[2] / l;
    g[1] = gq1;
  } else {                                                   // Capsule, as plb_capsule_local_adj
    const double py = pl[1] + ch / 2;
    const double p[3] = {pl[0], py - fmin(fmax(py, 0.0), ch), pl[2]};
    const double pass_y = (py >= 0.0 && py <= ch) ? 0.0 : 1.0;
    const double il = 1.0 / sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + 1e-14);
    const double gl = gdist - (gnl[0] * p[0] + gnl[1] * p[1] + gnl[2] * p[2]) * il * il;
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = gnl[k] * il + gl * p[k] * il;
    g[1] *= pass_y;
  }
}
// the pair the contact goes through on a shape handle, behind inv_trans as plb_capsule_local / _adj are: d = point - position -> pl and the distance
template <bool ROT = false, int SH = 1>
__device__ __forceinline__ double plb_shape_local(const PlbPrim& pr, const PlbShape& sh, int pi, double radius, const double* d, double* pl, const double* qi = nullptr,
                                                  const double* gap = nullptr) {
  plb_qrot(plb_sel<ROT>(pr.qi[pi], qi), d, pl);
  return plb_shape_sdf<SH>(pr.kind[pi], plb_shape_consts<SH>(pr, sh, pi, gap), pr.h[pi], radius, pl);
}
// cotangents (gdist, gnl, gpl of pl directly) -> cotangent of d; ROT: also gpl_all, the whole cotangent of pl; SH == 2: also ggap (plb_shape_adj)
template <bool ROT = false, int SH = 1>
__device__ __forceinline__ void plb_shape_local_adj(const PlbPrim& pr, const PlbShape& sh, int pi, const double* pl, double gdist, const double* gnl, const double* gpl,
                                                    double* gd, const double* qi = nullptr, double* gpl_all = nullptr, double* ggap = nullptr,
                                                    const double* gap = nullptr) {
  double g[3];
  if constexpr (SH == 2) plb_shape_adj<2>(pr.kind[pi], plb_shape_consts<2>(pr, sh, pi, gap), pr.h[pi], pl, gdist, gnl, g, ggap);
  else plb_shape_adj(pr.kind[pi], sh.c[pi], pr.h[pi], pl, gdist, gnl, g);
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] += gpl[k];
  plb_qrot_t(plb_sel<ROT>(pr.qi[pi], qi), g, gd);
  if constexpr (ROT) { gpl_all[0] = g[0]; gpl_all[1] = g[1]; gpl_all[2] = g[2]; }
}


// everything Primitive.collide (primive_base.py:91-115) computes for one cell, kept for the adjoint
struct PlbCollide {
  bool active, flag;
  double pl[3], p[3], pass_y, len, dist, D[3], e, infl, cv[3], w[3], nc, mn, t[3], tn, arg, ts[3];
};
// what p holds differs by handle: the Capsule's unnormalised vector from the axis segment (with len and pass_y beside it), and on a shape handle
// (SH) the unit local normal itself, len and pass_y unused.  Read the unit local normal through this, never through p directly.
template <int SH> __device__ __forceinline__ void plb_local_normal(const PlbCollide& k, double* nl) {
  if constexpr (SH != 0) { nl[0] = k.p[0]; nl[1] = k.p[1]; nl[2] = k.p[2]; }
  else { nl[0] = k.p[0] / k.len; nl[1] = k.p[1] / k.len; nl[2] = k.p[2] / k.len; }
}
// gp: cell position, P0 / P1: the primitive's position at substeps f / f + 1, sf: softness, u: the cell velocity so far; ROT: q0 / qi / q1 =
// rotation[f], conj / |.| of it, rotation[f + 1]
// SH (a shape handle): distance and normal through the shape layer, sh = the handle's shape constants (SH == 2: with the gap of this substep)
template <bool ROT = false, int SH = 0>
__device__ __forceinline__ void plb_collide_eval(const PlbPrim& pr, int pi, double radius, double dt, const double* gp, const double* P0, const double* P1,
                                                 double sf, const double* u, PlbCollide& k, const double* q0 = nullptr, const double* qi = nullptr,
                                                 const double* q1 = nullptr, const PlbShape* sh = nullptr, const double* gap = nullptr) {
  const double d[3] = {gp[0] - P0[0], gp[1] - P0[1], gp[2] - P0[2]};
  if constexpr (SH != 0) {
    k.dist = plb_shape_local<ROT, SH>(pr, *sh, pi, radius, d, k.pl, qi, gap);
  } else {
    k.len = plb_capsule_local<ROT>(pr, pi, d, k.pl, k.p, k.pass_y, qi);
    k.dist = k.len - radius;
  }
  k.e = exp(-k.dist * sf);
  k.infl = fmin(k.e, 1.0);
  k.active = (sf > 0 && k.infl > 0.1) || k.dist <= 0;       // no 0.001 and no trailing `and softness > 0`: those are the Sphere override's
  k.flag = false;
  if (!k.active) return;
  if constexpr (SH != 0) plb_shape_normal<SH>(pr.kind[pi], plb_shape_consts<SH>(pr, *sh, pi, gap), pr.h[pi], k.pl, k.p);
  double nl[3], back[3];
  plb_local_normal<SH>(k, nl);
  plb_qrot(plb_sel<ROT>(pr.q[pi], q0), nl, k.D);
  plb_qrot(plb_sel<ROT>(pr.q[pi], q1), k.pl, back);          // constant orientation: rotation[f + 1] = rotation[f]
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
template <int SH = 0>
__device__ __forceinline__ bool plb_collide(const PlbPrim& pr, int pi, double radius, double dt, const double* gp, const double* P0, const double* P1, double sf,
                                            double* u, const PlbShape* sh = nullptr) {
  PlbCollide k;
  plb_collide_eval<false, SH>(pr, pi, radius, dt, gp, P0, P1, sf, u, k, nullptr, nullptr, nullptr, sh);
  if (!k.active) return false;
#pragma unroll
  for (int i = 0; i < 3; ++i) u[i] = k.cv[i] + k.w[i] * (1 - k.infl) + k.ts[i] * k.infl;
  return true;
}
// the same on a rot_state handle: q0 / q1 = rotation[f] / rotation[f + 1] of this env and primitive
template <int SH = 0>
__device__ __forceinline__ void plb_collide_eval_rot(const PlbPrim& pr, int pi, double radius, double dt, const double* gp, const double* P0, const double* P1,
                                                     const double* q0, const double* q1, double sf, const double* u, PlbCollide& k, const PlbShape* sh = nullptr,
                                                     const double* gap = nullptr) {
  double qi[4];
  plb_qinv(q0, qi);
  plb_collide_eval<true, SH>(pr, pi, radius, dt, gp, P0, P1, sf, u, k, q0, qi, q1, sh, gap);
}
template <int SH = 0>
__device__ __forceinline__ bool plb_collide_rot(const PlbPrim& pr, int pi, double radius, double dt, const double* gp, const double* P0, const double* P1,
                                                const double* q0, const double* q1, double sf, double* u, const PlbShape* sh = nullptr, const double* gap = nullptr) {
  PlbCollide k;
  plb_collide_eval_rot<SH>(pr, pi, radius, dt, gp, P0, P1, q0, q1, sf, u, k, sh, gap);
  if (!k.active) return false;
#pragma unroll
  for (int i = 0; i < 3; ++i) u[i] = k.cv[i] + k.w[i] * (1 - k.infl) + k.ts[i] * k.infl;
  return true;
}
// adjoint of an ACTIVE collide: G = cotangent of u_out (in), cotangent of u_in (out, may alias nothing of the inputs); g0 / g1 = cotangents of P_f / P_{f+1}.
// ROT: also gq0 / gq1 = cotangents of rotation[f] (through the normal's rotation back, the local point and the inverse with its normalisation) and of
// rotation[f + 1] (through the collider velocity), assigned; d = cell - P_f.
template <bool ROT = false, int SH = 0>   // SH == 2: gap as plb_collide_eval took it; also ggap (assigned), the cotangent of gap[pi]
__device__ __forceinline__ void plb_collide_adj(const PlbPrim& pr, int pi, double dt, const PlbCollide& k, double sf, const double* G, double* gu, double* g0,
                                                double* g1, const double* q0 = nullptr, const double* qi = nullptr, const double* q1 = nullptr,
                                                const double* d = nullptr, double* gq0 = nullptr, double* gq1 = nullptr, const PlbShape* sh = nullptr,
                                                double* ggap = nullptr, const double* gap = nullptr) {
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
  plb_qrot_t(plb_sel<ROT>(pr.q[pi], q1), gback, gpl);
  plb_qrot_t(plb_sel<ROT>(pr.q[pi], q0), gD, gnl);
  [[maybe_unused]] double gpl_all[3];
  if constexpr (SH == 2) plb_shape_local_adj<ROT, 2>(pr, *sh, pi, k.pl, glen, gnl, gpl, gd, qi, gpl_all, ggap, gap);
  else if constexpr (SH != 0) plb_shape_local_adj<ROT>(pr, *sh, pi, k.pl, glen, gnl, gpl, gd, qi, gpl_all);
  else plb_capsule_local_adj<ROT>(pr, pi, k.p, k.len, k.pass_y, glen, gnl, gpl, gd, qi, gpl_all);
#pragma unroll
  for (int i = 0; i < 3; ++i) g0[i] = -gd[i];                // d = g - P_f
  if constexpr (ROT) {
    double nl[3], gqi[4];
    plb_local_normal<SH>(k, nl);
    plb_qrot_adj_rot(q1, k.pl, gback, gq1);
    plb_qrot_adj_rot(q0, nl, gD, gq0);
    plb_qrot_adj_rot(qi, d, gpl_all, gqi);
    plb_qinv_adj(q0, qi, gqi, gq0);
  }
}
template <int SH = 0>
__device__ __forceinline__ void plb_collide_adj_rot(const PlbPrim& pr, int pi, double dt, const PlbCollide& k, double sf, const double* gp, const double* P0,
                                                    const double* q0, const double* q1, const double* G, double* gu, double* g0, double* g1, double* gq0,
                                                    double* gq1, const PlbShape* sh = nullptr, double* ggap = nullptr, const double* gap = nullptr) {
  double qi[4];
  plb_qinv(q0, qi);
  const double d[3] = {gp[0] - P0[0], gp[1] - P0[1], gp[2] - P0[2]};
  plb_collide_adj<true, SH>(pr, pi, dt, k, sf, G, gu, g0, g1, q0, qi, q1, d, gq0, gq1, sh, ggap, gap);
}

}  // namespace ud
