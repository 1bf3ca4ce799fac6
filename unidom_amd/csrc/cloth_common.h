// Shared argument structs of the cloth kernels (exact-order kernels: cloth.hip, fast kernels: cloth_fast.hip).
#pragma once
#include "common.h"

namespace ud {

struct ClothConst {
  float gdt;      // float(gravity*dt)        :259
  float g;        // gravity                  :278
  float dt;
  float damp;     // exp(-damping*dt) in f32  :309
  float max_v;
  float eps;      // small_num
  float n_mask;   // cloth_mask.sum()         :192
  int P, Pp, S;
  float cell;     // 1/N
  float Ls, Ld;   // rest lengths of the straight (links 0-3) / diagonal (4-7) springs, f32 as cloth_simulator.py:61-63
};

struct ClothFwdArgs {
  ClothConst c;
  const int* nbr;      // [8][Pp]
  const float* L0;     // [8][Pp]
  int B, T;
  const float *x, *v, *prim, *k, *mu, *actions;
  float *x_out, *v_out, *prim_out, *x_list, *v_list, *prim_list;
  float* ckpt;
  uint8_t* grasp;
};

struct ClothBwdArgs {
  ClothConst c;
  const int* nbr;
  const float* L0;
  int B, T;
  const float* ckpt;
  const float *k, *mu, *actions;
  const float *g_x, *g_v, *g_prim, *g_x_list, *g_v_list, *g_prim_list;
  int normalize;
  float *g_x0, *g_v0, *g_prim0, *g_actions, *g_k, *g_mu;
  int dec;   // the checkpoint carries decision words (below): cloth_launch_bwd_fast runs the kernels that read them
};


// Checkpoint arena written by the forward kernels, read by the backward kernels:
//   per env b: (T*S + 1) records of (6*Pp + 8) floats = x[3][Pp] | v[3][Pp] | primitive0[4] primitive1[4];
//   record t*S+s is the INPUT state of substep (t,s); the last record is the final state.
//   Behind the records of ALL envs, where the one-workgroup fast adjoint will run on at most UD_CLOTH_DEC_MAX_B envs (cloth.hip,
//   cloth_use_decisions): B * T*S * Pp decision words, [b][t*S+s][lane] -- the discrete choices of substep (t,s) as the forward took
//   them, written by cloth_decisions_kernel (cloth_fast_bwd.hip) right behind the forward kernel and read by the adjoint's sweep in
//   place of re-deriving them.  The records' layout and per-env stride are the same with and without the words.
__host__ __device__ inline size_t cloth_rec_floats(int Pp) { return (size_t)6 * Pp + 8; }
__host__ __device__ inline size_t cloth_env_records(int T, int S) { return (size_t)T * S + 1; }
__host__ __device__ inline size_t cloth_dec_words(int B, int T, int S, int Pp) { return (size_t)B * T * S * Pp; }

// One decision word (all factors are discrete; no float leaves the sweep, so no rounding can move):
//   bits  0-7, 8-15, 16-23   2 * clip_grad_01(x2[d]), d = 0, 1, 2: 0 / 1 / 2 (byte fields: v_cvt_f32_ubyteN, times 0.5, both exact)
//   bits 24, 25, 26          |v_{n+1}[d]| < max_v
//   bit  27, 28              the particle is held by gripper 0, gripper 1
//   bits 29-30               lanes 0-7 only: 2 * clip_grad_01 of this lane's component of the moved primitives
// A padding lane (i >= P) holds 0 in every particle field.
constexpr int UD_DEC_DV = 24, UD_DEC_M0 = 27, UD_DEC_M1 = 28, UD_DEC_PRIM = 29;
// Largest B that takes the decisions path: the pre-pass streams every record once, so its time grows with B, while the sweep's
// saving does not (envs run side by side).  Measured table: profiles/r12_ablation.txt, DESIGN.md 3.1.
#ifndef UD_CLOTH_DEC_MAX_B
#define UD_CLOTH_DEC_MAX_B 32
#endif

// The grasp test |x - pos| <= radius (cloth_simulator.py:201,213) without a per-particle square root.  IEEE sqrtf
// is monotone, so  sqrtf(s) <= r  <=>  s <= T(r)  where T(r) is the largest float whose correctly rounded root is
// <= r: the booleans are identical to the sqrt form's (this is what keeps cloth_v2.hip bit-exact to the oracle).
// T(r) lies within [-1, +3] ulp of RN(r*r) (|(r + ulp/2)^2 - r^2| < 2.5 ulp(r^2)), so a short walk finds it; the
// result is verified and a miss traps instead of returning a wrong set (unreachable: tools/check_exact_math.hip runs
// the same walk for all 2 139 095 040 finite non-negative radii on the GPU and finds every one tight).
__device__ inline float grasp_thr(float r) {
  if (!(r >= 0.f)) return -1.f;                         // negative / NaN radius never grasps (s >= 0)
  if (r == INFINITY) return r;
  unsigned t = __builtin_bit_cast(unsigned, r * r);
  for (int it = 0; it < 4; ++it) if (sqrtf(__builtin_bit_cast(float, t)) > r) --t;
  for (int it = 0; it < 4; ++it) if (sqrtf(__builtin_bit_cast(float, t + 1u)) <= r) ++t;
  if (!(sqrtf(__builtin_bit_cast(float, t)) <= r && !(sqrtf(__builtin_bit_cast(float, t + 1u)) <= r))) __builtin_trap();
  return __builtin_bit_cast(float, t);
}

// The radius is component 3 of a primitive; the substep maps it to clip(radius + 0, 0, 1) (:322-323), which is
// idempotent: only the very first substep of a rollout can see an unclipped radius.  Two thresholds per gripper
// (first substep / every later one), computed once per launch, uniform.
struct GraspThr {
  float first, rest;
  __device__ __forceinline__ void init(float radius0) {
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, radius0)));
    first = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, grasp_thr(r0))));
    rest = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, grasp_thr(clipf(r0 + 0.f, 0.f, 1.f)))));
  }
  __device__ __forceinline__ float at(bool first_substep) const { return first_substep ? first : rest; }
};

// Issue priority of the one-workgroup rollout kernels at two waves per SIMD (bodies of 257-512 padded particles: wave w shares its
// SIMD with wave w + 4).  The SIMD arbitrates VALU issue by priority, then age: at equal priority the first-dispatched wave runs nearly
// unimpeded, its partner gets the leftover slots, arrives late at every barrier, and while it finishes alone the SIMD issues at one
// wave's rate (measured: waves 0-3 waited a third of every substep at the barriers, waves 4-7 not at all;
// profiles/r10_wave_stamps.txt).  So the losing wave enters every barrier interval at priority 1 (`up`, in front of the barrier that
// opens it) and drops to 0 part-way through (`drop`), where age hands the SIMD to its partner and both reach the next barrier together.
// s_setprio is a scalar instruction that ignores EXEC: `lose` is wave-uniform (readfirstlane) and the kernels branch on it ONCE,
// into a copy of their loop with the priority changes or into one without any.  A wave with no partner on its SIMD (every wave of a body
// of at most 256 padded particles, waves 1-3 of a 5-wave body) and a body of more than 8 waves run the copy without.
struct WavePrio {
  bool lose;
  __device__ __forceinline__ void init(int Pp) {
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 6;
    lose = w >= 4 && Pp <= 512;   // waves 4-7 were the later-dispatched half in every workgroup sampled
  }
  static __device__ __forceinline__ void up() { __builtin_amdgcn_s_setprio(1); }
  // pinned against the instruction scheduler; arithmetic that the optimiser moves before scheduling can still cross it, so the place is
  // read off the ISA (tools/asm_loop_stats.py --dump) at every change of the surrounding code
  static __device__ __forceinline__ void drop() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  }
};

void cloth_launch_fwd_v2(const ClothFwdArgs& a, hipStream_t stream);
bool cloth_ref_consts_ok(const ClothConst& c);                                 // cloth_ref.hip: the mode-3 fast path's per-launch constant checks
bool cloth_ref_fast_ok(const ClothConst& c);                                   // ... and Pp <= 512: cloth_ref.hip's kernel may run
void cloth_launch_fwd_ref(const ClothFwdArgs& a, hipStream_t stream);
void cloth_launch_fwd_fast(const ClothFwdArgs& a, hipStream_t stream);
void cloth_launch_bwd_fast(const ClothBwdArgs& a, hipStream_t stream);
void cloth_launch_decisions(const ClothConst& c, int B, int T, float* ckpt, const float* actions, hipStream_t stream);   // cloth_fast_bwd.hip

}  // namespace ud
