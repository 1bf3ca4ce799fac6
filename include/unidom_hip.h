/*
 * unidom_hip.h -- C ABI of libunidom_hip.so: MI355X (gfx950) kernels for the differentiable-physics
 * hot path of Kuroki1931/UniDOM (the substep that APG training drives through env.step_diff).
 *
 * The reference has no FFI for this path: it sits behind a Python/JAX functional API
 *     simulator.step_jax(state, action) -> (state, state)
 * consumed by lax.scan in step_diff and differentiated by jax.grad.  Each entry point below names the
 * reference interface it replaces (paths relative to /root/reference/DaXBench/daxbench/).
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer (HBM) unless marked "host"; float32, C-contiguous, AoS at the
 *     boundary ([B,P,3] etc., the reference's own layouts); the library transposes to SoA internally.
 *   - purely functional like the reference (NamedTuple._replace): inputs are never written, the caller owns
 *     every state / gradient / checkpoint buffer; a handle owns constant tables and, for the many-workgroup MPM and
 *     PLB paths, a scratch arena (HBM grid + active-cell lists) that is (re)allocated when a larger batch arrives.
 *   - all launches are asynchronous on `stream` (a hipStream_t passed as void*); no allocation and no host synchronisation
 *     inside any rollout / step / loss call: handle-owned scratch is allocated in ud_*_create for conf.max_envs envs
 *     (the reference's per-handle constants, mpm_simulator.py:117-122,154: the batch size is known when the simulator
 *     is built) and a call with more envs than that returns UD_ERR_INVALID.  The only entry points that synchronise
 *     are the ud_*_poll_* / ud_*_reset calls, which say so.
 *   - return value: 0 = ok, negative = ud_status; ud_last_error() gives the text (thread-local).
 *   - a handle is bound to the device current at create time; not thread-safe per handle.
 */
#ifndef UNIDOM_HIP_H
#define UNIDOM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  UD_OK = 0,
  UD_ERR_INVALID = -1,      /* bad argument (null pointer, size out of range) */
  UD_ERR_UNSUPPORTED = -2,  /* configuration the kernels do not cover (stated in the message) */
  UD_ERR_HIP = -3,          /* a HIP runtime call failed (no device, launch error, ...) */
  UD_ERR_OVERFLOW = -4      /* a device-side capacity (MPM LDS cell table) was exceeded */
} ud_status;

const char* ud_last_error(void);
/* 3-part version + the gfx arch the code object was built for, e.g. "0.1.0 gfx950" */
const char* ud_version(void);

/* ------------------------------------------------------------------------------------------------
 * Cloth (mass-spring) -- replaces ClothSimulator.step_jax = vmap(jit(robot_step_wrapper))
 *   core/engine/cloth_simulator.py:26-70 (tables), :163-180 (robot_step), :257-337 (step),
 *   :198-226 (gripper), :182-196 (norm_grad), :228-255 (what is differentiated)
 * driven by lax.scan over the 40 macro actions of one step_diff (core/envs/basic/cloth_env.py:211).
 * ------------------------------------------------------------------------------------------------ */
typedef struct ud_cloth ud_cloth;

typedef struct {
  int N;           /* lattice size (80)                    fold_cloth1_env.py:17 */
  float gravity;   /* 0.5                                  :19 */
  float damping;   /* 2                                    :21 */
  float dt;        /* 2e-3                                 :22 */
  float max_v;     /* 2.0                                  :23 */
  float small_num; /* 1e-8                                 :24 */
  int substeps;    /* 50 = fori_loop bound                 cloth_simulator.py:176 */
  int mode;        /* 0 (default): forward in operation order "v2" -- the reference's formulas re-associated into fewer
                    *    IEEE operations, no FMA contraction; bit-identical to the CPU restatement compiled in the SAME
                    *    order (oracle cloth_substep_fwd_v2), and 1.5e-5 (v, one substep) / 9e-3 (50 substeps) away from
                    *    the reference-order restatement in f32, 1e-9 in f64 -- + restructured adjoint
                    *    kernel (one reduction round per substep);
                    * 1: forward in the reference's literal f32 operation order (bit-identical to the CPU restatement
                    *    of that order) AND reference-order adjoint (six reductions per substep);
                    * 2: v2 structure with fast-math (v_rsq, FMA) forward + restructured adjoint (f32 round-off
                    *    differences, which this stiff system amplifies over long rollouts -- see DESIGN.md).
                    * 3: forward in the reference's literal f32 operation order (mode 1's forward kernel: k*r/len*(len-L0)/L0,
                    *    cloth_simulator.py:264-268, and the friction block :281-306 as written; bit-identical to the CPU
                    *    restatement of THAT order) + the restructured adjoint of modes 0 / 2 (it reads the same checkpoint
                    *    records and re-derives the grasp sets from them).  Bodies of at most 512 particles or of more
                    *    than 1024 (UD_ERR_UNSUPPORTED for 513-1024).
                    * Bodies of 513-1024 particles (padded to whole waves: 512 < Pp <= 1024) have mode 1's kernels only, one
                    *    workgroup of Pp lanes per env: modes 0 and 2 run them as well, so THERE THE FORWARD IS IN THE REFERENCE'S
                    *    LITERAL ORDER (bit-identical to the reference-order restatement, not to v2's) and the adjoint is the
                    *    literal six-reduction one; mode 3 is refused.
                    * Bodies above 1024 particles: modes 0 / 2 run the v2-order forward and the restructured adjoint on
                    *    SEVERAL workgroups per env (512 particles each, halo positions / force cotangents / block sums handed
                    *    over through HBM every substep; forward still bit-identical to the v2 restatement); mode 3 runs the
                    *    reference-order forward on the same parts and hand-off (bit-identical to the reference-order
                    *    restatement) and the same restructured adjoint; mode 1 runs the reference-order kernels on one
                    *    1024-lane workgroup per env.  Where the several-workgroup kernels do not apply (one_workgroup_per_env,
                    *    a spring spanning more than 256 particle indices, more parts than CUs per XCD) modes 0 / 2 / 3 run
                    *    mode 1's one-workgroup kernels too: reference order. */
  int max_envs;    /* the largest B any call on this handle will pass (>= 1): handle-owned scratch (bodies above 1024 particles: the
                    * several-workgroup kernels' hand-off arena, or the one-workgroup adjoint's parking area) is allocated in
                    * ud_cloth_create for this many envs; a call with more returns UD_ERR_INVALID */
  int one_workgroup_per_env;   /* bodies above 1024 particles only.  != 0: keep the one-workgroup-per-env kernels where the library would
                    * run several workgroups per env (diagnostics and tests; fixed at create) */
} ud_cloth_conf;

/* mask: host pointer, N*N bytes, row-major, non-zero = cloth particle (create_cloth_mask,
 * fold_cloth1_env.py:48-53).  Particle order = row-major nonzero(mask) (cloth_simulator.py:52).
 * Limits: 1 <= P <= 4096 (P <= 1024: one workgroup per env, one particle per lane -- the kernels of the handle's mode up to 512
 * particles, mode 1's reference-order forward and literal adjoint in modes 0 / 1 / 2 for 513-1024; above: ceil(P / 512) workgroups per
 * env, one particle per lane -- a call is cut into launches of ud_cloth_launch_envs() envs so that the workgroups that
 * wait for each other are resident together -- or, in mode 1 / when a spring spans more than 256 particle indices, one
 * workgroup per env with up to four particles per lane); the mask must not touch the lattice border
 * (UD_ERR_UNSUPPORTED otherwise). */
int ud_cloth_create(const ud_cloth_conf* conf, const uint8_t* mask, ud_cloth** out);
void ud_cloth_destroy(ud_cloth* h);
int ud_cloth_num_particles(const ud_cloth* h);
/* envs per kernel launch of a call with B envs (B itself unless the several-workgroup kernels run: then at most
 * 8 * floor((CUs / 8) / parts), every XCD holding whole envs) */
int ud_cloth_launch_envs(const ud_cloth* h, int B);
/* Several-workgroup kernels only: a part that waits for a sibling longer than ~seconds gives up, the env's outputs are
 * NaN and a device-side counter is raised.  This call SYNCHRONISES `stream`, returns the number of such workgroups
 * since the previous call (0 = none; also 0 for handles that never take that path; ud_last_error() holds the text
 * otherwise) and resets the counter.  The rollout calls themselves stay asynchronous and return UD_OK. */
int ud_cloth_poll_timeouts(ud_cloth* h, void* stream);
/* bytes of the per-substep checkpoint arena a forward rollout of T macro steps x B envs writes: the records of all envs,
 * B * (T * substeps + 1) * (6 * Ppad + 8) floats, and behind them -- only where the one-workgroup restructured adjoint will
 * run (a body of at most 512 padded particles, mode != 1) on at most 32 envs -- one 32-bit decision word per env, substep
 * and padded particle, written by the forward call for the adjoint.  The same B and T must be given to both rollout calls. */
size_t ud_cloth_ckpt_bytes(const ud_cloth* h, int B, int T);

/* Forward: T macro steps (robot_step) of `substeps` substeps each, for B independent envs.
 *   x, v [B,P,3]; prim [B,2,4] = (primitive0, primitive1) = (pos xyz, radius); stiffness, mu [B];
 *   actions [T,B,8] (the scan xs: get_pnp_actions output, cloth_env.py:134-173).
 * Outputs: final x_out, v_out [B,P,3], prim_out [B,2,4]; optional per-macro-step state_list
 *   x_list, v_list [T,B,P,3], prim_list [T,B,2,4] (the scan ys, may be NULL);
 *   ckpt (may be NULL = no backward): ud_cloth_ckpt_bytes() bytes, opaque, consumed by ud_cloth_rollout_bwd;
 *   grasp (may be NULL, debug/tests): [T,substeps,B,2,P] bytes, 1 where the gripper mask was true (Q3). */
int ud_cloth_rollout_fwd(ud_cloth* h, int B, int T, const float* x, const float* v, const float* prim,
                         const float* stiffness, const float* mu, const float* actions, float* x_out,
                         float* v_out, float* prim_out, float* x_list, float* v_list, float* prim_list,
                         void* ckpt, uint8_t* grasp, void* stream);

/* Backward: the adjoint jax.grad produces through robot_step_wrapper / step_wrapper
 * (cloth_simulator.py:107-145, :228-255) including the per-substep norm_grad rescaling (:189-194) when
 * normalize != 0.  g_x, g_v [B,P,3], g_prim [B,2,4]: cotangents of the final state;
 * g_*_list (may be NULL): cotangents of the scan ys.  Outputs: cotangents of the initial state,
 * of actions [T,B,8] and the contributions to stiffness / mu [B] (the identity pass-through of those two
 * state fields is the caller's to add). */
int ud_cloth_rollout_bwd(ud_cloth* h, int B, int T, const void* ckpt, const float* stiffness, const float* mu,
                         const float* actions, const float* g_x, const float* g_v, const float* g_prim,
                         const float* g_x_list, const float* g_v_list, const float* g_prim_list, int normalize,
                         float* g_x0, float* g_v0, float* g_prim0, float* g_actions, float* g_stiffness,
                         float* g_mu, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MLS-MPM -- replaces SimpleMPMSimulator.step_jax = vmap(jit(step))
 *   core/engine/mpm_simulator.py:27-63 (constructor), :413-429 (step), :223-330 (substep),
 *   :178-221 (p2g_micro / g2p_micro), :365-373 (copy_frame), :375-411 (norm_grad_state / norm_grad),
 *   core/engine/svd_safe_batch.py:19-102 (svd + safe VJP),
 *   core/engine/primitives/primitives.py:185-239 (forward_kinematics, set_action, position_control_batch),
 *   core/engine/primitives/box.py:6-18 (box SDF)
 * driven by lax.scan over the macro actions of one step_diff (core/envs/basic/mpm_env.py:141).
 * One call = one `simulator.step` = conf.steps substeps for B independent envs, ONE kernel launch.
 *   core/engine/primitives/primitives.py:105-182 (inv_trans, sdf, finite-difference normal, collider velocity,
 *   collide_batch)
 *   core/engine/primitives/container.py:8-16 (container SDF)
 * Scope this round: one box primitive in position-control mode (whip_rope); 1..4 box or container primitives in
 * soft-contact mode (collide_batch: shape_rope, pour_water), applied one after the other (mpm_simulator.py:292-294).
 * With n_primitive = P > 1 every primitive array gains a primitive axis after the env axis -- position [B,P,steps,3],
 * rotation [B,P,steps,4], size [B,P,3], v / w [B,P,steps,3], action [B,6P] -- in both directions.  Materials 1 (elastic), 2 (plastic clamp) and 0 (liquid mu=0, la=1) in the particle pre-pass.
 * Position control with N <= 128 particles per env: one workgroup per env, the touched part of the `res` grid in an
 * LDS cell table, ONE launch per step.  N > 128, or soft contact: many workgroups per env, dense grid in HBM, a few
 * launches per substep (all on `stream`).
 * ------------------------------------------------------------------------------------------------ */
typedef struct ud_mpm ud_mpm;

typedef struct {
  int n_particles;
  int n_grid;                /* conf.n_grid (dx = 1/n_grid)                 whip_rope_env.py:47 */
  int res[3];                /* conf.res: allocated grid (index wrap/clamp)  :59 */
  int steps;                 /* conf.steps substeps per step                :51 */
  float dt;                  /* :48 */
  float p_mass, p_vol;       /* :62-63 */
  float gravity[3];          /* :64 */
  int use_position_control;  /* 1: position_control_batch (primitives.py:232-239), 0: collide_batch soft contact (:154-182) */
  float prim_friction;       /* PrimitiveState.friction  (create_primitive, mpm_env.py:201-207): collide_batch only */
  float prim_softness;       /* PrimitiveState.softness  (666 in every reference env): collide_batch only */
  int n_primitive;           /* conf.n_primitive (0 = 1).  > 1 (up to 4) in soft-contact mode only: pour_water_env.py:32 */
  int sdf_kind;              /* the SDF installed by set_sdf (primitives.py:26-28): 0 box (box.py:6-18), 1 container =
                                cut hollow sphere, size = (r, h, t) (container.py:8-16); soft-contact mode only */
  int grid_ckpt_cells;       /* many-workgroup path only.  0: the backward recomputes p2g + grid op per substep (the reference
                                rematerialises the whole substep, mpm_simulator.py:332-359).  K > 0: the forward also
                                checkpoints the active grid cells (32 B each) into a pool of K * n_particles records per
                                substep on average, inside the caller's checkpoint (ud_mpm_ckpt_bytes grows accordingly),
                                and the backward restores them.  A pool that runs out flags the env in status[] (1) and in a word
                                of the checkpoint itself, which ud_mpm_step_bwd reads on the device under clip bit 2 */
  int sort_particles;        /* many-workgroup path only.  != 0: at every step the handle re-orders the particles by grid cell
                                (Morton key) internally, for bodies whose particles come in no spatial order (uniformly
                                sampled liquids, mpm_simulator.py:87-91); bodies above 8192 particles keep their order (the
                                sort runs in the LDS of one workgroup per env).  Invisible at this boundary: inputs, outputs and
                                gradients stay in the caller's order; only the summation order of the scatters changes */
  float prim_friction_each[4], prim_softness_each[4];   /* soft contact with several primitives: friction / softness of primitive i where
                                prim_softness_each[i] > 0 (create_primitive passes them per primitive, mpm_env.py:201-217); entries left
                                at 0 take prim_friction / prim_softness (every reference env passes 0.1 / 666 to all of them) */
  int deterministic;         /* != 0: ud_mpm_step_fwd sums every grid cell in the order of the reference's flattened scatter-add array
                                (mpm_simulator.py:178-194: [27 offsets][N particles] -- offsets in (i, j, k) order, the particles of an
                                offset in ascending index), in f32, and g2p adds its cells in (i, j, k) order; no float atomics, IEEE
                                arithmetic (no FMA contraction, correctly rounded divide / sqrt).  Two calls on the same inputs return
                                the same bits, and x, v, C, F equal the CPU build of the same source bit for bit (tests/test_mpm_det.py).
                                Per substep the particles are bucketed by base cell (one sort per env) and a cell walks the 27 buckets
                                that can reach it: 3.1x the default forward at 67 particles, 5.3x at 798 (profiles/r04*_det_cost.txt; rounds
                                2-3, every cell walking every particle: 13x / 332x).  Position control or soft contact (collide_batch of
                                box / container primitives: its exp is a plain-IEEE polynomial in this mode so that both builds agree; a
                                primitive's ROTATION still goes through the platform's sinf / cosf); at most 8192 particles
                                (UD_ERR_UNSUPPORTED otherwise); grid_ckpt_cells and sort_particles are ignored.  ud_mpm_step_bwd of such a
                                handle is deterministic too -- the grid recomputed by the deterministic forward's kernels, the g2p adjoint's
                                scatter an ordered sum per cell over (offset, particle), every per-env sum (ground friction, controlled
                                velocity, the collide adjoint's per-primitive cotangents, mu / lamda, the clip's norm) added in a fixed
                                order: two calls return the same bits (fast-math arithmetic, so no CPU build is bit-equal to it; checked
                                against the oracle by tolerance).  At most 32768 touched cells per env and substep (status[b] = 1 beyond) */
  int max_envs;              /* the largest B any call on this handle will pass (>= 1).  Every arena of the many-workgroup path (dense
                                grids, active lists, cotangent grids, the persistent forward's rotating grids, the deterministic mode's
                                scratch) is allocated in ud_mpm_create for this many envs: no step call allocates or synchronises the
                                host; a call with B > max_envs returns UD_ERR_INVALID.  (SimpleMPMSimulator's batch size,
                                mpm_simulator.py:27-63: known when the simulator is built) */
  /* Kernel selection of the many-workgroup path, fixed at create; 0 everywhere = the library's choice by measurement,
     which ud_mpm_launch_plan reports.  The other values exist for diagnostics and so that the tests can put every kernel before the
     oracle at sizes the oracle can follow: */
  int tune_lanes;            /* lanes per particle of the particle kernels: 0 = 4 below 100 000 particles per launch, 1 beyond; 1 / 4 force */
  int tune_cluster;          /* the persistent forward (one launch per step call): 0 = solids with one primitive in the four-lane regime;
                                1 = wherever its parts fit the chip; -1 = never (the multi-kernel forward) */
  int tune_cluster_part_lanes; /* its lanes per part: 0 = 128 (32 particles), 64 (16 particles: a part can never outgrow its cell table) */
  int tune_cluster_envs;     /* > 0: at most this many envs per persistent launch (several launches per call) */
  int tune_env_groups;       /* > 0: this many stream groups on the multi-kernel path (1 = everything on the caller's stream) */
  int tune_bwd_two_launch;   /* backward with the grid checkpoint: 0 = two launches per reverse substep where they apply (four lanes, one
                                primitive); -1 = always the four-kernel sequence */
  int tune_collide_records;  /* soft contact with the grid checkpoint: 0 = the forward's grid op leaves exp(-dist * softness) and the
                                finite-difference normal of every cell and primitive beside the checkpoint and the grid-op adjoint reads them
                                (16 B per cell, primitive and substep each way; same bits as evaluating the SDFs again); -1 = the adjoint
                                evaluates the SDFs again (7 per cell and primitive, three passes for two primitives) */
} ud_mpm_conf;

/* material, hardness: host arrays [n_particles] (SimpleMPMSimulator.material / .h, mpm_simulator.py:117-122) */
int ud_mpm_create(const ud_mpm_conf* conf, const int* material, const float* hardness, ud_mpm** out);
void ud_mpm_destroy(ud_mpm* h);
/* bytes of the checkpoint one ud_mpm_step_fwd call with B envs writes for its backward: the particle state of every substep; on
 * the many-workgroup path also the primitive rows, the spatial order, the grid-checkpoint pool and -- while B * n_particles is
 * below 100 000 (the regime where a launch waits for one wave's serial chain) -- the SVD factors of every substep's F, which
 * the backward reads instead of iterating again; with grid_ckpt_cells > 0 also one int per env beside the pool's record index, which the
 * forward sets to non-zero exactly when it raises bit 0 of that env's status[] (the forward initialises it: the checkpoint may be
 * uninitialised memory).  The layout is the library's; the same B must be passed to the backward */
size_t ud_mpm_ckpt_bytes(const ud_mpm* h, int B);
/* Which kernels a call with B envs runs (the choice is the library's, by measurement: DESIGN.md 3.2); for logs and benchmark
 * labels, nothing at this boundary depends on it.  0: one workgroup per env (bodies up to 128 particles, one box primitive).
 * Bit 0: the many-workgroup path.  Bit 1: its forward is one persistent launch per group of envs (several workgroups per
 * env that hand grid cells to each other through HBM), else four launches per substep.  Bit 2: its backward, restoring
 * the grid from the checkpoint (grid_ckpt_cells > 0), takes two launches per substep, else four (six when it recomputes).
 * Negative: bad arguments. */
int ud_mpm_launch_plan(const ud_mpm* h, int B);
/* Measurement aid (bench.py's algorithmic-byte count, tools/traffic_table.py): cells[b] = the number of grid-checkpoint records env b's forward
 * left in `ckpt` = its active grid cells summed over the substeps of that step call (SURVEY 8(d)'s G_act, per substep, is cells[b] / substeps).
 * `cells`: device array of B ints, written asynchronously on `stream`.  Handles without a grid checkpoint (one workgroup per env,
 * grid_ckpt_cells = 0, deterministic mode) write 0.  Same B as the forward that wrote `ckpt`. */
int ud_mpm_ckpt_cells(const ud_mpm* h, int B, const void* ckpt, int* cells, void* stream);
/* Puts every handle-owned arena back into its rest state, asynchronously on `stream` (no host synchronisation).  For the one case in which
 * a step call can leave them dirty: status bit 4 of the persistent forward (a workgroup gave up waiting for its siblings and skipped
 * the zeroing of its cells).  Until then later calls on the handle would sum into stale cells.  The Python mirror calls it when its
 * status check sees that bit.  The persistent forward needs every workgroup of a launch resident at once (launch size = occupancy x CUs
 * of an otherwise idle device): kernels of other streams or processes that occupy CUs for seconds are what can cause such a time-out. */
int ud_mpm_reset(ud_mpm* h, void* stream);

/* Forward `step`: state (x,v [B,N,3]; C,F [B,N,3,3]; J [B,N]), primitive 0 (position [B,steps,3], rotation
 * [B,steps,4] (w,x,y,z), size [B,3]), friction/mu/lamda [B], action [B,6] -> new state, primitive position /
 * rotation after copy_frame(steps,0) and the v,w [B,steps,3] written by set_action.
 * ckpt (may be NULL = no backward): ud_mpm_ckpt_bytes() bytes. status [B] int32, written asynchronously, the caller reads
 * it when it next synchronises: 0 ok.  One-workgroup path: 1 = LDS cell table overflow in that env (outputs invalid).
 * Many-workgroup path, a bit mask: 1 = the grid checkpoint of that env is incomplete -- its pool ran out, or (persistent forward) a
 * part of 32 particles touched more cells than its 512-slot table holds and sent the rest to the HBM grid directly (outputs valid; that
 * step's backward must recompute the grid for that env: clip bit 2 of ud_mpm_step_bwd lets the backward see the same fact in the
 * checkpoint and decide per env on the device; clip bit 1 forces it for every env); 2 = a part's spill list overflowed as well (more than 896
 * cells for 32 particles: cannot happen with a 27-cell stencil; outputs invalid); 4 = a workgroup gave up waiting for a sibling
 * (outputs invalid; call ud_mpm_reset before the next step). */
int ud_mpm_step_fwd(ud_mpm* h, int B, const float* x, const float* v, const float* C, const float* F, const float* J,
                    const float* prim_position, const float* prim_rotation, const float* prim_size,
                    const float* friction, const float* mu, const float* lamda, const float* action, float* x_out,
                    float* v_out, float* C_out, float* F_out, float* J_out, float* prim_position_out,
                    float* prim_rotation_out, float* prim_v_out, float* prim_w_out, void* ckpt, int* status,
                    void* stream);

/* Backward `step`: cotangents of (x,v,C,F, primitive position, primitive rotation) at the step output ->
 * cotangents at the step input plus friction/mu/lamda [B] and action [B,6].  J receives no gradient (excluded
 * from the reference's substep loss, mpm_simulator.py:343-350).  g_prim_rotation (in) and g_prim_rotation0 (out)
 * [B,steps,4] may be NULL (= zero cotangent / not wanted).
 * Position control: nothing reaches the rotation array (g_prim_rotation0 = 0) and action[3:6] is reported as 0 --
 * the reference yields NaN there for w = 0 and launders it with nan_to_num at this boundary.
 * Soft contact: rotation and action[3:6] carry the chain rule as the reference writes it, NaN at w = 0 included
 * (d|w|/dw, primitives.py:86); clip != 0 launders it exactly like the reference.
 * clip bit 0 applies norm_grad_state / norm_grad (nan_to_num + global-norm clip to 1, :389-408); in soft-contact
 * mode the norm also covers the cotangents of the primitive's rotation, size, friction and action_scale leaves.
 * clip bit 1 (many-workgroup path with grid_ckpt_cells > 0): ignore the grid checkpoint and recompute p2g + grid op --
 * for a step whose forward flagged a pool overflow in status[]; the particle history in the checkpoint is always complete.
 * clip bit 2 (value 4; same handles): decide per env, on the device, from the word the forward left in the checkpoint -- every env whose
 * word is clear restores its grid from the checkpoint, every env whose word is set recomputes p2g + grid op, in this same call.  The
 * host reads nothing: a forward / backward pair needs no host code between its two calls (clip = 1 | 4 is the whole binding, under
 * jit or inside a captured graph too).  Bit 1 wins over bit 2 (every env recomputes).  Bit 2 is ignored where there is no grid
 * checkpoint to choose from: the one-workgroup path, grid_ckpt_cells = 0, deterministic mode.
 * status [B] int32 of the backward: 0 ok; deterministic mode: 1 = more than 32768 touched cells in that env; under clip bit 2, value 8 =
 * the grid of that env was recomputed (a report, not an error). */
int ud_mpm_step_bwd(ud_mpm* h, int B, const void* ckpt, const float* prim_size, const float* friction,
                    const float* mu, const float* lamda, const float* action, const float* g_x, const float* g_v,
                    const float* g_C, const float* g_F, const float* g_prim_position, const float* g_prim_rotation, int clip,
                    float* g_x0, float* g_v0, float* g_C0, float* g_F0, float* g_prim_position0, float* g_prim_rotation0,
                    float* g_friction, float* g_mu, float* g_lamda, float* g_action, int* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PlasticineLab-style MLS-MPM, float64, von-Mises plasticity, sticky Sphere and Capsule primitives (GenORM Torus task,
 * BASELINE config 5; PlasticineLab sim2sim Writer) -- replaces TaichiEnv.step -> MPMSimulator.step(is_copy=True) = `substeps` x substep
 *   GenORM/policy/pbm/plb/engine/mpm_simulator.py:438-449 (step), :256-268 (substep: clear_grid, compute_F_tmp,
 *   svd, p2g :166-195 with compute_von_mises :133-150, forward_kinematics, grid_op :200-232, g2p :234-253),
 *   engine/primitive/primitives.py:17-53 (Sphere), engine/primitive/primive_base.py:118-121,185-192.
 * Adjoint (ud_plb_step_bwd): substep_grad :271-289 with backward_svd :107-124; the differentiable leaves are the particle
 * state, primitive 0's action and position, and per env E, nu, yield_stress (PlasticineLab/sim2sim/plb/engine/
 * mpm_simulator.py:27-29,485-498: get_parameter_grad) and the ground friction (optimize_ground_friction, :57-58).
 * Losses (ud_plb_loss_*): engine/losses/loss.py:112-243 (density, SDF, soft / hard contact, weighted sum).
 * Primitive kinds (prim_kind).  0, the sticky Sphere (primitives.py:17-53): a cell within the soft shell takes the collider's
 * velocity.  1, the Capsule (primitives.py:55-73) with the base class's contact model (primive_base.py:57-115): the cell g is
 * taken into the primitive's frame (p = qrot(conj(q) / |q|, g - P_f), p.y += h / 2, p.y -= clamp(p.y, 0, h)); dist =
 * sqrt(p.p + 1e-14) - r, normal D = qrot(q, p / sqrt(p.p + 1e-14)), influence = min(exp(-dist softness), 1); the cell is active
 * when (softness > 0 and influence > 0.1) or dist <= 0; an active cell's velocity u becomes cv + w (1 - influence) + t' influence
 * with cv the collider velocity, w = u - cv, t = w - min(w.D, 0) D and t' = t / |t| max(0, |t| + (w.D) prim_friction) where
 * w.D < 0 (|t| = sqrt(t.t + 1e-8)).  Its adjoint holds the two branch decisions constant and reaches u, P_f (through p, dist,
 * D, influence, cv) and P_{f+1}; orientation, height, radius, friction and softness are not leaves.  The contact loss takes the
 * Capsule's distance.  Without rot_state the orientation is a handle constant (three action dimensions per actuated primitive).
 * A handle with a Capsule, or with an action_scale other than (1, 1, 1), runs the multi-kernel path only.
 * 3 Box, 4 Cylinder, 5 Torus (primitives.py:241-269, 176-202, 211-231): the same contact model, with the kind's own _sdf / _normal of the
 * local point pl in place of the Capsule's; length(x) = sqrt(x.x + 1e-14) everywhere.  Box (prim_shape = size, three half extents):
 * q = |pl| - size, sdf = length(max(q, 0)) + min(max(q0, q1, q2), 0); the normal is the reference's central difference of that sdf,
 * n_i = (0.5 / d)(sdf(pl + d e_i) - sdf(pl - d e_i)) with d = 1e-4, normalised -- not an analytic normal.  Cylinder (prim_shape = (h, r):
 * h the radial half extent, r the axial one): d = (length((pl.x, pl.z)) - h, |pl.y| - r), sdf = min(max(d0, d1), 0) + length(max(d, 0)),
 * normal from n2 = max(d, 0) + [max(d0, d1) <= 0] ([d0 > d1], 1 - [d0 > d1]) normalised, spread over (pl.x, pl.z) / l and the sign
 * [pl.y >= 0] 2 - 1, normalised again.  Torus (prim_shape = (tx, ty)): q = (length((pl.x, pl.z)) - tx, pl.y), sdf = length(q) - ty,
 * normal (x / l q0 / |q|, q1 / |q|, z / l q0 / |q|) normalised.  Their adjoints hold indicators, signs and the arm abs / min / max took
 * constant (sub-gradients at ties are unspecified); the Box normal's adjoint is the exact derivative of the finite-difference formula (the
 * analytic sdf gradient at the six sample points), not that of a true box normal.  Shape constants are not leaves.  Such a handle runs
 * kernels of its own on the multi-kernel path; a Capsule may sit beside a new shape.  Specification: tests/plb_shape_twin.py.
 * Rotating primitives (rot_state; the *_rot entry points).  Every primitive carries a rotation (w, x, y, z) beside its position, as the
 * reference's Primitive does (primive_base.py:31-38), turned once per substep (:117-121):
 *   a = clip(action, -1, 1) (its cotangent passes at equality and is zero outside);
 *   kinds 0 and 1:  v = a[0:3] action_scale / substeps, w = a[3:6] action_scale_w / substeps (0 with three action dimensions and for
 *     an unactuated primitive 1; an actuated one: "Two actuated primitives" below);  pos[f+1] = clamp(pos[f] + v, lower_bound, upper_bound);  rot[f+1] = qmul(w2quat(w), rot[f]);
 *   kind 2, the RollingPin (primitives.py:83-99; the Capsule's geometry and contact):  (dw, dth, dy) = a action_scale / substeps;
 *     y_dir = qrot(rot[f], (0, -1, 0));  x_dir = cross((0, 1, 0), y_dir) dw 0.03, x_dir.y = dy;  pos[f+1] = clamp(pos[f] + x_dir);
 *     rot[f+1] = qmul(w2quat((0, -dth, 0)), qmul(rot[f], w2quat((0, dw, 0)))) -- the position step depends on the rotation.
 *   qmul (utils.py:19-27) is the Hamilton product, normalised: rot[f >= 1] is unit, rot[0] is used as given.  w2quat (utils.py:29-41)
 *   is (cos(|w|/2), w/|w| sin(|w|/2)), and the identity when |w| <= 1e-9; on that arm the cotangent of w is DEFINED as 0 (taichi's reverse
 *   mode would form 0 * inf there).  The contact at substep f is the Capsule's above with q = rot[f] (distance, normal, conj(q) / |q|) and
 *   rot[f+1] in the collider velocity (primive_base.py:82-89); its adjoint also reaches rot[f] (through the inverse with its
 *   normalisation, the local point and the normal's rotation back) and rot[f+1].  The reference asserts |q| > 0.9 (inv_trans); on the
 *   device this is the CALLER'S duty: prim_rot is not checked.  Specification: tests/plb_rot_twin.py.
 * 6 Chopsticks (primitives.py:102-173; the *_gap entry points): two Capsules of (capsule_h, radius) = (h, r) side by side, the one kind whose
 * SHAPE is state.  Beside position and rotation it carries its opening `gap` (the reference's state_dim = 8), which closes once per substep:
 *   a = clip(action, -1, 1), seven dimensions;  v = a[0:3] action_scale / substeps, w = a[3:6] action_scale_w / substeps, gap_vel = a[6]
 *     action_scale_gap / substeps;
 *   gap[f+1] = max(gap[f] - gap_vel, min_gap);  pos[f+1] = clamp(pos[f] + v, lower_bound, upper_bound);  rot[f+1] = qmul(rot[f], w2quat(w)):
 *     a RIGHT multiplication (a turn about the body's own axes), where the base class multiplies on the left.
 *   Geometry at substep f, for the local point pl = qrot(conj(q) / |q|, g - P_f): p = pl + (0, h/2, 0), delta = (gap[f] / 2, 0, 0), a =
 *   capsule_sdf(p - delta), b = capsule_sdf(p + delta) with capsule_sdf the Capsule's above, which shifts y by h/2 AGAIN before it takes off
 *   clamp(y, 0, h): each stick's axis segment spans local y in [-h, 0] at x = -+gap/2 -- the primitive's position is the TOP END of the sticks, not
 *   their middle (this doubled h/2 offset is the reference's, kept to the letter).  sdf = min(a, b); the local normal is the Capsule's normal of
 *   stick a where a <= b (a tie takes stick a for both) and of stick b otherwise.  World normal, contact model and collider velocity are the
 *   base class's, unchanged: the sticks' closing motion is NOT part of the collider velocity.
 *   Adjoint: the selected stick and the arms of clamp / max are held constant.  gap[f] is a leaf of the contact at substep f: it enters through
 *   -+delta in the selected stick's local point, so its cotangent is -+1/2 of the x-component of that point's cotangent (distance and normal).
 *   Through max(gap - gap_vel, min_gap) the cotangent passes to gap[f] and -gap_vel where gap[f] - gap_vel > min_gap and is zero where it is
 *   smaller; at exact equality it is UNSPECIFIED.  The right-multiplied step has its own adjoint; w's cotangent on the |w| <= 1e-9 arm is 0 as
 *   above.  h, r, min_gap and the scales are not leaves.  Only primitive 0 can be a Chopsticks, on rot_state with action_dim = 7; primitive 1 is
 *   a sticky Sphere that never moves or, with action_dim1 != 0, an actuated kind 0, 1, 3, 4 or 5 as on every rot_state handle; its gap entry is
 *   carried along unchanged.  Multi-kernel path only.
 *   Specification: tests/plb_chopsticks_twin.py (the reference ships no chopsticks.yml and no recording).
 * Two actuated primitives (action_dim1 != 0; engine/primitive/primitives.py:280-319: Primitives gives every primitive its own action.dim and slices
 * one flat action vector by the running offsets action_dims, set_action :307-311; get_grad concatenates the per-primitive gradients, :313-319).
 *   A0 = what primitive 0 takes (3, or action_dim: 6, the Chopsticks' 7), A = A0 + action_dim1.  On all three entry-point families (plain, _rot,
 *   _gap) action and g_action are [B, A]: primitive 0's block in columns 0 .. A0 - 1, exactly as without the field, primitive 1's in columns
 *   A0 .. A - 1.  a = clip(action, -1, 1) per component over the whole row (its cotangent passes at equality and is zero outside).
 *   Primitive 1 ALWAYS follows the base class, also beside a RollingPin or a Chopsticks: v = a1[0:3] action_scale1 / substeps, w = a1[3:6]
 *   action_scale_w1 / substeps (0 with action_dim1 = 3);  pos[f+1] = clamp(pos[f] + v, lower_bound, upper_bound);  rot[f+1] = qmul(w2quat(w),
 *   rot[f]) (left multiplication; the |w| <= 1e-9 arm sends the cotangent 0 to w, as for primitive 0).
 *   With action_dim1 != 0 primitive 1 of a rot_state handle may be kind 0, 1, 3, 4 or 5 (its rotation is read by the contact and the loss and is
 *   a leaf of both); without rot_state it may be what it may be with action_dim1 = 0.  RollingPin (2) and Chopsticks (6) stay primitive 0 only.
 *   A Sphere + Sphere handle with action_dim1 = 3 and both unit scales runs the persistent path; any other such handle the multi-kernel path.
 *   The checkpoint layout does not change: the trajectories already carry a primitive axis.  Specification: tests/plb_multi_twin.py (the
 *   reference ships no two-handed task).
 * Parity for these entry points is UNPINNED: taichi is absent and the reference ships no recording of this path; the torch
 * restatements (oracle/twin/plb_twin_torch.py, tests/plb_prim_twin.py for the Capsule) are the specification the kernels are held to.
 * ------------------------------------------------------------------------------------------------ */
typedef struct ud_plb ud_plb;

typedef struct {
  int n_particles;
  int n_grid;            /* int(128 * quality * 0.5)                  mpm_simulator.py:14-18 */
  int substeps;          /* int(2e-3 // dt)                           :32 */
  double dt;             /* 0.5e-4 / (quality * 0.5)                  :21 */
  double gravity[3];     /* SIMULATOR.gravity (the kernel applies x30, :205) */
  double ground_friction;
  int n_primitives;      /* 1 or 2 primitives (Spheres unless prim_kind says otherwise); primitive 0 is actuated (3 action dims, or action_dim),
                            primitive 1 only with action_dim1 below */
  double radius[2];
  double lower_bound[3], upper_bound[3];   /* primitive xyz_limit */
  int grid_ckpt_cells;   /* 0: ud_plb_step_bwd runs p2g again for every substep (substep_grad recomputes the whole substep,
                            mpm_simulator.py:271-289).  K > 0: a forward with a checkpoint also keeps the touched grid cells
                            (index, m, mv: 36 B each; up to min(27, K) * n_particles per substep, inside the caller's checkpoint:
                            ud_plb_ckpt_bytes grows accordingly) and the backward restores them; a substep that touched more
                            cells than that falls back to recomputing, per env, on the device.  K >= 27 can never fall back.
                            Multi-kernel path only (the persistent path always keeps its parts' cells: ud_plb_ckpt_bytes says what a
                            checkpoint takes) */
  int max_envs;          /* the largest B any call on this handle will pass (>= 1).  Every arena -- exchange grids, active lists, adjoint
                            and loss scratch -- is allocated in ud_plb_create for this many envs; no step or loss call allocates or
                            synchronises the host; a call with B > max_envs returns UD_ERR_INVALID */
  int path;              /* which kernels the handle runs, fixed at create (ud_plb_launch_plan reports it).  0: the library's choice --
                            ONE persistent launch per step call and direction (csrc/plb_cluster.hip: parts of 32 particles, one
                            workgroup each, the particle state in registers, the grid exchanged through HBM once per substep) where
                            every workgroup of a launch can be resident and the exchange grids fit (bodies up to ~8 000 particles per
                            env), else the multi-kernel path (2 launches per forward substep, 5 per reverse one).  1: the multi-kernel
                            path.  2: the persistent path (UD_ERR_UNSUPPORTED where it cannot run) */
  int lanes;             /* multi-kernel path: lanes per particle in the particle kernels.  0: by launch size (8 up to 16 000 particles
                            per launch, 4 below 100 000, 1 beyond); 1 / 4 / 8 force one mapping (how the tests put all three before
                            the restatement at their sizes) */
  int sort_every;        /* the handle orders each env's particles by grid cell internally (invisible at this boundary) on the first
                            call and every sort_every-th forward call after it; 0 = 8; negative = never */
  /* Everything below: zero = the handle of before these fields existed (sticky Spheres, action scale 1) */
  int prim_kind[2];      /* 0 sticky Sphere, 1 Capsule (radius[i], capsule_h[i], prim_rot[i], prim_friction[i]), 2 RollingPin (the Capsule's
                            geometry, its own kinematics; needs rot_state and three action dimensions), 3 Box, 4 Cylinder, 5 Torus
                            (prim_shape[i], prim_rot[i], prim_friction[i]; radius[i] and capsule_h[i] are ignored), 6 Chopsticks (radius[i],
                            capsule_h[i], prim_friction[i], min_gap[i]; prim_shape ignored; primitive 0 only, needs rot_state and
                            action_dim = 7: UD_ERR_INVALID without); else UD_ERR_INVALID.
                            A handle with any kind but 0 runs the multi-kernel path (path = 0 picks it; path = 2: UD_ERR_UNSUPPORTED) */
  double capsule_h[2];   /* Capsule: length of the axis segment (along the primitive's y), >= 0; radius[i] > 0 */
  double prim_rot[2][4]; /* Capsule: constant orientation (w, x, y, z); all four zero = identity, else |q| > 0.9 as the reference asserts */
  double prim_friction[2];   /* Capsule: Coulomb friction of the contact (primitive cfg.friction) */
  double action_scale[3];    /* primitive 0: v = clip(action, -1, 1) * action_scale / substeps (set_velocity); all zero = (1, 1, 1).  Any
                                other value: multi-kernel path, as with a Capsule */
  int rot_state;             /* nonzero: every primitive's orientation is per-env state, passed through the *_rot entry points (prim_rot above is
                                then unused by the kernels).  Primitive 0 must be kind 1 to 6; primitive 1 a sticky Sphere that never moves or,
                                with action_dim1 != 0, an actuated kind 0, 1, 3, 4 or 5: anything else, and path = 2, UD_ERR_UNSUPPORTED */
  int action_dim;            /* 0 or 3: three action dimensions.  6: (v, w) of the base class (set_velocity, primive_base.py:185-193); needs
                                rot_state (UD_ERR_INVALID without).  7: the Chopsticks' (v, w, gap_vel); UD_ERR_INVALID with any other kind */
  double action_scale_w[3];  /* action.scale[3:6]: w = clip(action[3:6], -1, 1) * action_scale_w / substeps; all zero = (1, 1, 1) */
  double prim_shape[2][3];   /* kinds 3 to 5: Box size (three half extents), Cylinder (h, r, -), Torus (tx, ty, -); a used constant <= 0 is
                                UD_ERR_INVALID.  Kinds 0 to 2 ignore it (zero = the handle of before) */
  double min_gap[2];         /* kind 6: Chopsticks.minimal_gap, >= 0 (the reference's default: 0.06); other kinds ignore it */
  double action_scale_gap;   /* kind 6: action.scale[6], gap_vel = clip(action[6], -1, 1) * action_scale_gap / substeps; 0 = 1 */
  int action_dim1;           /* primitive 1's action block, behind primitive 0's A0 columns (see "Two actuated primitives" above).  0: primitive 1
                                is unactuated, the handle of before in every respect.  3: it takes v.  6: (v, w) of the base class; needs
                                rot_state.  Anything else, 6 without rot_state, or nonzero with n_primitives < 2: UD_ERR_INVALID */
  double action_scale1[3];   /* primitive 1: v = clip(action[A0:A0+3], -1, 1) * action_scale1 / substeps; all zero = (1, 1, 1).  Any other
                                value: multi-kernel path */
  double action_scale_w1[3]; /* primitive 1: w = clip(action[A0+3:A0+6], -1, 1) * action_scale_w1 / substeps; all zero = (1, 1, 1) */
} ud_plb_conf;

int ud_plb_create(const ud_plb_conf* conf, ud_plb** out);
void ud_plb_destroy(ud_plb* h);
/* 1: the multi-kernel path, 2: the persistent path (one launch per step call and direction); negative: bad arguments (B > max_envs) */
int ud_plb_launch_plan(const ud_plb* h, int B);
/* Persistent path only: a workgroup that waits for a sibling longer than ~seconds gives up, its env's outputs are NaN and a device-side
 * counter is raised.  This call SYNCHRONISES `stream`, returns the number of such workgroups since the previous call (0 = none, also on
 * the multi-kernel path; ud_last_error() holds the text otherwise) and, when it is not 0, puts the handle's exchange arena back into its
 * rest state so that later calls are valid again.  The step calls themselves stay asynchronous and return UD_OK.  Between a time-out
 * and the poll that clears it the handle is POISONED: every persistent launch sees the raised counter at entry, touches neither barrier
 * words nor exchange grids and writes NaN to all its outputs -- a time-out can never turn into finite-but-wrong results of later steps. */
int ud_plb_poll_timeouts(ud_plb* h, void* stream);
/* One env.step for B independent envs (float64 device arrays): x, v [B,N,3]; C, F [B,N,3,3]; prim_pos
 * [B,n_primitives,3]; softness [B,n_primitives]; action [B,A] (A = 3 + action_dim1: "Two actuated primitives" above); E, nu, yield_stress [B]. */
int ud_plb_step_fwd(ud_plb* h, int B, const double* x, const double* v, const double* C, const double* F,
                    const double* prim_pos, const double* softness, const double* action, const double* E,
                    const double* nu, const double* yield_stress, double* x_out, double* v_out, double* C_out,
                    double* F_out, double* prim_pos_out, void* ckpt, void* stream);
/* ckpt (may be NULL = no backward): ud_plb_ckpt_bytes(h, B) bytes, caller-owned, opaque: every substep's particle state,
 * the primitive trajectory and the internal spatial order of this call, consumed by ud_plb_step_bwd. */
size_t ud_plb_ckpt_bytes(const ud_plb* h, int B);
/* The same on a rot_state handle (UD_ERR_INVALID on any other; ud_plb_step_fwd / _bwd / ud_plb_loss_* return UD_ERR_INVALID on a
 * rot_state handle): prim_rot [B,n_primitives,4] (w, x, y, z; |q| > 0.9 is the caller's duty), action [B,A] (A = action_dim + action_dim1), prim_rot_out
 * [B,n_primitives,4].  The checkpoint (ud_plb_ckpt_bytes) also keeps the rotation trajectory.  Launches only: no allocation, no
 * synchronisation. */
int ud_plb_step_fwd_rot(ud_plb* h, int B, const double* x, const double* v, const double* C, const double* F,
                        const double* prim_pos, const double* prim_rot, const double* softness, const double* action,
                        const double* E, const double* nu, const double* yield_stress, double* x_out, double* v_out,
                        double* C_out, double* F_out, double* prim_pos_out, double* prim_rot_out, void* ckpt, void* stream);

/* The same on a Chopsticks handle (prim_kind[0] = 6; UD_ERR_INVALID on any other, and ud_plb_step_fwd / _fwd_rot and their siblings return
 * UD_ERR_INVALID on a Chopsticks handle, touch no output and name the reason): prim_gap [B,n_primitives] (primitive 1's entry is carried
 * through), action [B,A] (A = 7 + action_dim1), prim_gap_out [B,n_primitives].  The checkpoint also keeps the gap trajectory (ud_plb_ckpt_bytes grows for such
 * handles only).  Launches only: no allocation, no synchronisation; graph-capturable like its siblings. */
int ud_plb_step_fwd_gap(ud_plb* h, int B, const double* x, const double* v, const double* C, const double* F,
                        const double* prim_pos, const double* prim_rot, const double* prim_gap, const double* softness,
                        const double* action, const double* E, const double* nu, const double* yield_stress, double* x_out,
                        double* v_out, double* C_out, double* F_out, double* prim_pos_out, double* prim_rot_out,
                        double* prim_gap_out, void* ckpt, void* stream);

/* Adjoint of one env.step.  g_x, g_v [B,N,3], g_C, g_F [B,N,3,3], g_prim_pos [B,n_primitives,3]: cotangents of the
 * step's outputs (any may be NULL = zero).  Outputs: cotangents of the inputs x, v, C, F (required), of prim_pos
 * [B,n_primitives,3], of action [B,A] (both blocks), and per env of E, nu, yield_stress and the ground friction [B] (each may be NULL).
 * softness, action, E, nu, yield_stress: the forward call's inputs again. */
int ud_plb_step_bwd(ud_plb* h, int B, const void* ckpt, const double* softness, const double* action, const double* E,
                    const double* nu, const double* yield_stress, const double* g_x, const double* g_v, const double* g_C,
                    const double* g_F, const double* g_prim_pos, double* g_x0, double* g_v0, double* g_C0, double* g_F0,
                    double* g_prim_pos0, double* g_action, double* g_E, double* g_nu, double* g_yield_stress,
                    double* g_ground_friction, void* stream);
/* ... of ud_plb_step_fwd_rot: g_prim_rot [B,n_primitives,4] (in, may be NULL = zero), g_prim_rot0 [B,n_primitives,4] (out, may be
 * NULL), g_action [B,A]. */
int ud_plb_step_bwd_rot(ud_plb* h, int B, const void* ckpt, const double* softness, const double* action, const double* E,
                        const double* nu, const double* yield_stress, const double* g_x, const double* g_v, const double* g_C,
                        const double* g_F, const double* g_prim_pos, const double* g_prim_rot, double* g_x0, double* g_v0,
                        double* g_C0, double* g_F0, double* g_prim_pos0, double* g_prim_rot0, double* g_action, double* g_E,
                        double* g_nu, double* g_yield_stress, double* g_ground_friction, void* stream);
/* ... of ud_plb_step_fwd_gap: also g_prim_gap [B,n_primitives] (in, may be NULL = zero), g_prim_gap0 [B,n_primitives] (out, may be NULL),
 * g_action [B,A]. */
int ud_plb_step_bwd_gap(ud_plb* h, int B, const void* ckpt, const double* softness, const double* action, const double* E,
                        const double* nu, const double* yield_stress, const double* g_x, const double* g_v, const double* g_C,
                        const double* g_F, const double* g_prim_pos, const double* g_prim_rot, const double* g_prim_gap, double* g_x0,
                        double* g_v0, double* g_C0, double* g_F0, double* g_prim_pos0, double* g_prim_rot0, double* g_prim_gap0,
                        double* g_action, double* g_E, double* g_nu, double* g_yield_stress, double* g_ground_friction, void* stream);

/* Loss of a particle state (engine/losses/loss.py): x [B,N,3], prim_pos [B,n_primitives,3], target_density and target_sdf
 * [n_grid^3] (shared by the envs), weights [3] = (contact, density, sdf) -- all device arrays.
 *   density = sum_I |grid_mass_I - target_density_I|, sdf = sum_I target_sdf_I grid_mass_I  with grid_mass = the p2g of the
 *   particle masses (compute_grid_m_kernel); contact = sum_primitives min_dist^2 with, soft_contact != 0: min_dist =
 *   sum_i d_i w(d_i) / sum_i w(d_i), w(d) = 1 / (1 + 1e4 d^2), d_i = max(sdf(x_i), 0); soft_contact == 0: min_i d_i.
 * loss [B] = weights . (contact, density, sdf); parts [B,3] (may be NULL) = the three terms.
 * ud_plb_loss_bwd: g_loss [B] -> g_x [B,N,3], g_prim_pos [B,n_primitives,3] (may be NULL). */
int ud_plb_loss_fwd(ud_plb* h, int B, const double* x, const double* prim_pos, const double* target_density,
                    const double* target_sdf, const double* weights, int soft_contact, double* loss, double* parts, void* stream);
int ud_plb_loss_bwd(ud_plb* h, int B, const double* x, const double* prim_pos, const double* target_density,
                    const double* target_sdf, const double* weights, int soft_contact, const double* g_loss, double* g_x,
                    double* g_prim_pos, void* stream);
/* The same on a rot_state handle: the contact term takes the Capsule's distance in the primitive's current frame prim_rot
 * [B,n_primitives,4]; g_prim_rot [B,n_primitives,4] (out, may be NULL). */
int ud_plb_loss_fwd_rot(ud_plb* h, int B, const double* x, const double* prim_pos, const double* prim_rot, const double* target_density,
                        const double* target_sdf, const double* weights, int soft_contact, double* loss, double* parts, void* stream);
int ud_plb_loss_bwd_rot(ud_plb* h, int B, const double* x, const double* prim_pos, const double* prim_rot, const double* target_density,
                        const double* target_sdf, const double* weights, int soft_contact, const double* g_loss, double* g_x,
                        double* g_prim_pos, double* g_prim_rot, void* stream);
/* The same on a Chopsticks handle: the contact term takes the Chopsticks' distance at the caller's current gap prim_gap [B,n_primitives];
 * g_prim_gap [B,n_primitives] (out, may be NULL). */
int ud_plb_loss_fwd_gap(ud_plb* h, int B, const double* x, const double* prim_pos, const double* prim_rot, const double* prim_gap,
                        const double* target_density, const double* target_sdf, const double* weights, int soft_contact, double* loss,
                        double* parts, void* stream);
int ud_plb_loss_bwd_gap(ud_plb* h, int B, const double* x, const double* prim_pos, const double* prim_rot, const double* prim_gap,
                        const double* target_density, const double* target_sdf, const double* weights, int soft_contact,
                        const double* g_loss, double* g_x, double* g_prim_pos, double* g_prim_rot, double* g_prim_gap, void* stream);

/* Grid mass of a particle state, the field a goal is made of (TaichiEnv.get_grid_mass; create_goal1.py saves it as the target
 * density): grid_mass [B, n_grid^3] = the loss's p2g of the particle masses, written into the caller's array (zeroed here, summed with
 * atomics).  Any handle kind and path; B is not bound by max_envs: the call reads the handle's constants only and touches none of its
 * arenas, so it may run next to a loss call of the same handle on another stream.  Per axis base = (int)(x inv_dx - 0.5), truncated
 * toward zero, and each of the three stencil indices is clamped on its own, min(max(base + o, 0), n_grid - 1): a particle near or
 * outside a wall adds several of its 27 terms to one wall cell, and the total mass is N p_mass wherever the particles are. */
int ud_plb_grid_mass(ud_plb* h, int B, const double* x, double* grid_mass, void* stream);

/* Target SDF of T target densities (Loss.update_target / update_target_sdf, engine/losses/loss.py:77-106), handle-free: launches only,
 * no allocation, no synchronisation, capturable in a HIP graph.  G = n_grid^3, cell (i,j,k) at (i n + j) n + k; density, sdf [T,G].
 * State per cell: S (distance, 1000 = none yet) and P (the occupied cell nearest so far); S_c = 1000 everywhere at the start.  One
 * sweep, for every cell I from the copies (S_c, P_c) of the previous sweep:
 *   density[I] > threshold: S = 0, P = I;
 *   otherwise S = 1000, then for every offset o in {-3..2}^3 without 0, lexicographic with ox slowest, v = I + o inside the grid and
 *   S_c[v] < 1000:  d = sqrt(dx^2 + dy^2 + dz^2 + 1e-8) of x_I - x_{P_c[v]} with x_J = J * (1 / n_grid), summed left to right;
 *   d < S (strict): S = d, P = P_c[v].
 * The window is asymmetric (3 cells down, 2 up), the first minimal candidate in offset order wins, and a cell is recomputed in every
 * sweep.  sweeps = 0 runs the reference's 2 n_grid sweeps, sweeps = k exactly k.  One launch per sweep, all enqueued; a launch whose
 * predecessor changed no cell of its target returns at entry (a fixed point of a deterministic map stays one), so the outputs are those
 * of all the sweeps: sdf = S; nearest [T,G] (may be NULL) = linear index of P, -1 where S = 1000; sweeps_run [T] (device, may be NULL) =
 * the number of sweeps that did work for that target = min(sweeps, 1-based number of the first sweep that changed nothing).
 * work: ud_plb_target_work_bytes(n_grid, T) bytes (two int32 states per cell + one word per target; 0 for sizes the call rejects).
 * n_grid < 1, T < 1, sweeps < 0, null density / sdf / work: UD_ERR_INVALID; n_grid > 1024 (P is packed into 3 x 10 bits) or
 * T > 65535: UD_ERR_UNSUPPORTED.  Results are bit-identical from run to run. */
size_t ud_plb_target_work_bytes(int n_grid, int T);
int ud_plb_target_sdf(int n_grid, int T, const double* density, double threshold, int sweeps, double* sdf, int* nearest,
                      int* sweeps_run, void* work, void* stream);

/* Soft IoU of densities (iou_kernel, loss.py:239-254): a [T,G]; b [T,G] (b_batched != 0) or [G] shared by all t; iou [T].
 *   ma = max(0, max a), mb = max(0, max b), I = sum(a b) / ma / mb, U = sum(a) / ma + sum(b) / mb, iou = I / (U - I).
 * Every sum runs in a fixed order (two stages of binary trees): the same input gives the same bits.  ma = 0 or mb = 0 is not
 * special-cased: the result is what IEEE gives (0 / 0 = NaN).  work: ud_plb_density_iou_work_bytes(T) bytes.  Launches only. */
size_t ud_plb_density_iou_work_bytes(int T);
int ud_plb_density_iou(long G, int T, const double* a, const double* b, int b_batched, double* iou, void* work, void* stream);

/* System identification (PlasticineLab sim2sim / real2sim: optimizer/solver.py, engine/losses/loss.py new_target_density[f]):
 * the density loss of a SEQUENCE of particle clouds, each against a target of its own, with its adjoint (csrc/plb_sysid.hip).
 * An item is one cloud; the M items are any flattening of frames x envs.  Like ud_plb_grid_mass the calls read the handle's constants
 * only and touch none of its arenas: M is not bound by max_envs, any handle kind and path.  Launches only: no allocation, no
 * synchronisation, capturable in a HIP graph; no workgroup waits for another one.  G = n_grid^3.
 *   x [M,N,3]; targets [T,G]; target_index [M] (device int32; NULL = target 0 for every item); loss [M]:
 *   loss[m] = sum_I |gm_I(x_m) - targets[target_index[m], I]|, gm = the mass p2g of ud_plb_loss_fwd / ud_plb_grid_mass (same weights,
 *   same clamping of the cell indices into the grid).
 * The forward works in chunks of work_bytes / (8 G) items: a chunk's masses are scattered with f64 atomics into `work` (zeroed by a
 * kernel), then one sweep per chunk reads gm and the target, reduces |df| per item, records sign(df) and leaves the scratch zero for
 * the next chunk.  The result does not depend on the chunking beyond the order of the atomic sums.  work_bytes below one item (8 G):
 * UD_ERR_INVALID.  ud_plb_density_seq_work_bytes(h, M) = 8 G min(M, C) with C = the items that fit into 256 MiB (at least one, at
 * most 65535): never more than max(256 MiB, 8 G).
 * sign (may be NULL = no backward): ud_plb_density_seq_sign_bytes(h, M) bytes (2 bits per cell and item, 16-byte aligned), opaque;
 * three-valued, 0 where df == 0 and where df is NaN, as ud_plb_loss_bwd decides it (an empty cell of an empty target sends nothing).
 * A NaN in a target cell or in a coordinate makes the loss of the items that read it NaN and leaves every other item's loss, sign
 * field and g_x as they are without it; the backward reads the sign bit of the CLAMPED cell, the one the forward added to.
 * A target_index[m] outside [0, T) reads nothing out of bounds: loss[m] = NaN, that item's sign field is all zero, so its g_x is 0.
 * ud_plb_density_seq_bwd: g_x[m,p] = inv_dx g_loss[m] p_mass sum_{27 cells} sign_I grad w_I -- one gather per particle, no atomics, no
 * scratch: bit-identical from run to run for one sign field.  x is the forward's.
 * M < 1, T < 1, a null handle / x / targets / loss / work (fwd), a null x / sign / g_loss / g_x (bwd): UD_ERR_INVALID. */
size_t ud_plb_density_seq_work_bytes(const ud_plb* h, long M);
size_t ud_plb_density_seq_sign_bytes(const ud_plb* h, long M);
int ud_plb_density_seq_fwd(ud_plb* h, long M, const double* x, const double* targets, int T, const int* target_index, double* loss,
                           void* sign, void* work, size_t work_bytes, void* stream);
int ud_plb_density_seq_bwd(ud_plb* h, long M, const double* x, const void* sign, const double* g_loss, double* g_x, void* stream);

/* Chamfer distance of point clouds, the number an identification ends with (solver.py:187-196, scipy cdist), forward only, handle-free:
 * a [M,Na,3]; b [Tb,Nb,3]; b_index [M] (device int32; NULL = cloud 0 for every item); out [M]:
 *   out = mean_i min_j d(a_i, b_j) + mean_j min_i d(a_i, b_j),  d = sqrt((dx dx + dy dy) + dz dz), unfused.
 * min_ab [M,Na], min_ba [M,Nb] (each may be NULL) receive the two sets of minima.  NaN propagates as np.min does.  The means are
 * fixed-order sums: the same input gives the same bits, with or without the min arrays.  With both arrays given and M <= 65535 the
 * minima are taken by ceil(Na / 256) + ceil(Nb / 256) workgroups per item (the design point, 10 000 x 10 000 points per item);
 * with one array or none, or M > 65535, by one workgroup per item, which fills whichever array is given.  Every route gives the same
 * bits in out and in the minima.  Nothing of size Na x Nb is ever stored.  A b_index[m] outside [0, Tb) reads nothing out of bounds: out[m] and
 * that item's minima are NaN.  M, Na, Nb, Tb < 1 or a null a / b / out: UD_ERR_INVALID. */
int ud_plb_chamfer(long M, int Na, const double* a, int Tb, int Nb, const double* b, const int* b_index, double* out, double* min_ab,
                   double* min_ba, void* stream);

/* Closed-loop policy (GenORM policy/pbm/plb/engine/nn/mlp.py:63-127, driven by optimizer/solver_nn.py:28-43): the reference's MLP over a
 * strided sample of the particle state and every primitive's pose, for B envs, float64, handle-free (csrc/plb_policy.hip).  Launches
 * only: no allocation, no synchronisation, no atomics, capturable in a HIP graph; two runs give the same bits.
 *   dims (host, n_layer + 1 ints) = d_0 .. d_L;  d_0 = 6 obs_num + 7 P;  d_L = the action dimension.
 *   observation h_0[b] (mlp.py:68-86): for i < obs_num: x[b, i obs_step, 0..2], then v[b, i obs_step, 0..2] * velocity_weight; then per
 *     primitive prim_pos[b,p,0..2], prim_rot[b,p,0..3] (w, x, y, z).  x, v [B,N,3]; prim_pos [B,P,3]; prim_rot [B,P,4].
 *   layers (mlp.py:111-125): h_{l+1} = act(W_l h_l + b_l), W_l [d_{l+1}, d_l] row-major; activation 0 = relu, 1 = tanh on the hidden
 *     layers, none on the last.   action [B, d_L] = clamp(h_L, -1, 1) (mlp.py:92-99).
 *   params (get_params, mlp.py:161-166): W_0, b_0, W_1, b_1, ... flat, ud_plb_policy_n_params(n_layer, dims) doubles; env b reads
 *     params + b * param_stride: n_params (or more) for B policies side by side, 0 for one policy shared by every env.
 *   velocity_weight (mlp.py:44, needs_grad=False) is a plain argument and is not differentiated.
 *   tape: ud_plb_policy_tape_bytes(B, n_layer, dims) bytes, opaque (every layer's output and d_1 words per env that the backward hands
 *     from its first launch to its second: the backward WRITES those, so two backward calls on one tape must not run concurrently; one
 *     after the other they are independent).  NULL in the forward = no backward follows; the action has the same bits either way.
 * ud_plb_policy_bwd: given g_action [B, d_L] writes g_x, g_v [B,N,3] in full (zero at unobserved particles, g_v carrying
 *   velocity_weight), g_prim_pos [B,P,3], g_prim_rot [B,P,4], and ADDS the parameter gradient to g_params [B, n_params] (one row per
 *   env also with param_stride 0; the caller zeroes it: Taichi's W.grad / b.grad, get_grad mlp.py:154-159).  The clamp passes the
 *   cotangent where |h_L| <= 1, equality included; relu passes it where the output is > 0.  params are the forward's.
 * Limits: n_layer in [1, 4] (0 to 3 hidden layers); d_1 .. d_L in [1, 1024]; d_0 in [1, 4096]; B in [1, 65535]; P in [0, 64].
 * UD_ERR_INVALID, with nothing launched: n_layer or a width outside those limits, dims[0] != 6 obs_num + 7 P, obs_step < 1,
 * (obs_num - 1) obs_step >= N, activation not 0 / 1, a null array, 0 < param_stride < n_params.  The two size calls return 0 for
 * n_layer outside the limits or a width below 1. */
size_t ud_plb_policy_n_params(int n_layer, const int* dims);
size_t ud_plb_policy_tape_bytes(int B, int n_layer, const int* dims);
int ud_plb_policy_fwd(int B, int N, int P, int obs_step, int obs_num, int n_layer, const int* dims, int activation, double velocity_weight,
                      const double* x, const double* v, const double* prim_pos, const double* prim_rot, const double* params,
                      long param_stride, double* action, void* tape, void* stream);
int ud_plb_policy_bwd(int B, int N, int P, int obs_step, int obs_num, int n_layer, const int* dims, int activation, double velocity_weight,
                      const double* params, long param_stride, void* tape, const double* g_action, double* g_x, double* g_v,
                      double* g_prim_pos, double* g_prim_rot, double* g_params, void* stream);

/* Point-cloud policy (GenORM policy/pnet2_layers with tf_ops/sampling/tf_sampling_g.cu and tf_ops/grouping/tf_grouping_g.cu): the
 * sampling and grouping ops of the PointNet++ single-scale-grouping model, float32, handle-free (csrc/pc_group.hip).  Launches only: no
 * allocation, no synchronisation, no environment variable, no atomics, capturable in a HIP graph; two runs give the same bits.  Indices
 * are int32.  Every input is finite: a NaN (or an overflowing distance that turns into one) is outside the contract.  B in [1, 65535].
 *
 * ud_pc_fps: farthest-point sampling and the gather_point that follows it, one launch.  xyz [B,n,3] -> idx [B,m], new_xyz [B,m,3] =
 *   xyz[b, idx[b,j]].  idx[b,0] = 0; with mind[k] = 1e38f at the start, sample j updates mind[k] = min(mind[k], d(k, sample j-1)) and
 *   takes the arg-max of mind, d = (dx dx + dy dy) + dz dz unfused.  TIE RULE: the lowest index among the maxima.  That is the
 *   reference's block reduction for n <= 512 (every cloud the policy feeds it); for larger n the reference breaks ties by
 *   (k mod 512, k), which this call does not reproduce.  The deviation shows only on exact f32 ties between different points; tied
 *   duplicates have equal coordinates, so new_xyz is the same.  m > n is legal (the policy samples 512 of 200): once every mind is 0
 *   index 0 repeats.  n in [1, 8192] (above: UD_ERR_UNSUPPORTED), m >= 1.  n <= 256 runs one wave per cloud, larger n one workgroup.
 * ud_pc_ball_query: xyz [B,n,3], new_xyz [B,m,3] -> idx [B,m,nsample], cnt [B,m].  Row (b,j) = the first nsample indices k, ascending,
 *   with fmaxf(sqrtf((dx dx + dy dy) + dz dz), 1e-20f) < radius (strict; the correctly rounded sqrt, not s < r r); the remaining slots
 *   repeat the first hit; cnt = the number of hits, at most nsample.  A centre without a hit gets a row of zeros and cnt 0 (the
 *   reference leaves that row uninitialised).
 * ud_pc_group_fwd: sample_and_group's group, recentre and concat (pnet2_layers/utils.py:26-31), xyz first:
 *   out [B,m,nsample,3+C]: out[b,j,k,:3] = xyz[b,idx[b,j,k]] - new_xyz[b,j], out[b,j,k,3:] = feats[b,idx[b,j,k]].  feats [B,n,C], NULL
 *   with C = 0.  An index outside [0, n) reads nothing and gives a row of zeros.
 * ud_pc_group_bwd: its adjoint; every output is WRITTEN in full (nothing is added to).  g_new_xyz[b,j] = -(sum_k g_out[b,j,k,:3]), k
 *   ascending from +0; g_xyz[b,i] / g_feats[b,i] = the sum of g_out[b,j,k,:3] / [3:] over the (j,k) with idx[b,j,k] = i, in ascending
 *   (j,k) from +0 (an index outside [0, n) adds to nothing).  centre_idx [B,m] (the FPS indices; NULL = new_xyz is an independent
 *   input): g_new_xyz[b,j] is then added into g_xyz[b, centre_idx[b,j]], ascending j, after the sums above.  g_feats may be NULL
 *   with C = 0.  No scratch.
 * m nsample (3 + C) < 2^31 - 256 for the two group calls (UD_ERR_UNSUPPORTED above).  A size below 1, C < 0 or a null array:
 * UD_ERR_INVALID.  Nothing is launched on an error. */
int ud_pc_fps(int B, int n, int m, const float* xyz, int* idx, float* new_xyz, void* stream);
int ud_pc_ball_query(int B, int n, int m, float radius, int nsample, const float* xyz, const float* new_xyz, int* idx, int* cnt,
                     void* stream);
int ud_pc_group_fwd(int B, int n, int m, int nsample, int C, const float* xyz, const float* feats, const float* new_xyz, const int* idx,
                    float* out, void* stream);
int ud_pc_group_bwd(int B, int n, int m, int nsample, int C, const int* idx, const int* centre_idx, const float* g_out, float* g_xyz,
                    float* g_feats, float* g_new_xyz, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Cloth-env arithmetic either side of the rollout (the reference jit-fuses it into step_diff; here one forward and
 * one backward kernel per piece, one workgroup per env, instead of ~180 elementwise launches per step_diff).
 *   ud_chamfer_*    core/utils/util.py:138-153  calc_chamfer(x [B,P,3], y [Q,3]) -> [B]:
 *                   d(p,q) = sqrt(mean_xyz((x_p - y_q)^2)); out = mean_q min_p d + mean_p min_q d.
 *                   idx_xy [B,P] / idx_yx [B,Q] (int32) are the argmins the backward routes the cotangent through.
 *   ud_cloth_pnp_*  core/envs/basic/cloth_env.py:134-173 get_pnp_actions (actions [B,6], primitive0 [B,4]) ->
 *                   macro_actions [40,B,8], and :206-209 contact_distance [B] = min_p |actions[:, :3] - x_p|.
 *   ud_cloth_depth_* core/envs/basic/cloth_env.py:71-92 state_to_depth: the DEPTH observation (csrc/env_depth.hip), below.
 * P, Q <= 4096.  The backward entry points return what jax.grad returns for the same expressions.
 * ------------------------------------------------------------------------------------------------ */
int ud_chamfer_fwd(int B, int P, int Q, const float* x, const float* y, float* out, int* idx_xy, int* idx_yx, void* stream);
int ud_chamfer_bwd(int B, int P, int Q, const float* x, const float* y, const int* idx_xy, const int* idx_yx,
                   const float* g_out, float* g_x, void* stream);
int ud_cloth_pnp_fwd(int B, int P, const float* actions, const float* primitive0, const float* x, float* macro_actions,
                     float* contact_distance, int* contact_idx, void* stream);
/* g_contact_distance may be NULL (no auxiliary reward); g_x [B,P,3] is written in full (zero except the contact row) */
int ud_cloth_pnp_bwd(int B, int P, const float* actions, const float* x, const float* contact_distance,
                     const int* contact_idx, const float* g_macro_actions, const float* g_contact_distance,
                     float* g_actions, float* g_primitive0, float* g_x, void* stream);
/* DEPTH observation, core/envs/basic/cloth_env.py:71-92 (state_to_depth), for each of M images (B envs, or T*B for a state list):
 *   img [M,H,W] = zeros.at[py, px].set(x.y + z_offset) with px = clip(floor(x.x / pixel_size), 0, W-1), py = clip(floor(x.z /
 *   pixel_size), 0, H-1).  The division is a true IEEE f32 division and the clip is taken on the float, so -inf / NaN land in
 *   pixel 0 and +inf in the last one.  A pixel holds the height that is last in ascending (height, particle index) order
 *   among the particles landing there (stable argsort, last write wins; NaN above +inf); untouched pixels are 0.
 *   owner [M,P] (int32) = py*W + px for the particle that owns its pixel, -1 for every other; NULL when no backward follows.
 *   ud_cloth_depth_bwd: g_x [M,P,3], written in full: g_x[p].y = g_img[owner[p]] for owners, every other entry 0.
 * P <= 4096 and H*W <= 131072 (UD_ERR_UNSUPPORTED otherwise).  One launch each, bit-identical from run to run. */
int ud_cloth_depth_fwd(int M, int P, int H, int W, float pixel_size, float z_offset, const float* x, float* img, int* owner,
                       void* stream);
int ud_cloth_depth_bwd(int M, int P, int H, int W, const int* owner, const float* g_img, float* g_x, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MPM-env arithmetic either side of simulator.step (core/envs/basic/mpm_env.py), one workgroup per env.
 *   ud_mpm_focus_*   pre_step :99-114: shift [B,3] = (cx - mean_n x.x, 0, cz - mean_n x.z) with (cx, cz) = res/2/n_grid;
 *                    x_out = x + shift; prim_pos_out[p] = prim_pos[p] + shift for the n_prim (<= 4) primitive
 *                    trajectories [B,S,3].  prim_pos / prim_pos_out are HOST arrays of n_prim device pointers.
 *   ud_mpm_finish_*  post_step :116-125 (x - shift, prim_pos - shift; shift NULL = no focus), nan_to_num on x v C F J
 *                    :150-154, reward_func :90-94 = e ** (-10 * mean_n sqrt(mean_xyz((x - goal)^2))) with goal [Q,3], Q = N or 1
 *                    (calc_l2 broadcasts; a missing goal file is zeros((1,3)), mpm_env.py:46-48),
 *                    get_obs :57-76: obs [B, 6N + 3S] = x | v | primitive 0 trajectory.
 * Backward entry points: any cotangent pointer (and any entry of g_prim_pos_out) may be NULL = that output was unused.
 * nan_to_num passes a cotangent only where its argument was finite (jnp.where selection).  ud_mpm_focus_bwd does not
 * write primitive cotangents: they pass through unchanged (g_prim_pos[p] = g_prim_pos_out[p]).
 * ------------------------------------------------------------------------------------------------ */
int ud_mpm_focus_fwd(int B, int N, int n_prim, int S, float cx, float cz, const float* x, const float* const* prim_pos,
                     float* x_out, float* const* prim_pos_out, float* shift, void* stream);
int ud_mpm_focus_bwd(int B, int N, int n_prim, int S, const float* g_x_out, const float* const* g_prim_pos_out,
                     const float* g_shift, float* g_x, void* stream);
int ud_mpm_finish_fwd(int B, int N, int n_prim, int S, int Q, const float* x, const float* v, const float* C, const float* F,
                      const float* J, const float* shift, const float* const* prim_pos, const float* goal, float* x_out,
                      float* v_out, float* C_out, float* F_out, float* J_out, float* const* prim_pos_out, float* reward,
                      float* obs, void* stream);
/* shift and g_shift are both NULL or both given; g_shift [B,3] = -(sum of every shifted cotangent) */
int ud_mpm_finish_bwd(int B, int N, int n_prim, int S, int Q, const float* x, const float* v, const float* C, const float* F,
                      const float* shift, const float* goal, const float* reward, const float* g_x_out, const float* g_v_out,
                      const float* g_C_out, const float* g_F_out, const float* const* g_prim_pos_out, const float* g_reward,
                      const float* g_obs, float* g_x, float* g_v, float* g_C, float* g_F, float* const* g_prim_pos,
                      float* g_shift, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PLB renderer: TaichiEnv.render() (GenORM/policy/pbm/plb/engine/renderer/renderer.py, renderer_utils.py) for B envs per call.
 * A handle of its own; ud_plb_conf is not involved.  f32 throughout, as the reference's fields are.  The operation order written
 * below IS the contract: tests/plb_render_twin.py restates it in NumPy f32 and is the specification.  Parity with the reference
 * itself is UNPINNED by reference data: neither Taichi nor cv2 can be run beside this library, so no image of the reference's was
 * ever compared; the order below is read off its source.  Every a*b+c below is a rounded multiply, then a rounded add; divisions
 * and square roots are correctly rounded; norm(v) = sqrtf((v0*v0 + v1*v1) + v2*v2); normalize(v) = (1.0f / norm(v)) * v.
 * The directional light and Russian roulette (envs/torus.yml sets use_directional_light) are handle state, set by
 * ud_plb_render_set_light below; the two conf fields of those names must stay 0 (UD_ERR_UNSUPPORTED at create).  The `target`
 * overlay (commented out in the reference's next_hit) does not exist here.
 *
 * Arenas, all allocated at create for max_envs: 16 B per voxel cell and env (packed volume 8, sdf 4, smoothing scratch 4); the
 * reference's separate colour volume (12 B) is not kept, the colour bytes are decoded from the packed volume when sampled.  The
 * calls below launch (or enqueue copies) only: no allocation, no host synchronisation.
 *
 * ud_plb_render_bake (set_particles, :453-480, build_sdf_from_particles :88-131): x [B,N,3] f64, color [N] i32 (0xRRGGBB) ->
 *   bbox [B,2,3], status [B]; volume and sdf stay in the handle.  Per env: px = (float)x; bbox0[c] = min_i (floorf(px[c] * inv_dx)
 *   - 6.0f) * dx with dx = (float)conf.dx, inv_dx = (float)(1.0 / conf.dx); hi[c] the same with max; status = 1 when (hi[c] -
 *   bbox0[c]) / dx >= voxel_res[c] on any axis (the reference's assert) -- such an env is not baked and every later output of it
 *   is zero; bbox1 = (float)((double)bbox0 + voxel_res * (double)dx).  Every cell starts at 2^32 - 1.  For every particle and every
 *   offset (i,j,k) in [-bake_size-1, bake_size]^3: p = (px - bbox0) * inv_dx; idx = (int)p + (i,j,k), skipped outside the volume;
 *   d = (float)idx - p; dist = sqrtf((d0*d0 + d1*d1) + d2*d2); q = fminf(fmaxf(0, 51.0f * dist), 255.0f); atomic 64-bit min of
 *   ((int64)q << 24) + color.  sdf = ((c >> 24) & 255) / 255.0f; colour channel j = ((c >> 8 (2 - j)) & 255) / 255.0f.  Two
 *   smoothing passes (sdf -> scratch -> sdf): a boundary cell becomes 1, an interior one (sum of its 27 neighbours) / 27.0f, the
 *   sum starting from 0.0f with the first axis's offset outermost and the last innermost.  Volumes are [rx][ry][rz], z fastest.
 * ud_plb_render_read_volume: copies the packed volume [B,rx,ry,rz] (i64) and / or the smoothed sdf (f32) out (either may be NULL).
 *
 * Primitive state of the two calls below: prim_pos [B,n_prim,3], prim_rot [B,n_prim,4] (w,x,y,z; NULL = identity), prim_gap
 *   [B,n_prim] (read for a Chopsticks only; NULL otherwise), f64.  Distance and normal of primitive i at the f32 point pp:
 *   the shape layer of csrc/plb_prim.h in f64 (kinds 0..6) at qrot(conj(rot) / |rot|, (double)pp - pos), the normal turned back
 *   by qrot(rot, .), both cast to f32.
 *
 * ud_plb_render_gbuffer: the first hit of one ray per pixel through the pixel centre (both jitters 0.5), outputs [B,res0,res1]
 *   indexed (env, u, v): kind (0 nothing, 1 background plane, 2 ground, 3 + i primitive i, 16 body), t, normal [.,3], albedo [.,3].
 *   Camera: mat = Ry(camera_rot[1]) @ Rx(camera_rot[0]) as at :433-441, formed in f64 at create and rounded to nine f32;
 *   c = normalize(((0.46f * (u + ju)) / res1 - (float)(0.23 * res0 / res1)) - 1e-5f, ((0.46f * (v + jv)) / res1 - 0.23f) - 1e-5f,
 *   -1); d[r] = (mat[r][0] * c0 + mat[r][1] * c1) + mat[r][2] * c2; o = camera_pos.
 *   next_hit (:202-325) as written, closest = 1e10f, roughness = 0.05f at the start:
 *     plane: d2 != 0: rc = -(o2 + 5.5f) / d2, taken when rc > 0 and rc < closest; normal (0,0,1), colour (0.6,0.7,0.7), roughness 0.
 *     ground: d1 < 0: gd = (o1 + 0.002f) / (-d1), taken when gd < 100 and gd < closest; normal (0,1,0), roughness 0; p = o + d * gd;
 *       colour (0.3,0.5,0.7) * f, f = (float)(((int)(p0 / 0.25f) + (int)(p2 / 0.25f)) % 2) * 0.2f + 0.35f inside [0,1]^2, else 0.4f.
 *     primitives: dist = 0, sdf = 1e10f; while j < 200 and dist < 100 and sdf > 1e-8f: pp = o + dist * d; sdf = the smallest
 *       distance (the first primitive on a tie); dist += sdf.  Taken when dist < closest and dist < 100; normal at o + dist * d.
 *     body: ray_aabb_intersection (renderer_utils.py:42-70) with bbox; tnear = max(tnear, 0); pos = o + d * (tnear + 1e-4f);
 *       500 steps: s = sample_sdf(pos); s < 0: back = step, 20 times { back = back * 0.5f; if sample_sdf(pos - back) < 0: pos =
 *       pos - back }, dist = norm(o - pos), taken when dist < closest (normal, colour below; roughness keeps its value), stop;
 *       else step = d * fmaxf(s * 0.05f, 0.01f), pos += step.
 *     sample_sdf(pos): q = (pos - bbox0) / (bbox1 - bbox0); 0.0f unless every q[c] in [0,1]; else sample_tex(sdf, q) -
 *       (float)sdf_threshold.  sample_tex: p = q * res; base = min((int)p, res - 1); f = p - base; base1 = min(base + 1, res - 1);
 *       c00 = T[x,y,z] (1 - f0) + T[x1,y,z] f0; c01 = T[x,y,z1] .. T[x1,y,z1]; c10 = T[x,y1,z] .. T[x1,y1,z]; c11 = T[x,y1,z1] ..
 *       T[x1,y1,z1]; c0 = c00 (1 - f1) + c10 f1; c1 = c01 (1 - f1) + c11 f1; c0 (1 - f2) + c1 f2.  Colour: the same per channel.
 *     normal: n[i] = 500.0f * (sample_sdf(p + 1e-3f e_i) - sample_sdf(p - 1e-3f e_i)), normalized.
 *
 * ud_plb_render_image: render + trace + copy (:346-451) for spp samples (0 = the conf's) -> img [B,res1,res0,3] f32, already in
 *   render_frame's orientation (img[:, ::-1].transpose(1, 0, 2): row = res1 - 1 - v, column = u).  Per sample: the ray above with
 *   jitters r(.,.,0), r(.,.,1); throughput 1; up to max_ray_depth times: hit = next_hit(pos, d); hp = pos + t * d; if norm(normal)
 *   != 0: out_dir(normal) (renderer_utils.py:8-18: u = (1,0,0), or normalize(cross(n, (0,1,0))) when |n1| < 0.999f; v = cross(n, u);
 *   phi = 6.2831855f * r_phi; ay = sqrtf(r_r); ax = sqrtf(1 - r_r); ax * (cosf(phi) * u + sinf(phi) * v) + ay * n), glossy =
 *   (x, yz cosf(phi'), yz sinf(phi')) * roughness with x = r_u * 2 - 1, phi' = (r_v * 2) * 3.1415927f, yz = sqrtf(1 - x * x);
 *   d = normalize(out_dir + glossy); pos = hp + 1e-4f * d; throughput *= colour; else stop.  hit_sky is never cleared in the
 *   reference, so the sample is throughput * sky_color(d): c = clamp(((d0 * 0.8f + d1 * 0.65f) + d2 * 0.15f) * 0.5f + 0.5f, 0, 1),
 *   (c * 0.9f + (1 - c) * (0.7f, 0.7f, 0.8f)) * 1.5f.  Samples are summed in order from 0.0f.  copy: darken = 1 - 0.9f *
 *   fmaxf(sqrtf((u / res0 - 0.5f)^2 + (v / res1 - 0.5f)^2) - 0.0f, 0); img = sqrtf(((sum * darken) * 1.5f) / (float)spp).
 *   cosf / sinf are the device library's (an ulp from any other).
 *   The random draws are THIS PROJECT'S OWN (ti.random cannot be pinned): r(pixel, sample, k) = (h >> 8) * 2^-24, h =
 *   lowbias32(seed ^ (pixel * 0x9E3779B9 + sample * 0x85EBCA6B + k * 0xC2B2AE35)) in u32 wrap-around arithmetic, pixel = u * res1
 *   + v (the env does not enter: equal envs give equal images), lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *=
 *   0x846ca68b; x ^= x >> 16.  k = 0, 1: the pixel jitters; bounce b: k = 2 + 4b + (0 phi, 1 r of out_dir; 2 u, 3 v of glossy);
 *   k = 2^30 + 4b + (0, 1, 2 the light noise; 3 the roulette) -- the two ranges stay apart up to bounce 2^28 - 2.
 *
 * ud_plb_render_set_light: use_directional_light / use_roulette of cfg.RENDERER (:374-397) as handle state; host only (no launch,
 *   no allocation), read by the next ud_plb_render_image (ud_plb_render_gbuffer is unaffected).  light_direction is rounded to
 *   f32 at the call.  A null argument, a direction that is not finite in f32, or an all-zero one with use_directional_light on:
 *   UD_ERR_INVALID, the handle unchanged.  With both flags 0 the handle is a fresh one's (the image is bit-identical).  The image
 *   kernel is compiled once per (light, roulette); what the two add to the loop above:
 *   light, after pos = hp + 1e-4f * d and throughput *= colour of bounce b: noise[j] = (r_j - 0.5f) * 0.03f; direct =
 *     normalize(light_direction + noise); dot = (direct0 * n0 + direct1 * n1) + direct2 * n2; if dot > 0 and next_hit(pos, direct)
 *     returns a distance > 100: contrib += (throughput * 1.0f) * dot (light_color is 1); contrib starts at 0 per sample.  The
 *     sample is then contrib and the sky term is NOT added (:408-410).  The shadow ray is answered by an any-hit search: next_hit's
 *     candidates in next_hit's order with next_hit's conditions, stopping at the first one <= 100, no normal or colour fetched --
 *     next_hit's closest is its smallest candidate, so this is the same boolean.  The background plane z = -5.5 takes part: a
 *     light_direction with negative z meets it at -(pos2 + 5.5f) / direct2, which is <= 100 wherever pos2 <= 100 |direct2| - 5.5
 *     (for (2, 1, -0.7): z <= 24.4, about 20 away from anything in view).  Such a light is therefore occluded at every first hit
 *     of a camera that looks along -z (those lie at z <= camera z) and a max_ray_depth 1 image is exactly zero; with more bounces
 *     only a ray that lands on the unbounded ground that far behind the camera is lit.  The reference's behaviour as written; kept.
 *   roulette, at the end of every loop iteration, the one that hit the sky included: max_c = fmaxf(fmaxf(t0, t1), t2) of the
 *     throughput; if r > max_c: stop, throughput = 0; else throughput[c] = throughput[c] / max_c.  max_c == 0 with r == 0 divides
 *     0 by 0 as the reference does (NaN throughput from there on); kept as written.
 *
 * B < 1 or B > max_envs, a null handle or array (prim_pos on a handle with primitives; prim_gap with a Chopsticks): UD_ERR_INVALID,
 * nothing launched, no output touched.  Results are bit-identical from run to run.
 * ------------------------------------------------------------------------------------------------ */
#define UD_PLB_RENDER_MAX_PRIM 4
typedef struct ud_plb_render ud_plb_render;
/* (the tag is not needed: the binding parses tagged and untagged structs alike, and tools/gen_binding_stub.py names the structs it lists) */
typedef struct ud_plb_render_conf {
  double dx;                  /* cfg.RENDERER.dx, default 1 / 150 */
  int voxel_res[3];           /* (168, 168, 168); each >= 2 * bake_size and in [2, 1024], else UD_ERR_INVALID */
  int bake_size;              /* 6 */
  double sdf_threshold;       /* 0.65 * 0.56 */
  int image_res[2];           /* (512, 512) */
  int spp;                    /* 50: what ud_plb_render_image takes for spp = 0 */
  int max_ray_depth;          /* 2 */
  double camera_pos[3];       /* (0.5, 1.2, 4.0) */
  double camera_rot[2];       /* (0.2, 0.0) */
  int use_directional_light;  /* must be 0 (UD_ERR_UNSUPPORTED): see ud_plb_render_set_light */
  int use_roulette;           /* must be 0 (UD_ERR_UNSUPPORTED): see ud_plb_render_set_light */
  int n_primitives;           /* 0 .. UD_PLB_RENDER_MAX_PRIM */
  int prim_kind[UD_PLB_RENDER_MAX_PRIM];         /* as ud_plb_conf.prim_kind, 0 .. 6 */
  double prim_radius[UD_PLB_RENDER_MAX_PRIM];    /* Sphere / Capsule / RollingPin / Chopsticks radius */
  double prim_h[UD_PLB_RENDER_MAX_PRIM];         /* Capsule / RollingPin / Chopsticks height */
  double prim_shape[UD_PLB_RENDER_MAX_PRIM][3];  /* as ud_plb_conf.prim_shape (Box, Cylinder, Torus) */
  float prim_color[UD_PLB_RENDER_MAX_PRIM][3];   /* the primitive's cfg colour */
  int n_particles;            /* N of every bake call */
  int max_envs;               /* arenas are allocated for this many envs; a call with more returns UD_ERR_INVALID */
} ud_plb_render_conf;
int ud_plb_render_create(const ud_plb_render_conf* conf, ud_plb_render** out);
int ud_plb_render_destroy(ud_plb_render* h);
typedef struct ud_plb_render_light {
  int use_directional_light;  /* cfg.RENDERER.use_directional_light (default off; envs/torus.yml: on) */
  int use_roulette;           /* cfg.RENDERER.use_roulette (off everywhere in the reference) */
  double light_direction[3];  /* cfg.RENDERER.light_direction, default (2, 1, 0.7); not normalised by the caller */
} ud_plb_render_light;
int ud_plb_render_set_light(ud_plb_render* h, const ud_plb_render_light* light);
int ud_plb_render_bake(ud_plb_render* h, int B, const double* x, const int* color, float* bbox, int* status, void* stream);
int ud_plb_render_read_volume(ud_plb_render* h, int B, long long* packed, float* sdf, void* stream);
int ud_plb_render_gbuffer(ud_plb_render* h, int B, const double* prim_pos, const double* prim_rot, const double* prim_gap, int* kind,
                          float* t, float* normal, float* albedo, void* stream);
int ud_plb_render_image(ud_plb_render* h, int B, const double* prim_pos, const double* prim_rot, const double* prim_gap, int spp,
                        unsigned int seed, float* img, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Cloth renderer: MeshPyRenderer.render (daxbench/core/engine/pyrender/py_render.py:16-117) for M frames per call: the cloth's
 * triangle mesh (two-sided), S analytic spheres per frame (the gripper) and the ground rectangle, seen by the reference's camera.
 * A handle of its own; ud_cloth_conf is not involved.  f32 throughout.  The operation order written below IS the contract:
 * tests/cloth_render_twin.py restates it in NumPy f32, is the specification, and is bit-equal in colour, depth and triangle id.
 * Camera, projection, coverage, depth, mirror and channel order are the reference's.  UNPINNED by reference data (pyrender, OpenGL
 * and the wood texture cannot be had beside this library; nothing of the reference's was ever rendered for comparison):
 *   - the SHADING is this project's own (pyrender's PBR shader is not restated): flat normals, Lambert, the reference's three lights;
 *   - the ground is one flat colour, not wood_uv.png;
 *   - the gripper is an analytic sphere, not the reference's icosphere with random face colours;
 *   - a triangle with a vertex nearer than znear is dropped whole, not clipped (the cloth never comes within 0.05 of this camera).
 * Every a*b+c below is a rounded multiply, then a rounded add; divisions and square roots are correctly rounded; sums of three
 * are (a + b) + c.  Only + - * / sqrt min max floor ceil and comparisons occur.
 *
 * Frames.  The render frame is z-up: a sim point (x, y, z) is the render point (x, z, y) (py_render.py:83); vertices and sphere
 *   centres are passed in sim order and swapped here.  conf positions (camera, ground) are in the render frame.
 * Constants, formed in f64 at create and rounded to f32 once: look_at (:50-70) z = normalize(camera_pos - camera_target), x =
 *   normalize(cross(camera_up, z)), y = cross(z, x) -> R (rows x, y, z), P = camera_pos; t = tan(yfov / 2); fy = (height / 2) / t;
 *   fx = (width / 2) / ((width / height) t); cx = width / 2; cy = height / 2; cos_outer = cos(pi / 6); cos_range = cos(pi / 16) -
 *   cos(pi / 6); inv_pi = 1 / pi.  The light pose is the camera pose (the reference's cam_pose = None).
 * eye(p), p in the render frame: q = p - P; (R[r][0] q0 + R[r][1] q1) + R[r][2] q2 for r = 0, 1, 2.  The camera looks along -z.
 * Setup, per vertex: (xe, ye, ze) = eye; d = -ze; sx = cx + (fx xe) / d; sy = cy - (fy ye) / d.
 * Pixel (row v, column u) of the unmirrored image, row 0 at the top: px = u + 0.5, py = v + 0.5; its ray in the eye frame is
 *   t (rx, ry, -1) with rx = (px - cx) / fx, ry = (cy - py) / fy, so t is the depth (-z_eye).
 * Mesh.  Triangle i with vertices A, B, C (indices ia, ib, ic):
 *   dropped when any d < znear (not d >= znear); area = (Bx - Ax)(Cy - Ay) - (By - Ay)(Cx - Ax) on (sx, sy); dropped when area is
 *   not < 0 or > 0; s = sign(area).  Candidate pixels: ceil(min sx - 0.5) <= u <= floor(max sx - 0.5), the same in v with sy.
 *   edge(p -> q) at (px, py), with (p', q') = (p, q) when index(p) < index(q), else (q, p): e = (q'x - p'x)(py - p'y) - (q'y -
 *   p'y)(px - p'x), negated when the ends were swapped -- so the two triangles that share an edge compute exact negatives and the
 *   inclusive test below leaves no hole.  e0 = edge(B -> C), e1 = edge(C -> A), e2 = edge(A -> B).  Covered when s e0 >= 0, s e1
 *   >= 0, s e2 >= 0 and s esum > 0 with esum = (e0 + e1) + e2 (the doubled area, as the sum the barycentrics b_i = e_i / esum are
 *   normalised by: they add up to one to a rounding, which b_i = e_i / area does not for sub-pixel triangles).
 *   depth = esum / ((e0 / dA + e1 / dB) + e2 / dC) (perspective-correct: 1 / sum b_i / d_i); taken when depth >= znear.  The nearest
 *   depth wins, on equal depth bits the lower triangle index.
 * Spheres j = 0 .. S-1 (centre in sim order, radius r; r <= 0: absent): c = eye(centre); qa = (rx rx + ry ry) + 1; tc = ((rx cx
 *   + ry cy) - cz) / qa; q = (cx - tc rx, cy - tc ry, cz + tc); h2 = r r - ((qx qx + qy qy) + qz qz); hit when h2 >= 0; ts = tc -
 *   sqrt(h2 / qa), taken when ts >= znear (the near root only) and the pixel holds nothing yet or ts < the depth it holds (so the
 *   mesh and the earlier sphere keep an exact tie); normal ((ts rx - cx) / r, (ts ry - cy) / r, (-ts - cz) / r).
 * Ground, in the render frame: D[c] = (R[0][c] rx + R[1][c] ry) - R[2][c]; when D2 < 0: tg = (ground_z - P2) / D2; hx = P0 + tg D0;
 *   hy = P1 + tg D1; taken when tg >= znear, ground_min <= (hx, hy) <= ground_max and the pixel holds nothing or tg < its depth.
 *   Normal: the third column of R.
 * Shading of the winner at e = (depth rx, depth ry, -depth): mesh normal n = cross(B - A, C - A) of the eye positions, divided by
 *   its length sqrt((n0 n0 + n1 n1) + n2 n2) ((0, 0, 1) when that is 0).  ne = (n0 e0 + n1 e1) + n2 e2; ne > 0: n = -n.
 *   ndl_d = max(n2, 0); r2 = (e0 e0 + e1 e1) + e2 e2; rl = sqrt(r2); ndl_s = max(-((n0 e0 + n1 e1) + n2 e2) / rl, 0);
 *   cosang = -e2 / rl; s = min(max((cosang - cos_outer) / cos_range, 0), 1); spot = (s s)(3 - 2 s);
 *   lit = 0.05 + (1 ndl_d + ((10 spot) ndl_s) / r2) inv_pi   (ambient 0.05; directional light 1 along -z; spot light 10 at the eye,
 *   inner cone pi / 16, outer pi / 6, inverse-square);  channel = base * lit; u8 = (int)(min(max(channel, 0), 1) * 255 + 0.5).
 *   Nothing hit: white, depth 0.
 * Outputs, in the orientation py_render.py:110-111 returns: color [M,H,W,3] u8 mirrored left-right with the channels reversed
 *   (pixel (v, u) lands at [v, W-1-u] as B, G, R), depth [M,H,W] f32 mirrored the same way, and tri [M,H,W] i32 (NULL: not
 *   written): the winning triangle index, -1 nothing, -2 a sphere, -3 the ground.
 *
 * ud_cloth_render_create: faces is a HOST array [n_faces,3] of vertex indices, copied into the handle.  A null argument, a size
 *   below 1 (n_faces, n_spheres: below 0), yfov outside (0, pi), znear <= 0, a degenerate look_at or a face index outside [0,
 *   n_vertices): UD_ERR_INVALID.  width or height > 4096, n_vertices or n_faces > 2^20, n_spheres > 16, max_frames > 65535 or
 *   max_frames * n_vertices >= 2^31 - 256: UD_ERR_UNSUPPORTED.  Arena: 20 B per vertex and frame, allocated here for max_frames.
 * ud_cloth_render_frames: vertices [M,n_vertices,3], spheres [M,n_spheres,4] (NULL when n_spheres = 0), device arrays.  Two
 *   launches, no allocation, no host synchronisation.  A null handle / vertices / color / depth (spheres with n_spheres > 0), M < 1
 *   or M > max_frames: UD_ERR_INVALID, nothing launched, no output touched.  Results are bit-identical from run to run.
 * ------------------------------------------------------------------------------------------------ */
typedef struct ud_cloth_render ud_cloth_render;
typedef struct ud_cloth_render_conf {
  int width;                  /* 640 */
  int height;                 /* 480 */
  double yfov;                /* pi / 3 */
  double znear;               /* 0.05 (pyrender's default); no far plane */
  double camera_pos[3];       /* (0.9, 0.5, 1.0), render frame; also the pose of both lights */
  double camera_target[3];    /* (0.6, 0.5, 0.0) */
  double camera_up[3];        /* (0, 0, 1) */
  double ground_min[2];       /* (-0.02, -0.04): wood.obj scaled to 1 x 1 and moved to (0.48, 0.46, -0.02) */
  double ground_max[2];       /* (0.98, 0.96) */
  double ground_z;            /* -0.02 */
  float cloth_color[3];       /* base colours, RGB in [0, 1] */
  float ground_color[3];
  float sphere_color[3];
  int n_vertices;             /* V of every call */
  int n_faces;                /* F */
  int n_spheres;              /* S >= 0 spheres per frame */
  int max_frames;             /* arenas are allocated for this many frames; a call with more returns UD_ERR_INVALID */
} ud_cloth_render_conf;
int ud_cloth_render_create(const ud_cloth_render_conf* conf, const int* faces, ud_cloth_render** out);
int ud_cloth_render_destroy(ud_cloth_render* h);
int ud_cloth_render_frames(ud_cloth_render* h, int M, const float* vertices, const float* spheres, unsigned char* color, float* depth,
                           int* tri, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MPM renderer: what the five MLS-MPM envs show (ParticlePyRenderer and WaterPyRenderer, py_render.py:120-174; the primitives of
 * envs/basic/mpm_env.py:200-236) for M frames per call: one sphere (mode 0) or one screen-space point (mode 1) per particle, n_prims
 * primitives of one kind (0 oriented box, 1 cut hollow sphere) and the ground rectangle, seen by the reference's camera (cam_pose is
 * None in every MPM env: the cloth renderer's camera).  A handle of its own; ud_mpm_conf is not involved.  f32 throughout.  The
 * operation order written below IS the contract: tests/mpm_render_twin.py restates it in NumPy f32 by brute force over all pixels, is
 * the specification, and is bit-equal in colour, depth and id.
 * The reference's: camera, projection, the sphere radius 0.008, the particle grey, the water colour and alpha, the one-pixel point,
 * the unmirrored RGB orientation.  DEVIATIONS, none pinned by reference data (nothing of pyrender's was ever rendered for comparison):
 *   - a particle is an analytic sphere, not a uv_sphere mesh;
 *   - only the nearest point of a pixel blends (pyrender blends every layer in draw order);
 *   - a primitive is drawn where the simulator collides with it, from the inverse transform of inv_trans_batch (primitives.py:105-109),
 *     not through the reference's Euler-angle detour (as_euler('xyz'), negate [2], from_euler('zyx'));
 *   - the cut hollow sphere is sphere-traced on its SDF, not drawn from a marching-cubes mesh;
 *   - a particle nearer than the near plane is dropped whole, not clipped;
 *   - the shading and the primitive / ground colours are this project's own (as for the cloth renderer); the ground is one flat colour.
 * Frames, constants, eye(p), pixel rays (rx, ry), the ground, lit(n, e) and the u8 rounding are EXACTLY those of the ud_cloth_render
 * block above.  Every a*b+c is a rounded multiply, then a rounded add; sums of three are (a + b) + c; only + - * / sqrt min max floor
 * ceil fabs and comparisons occur.
 *
 * Further constants (f32): alpha = particle_color[3]; oma = 1 - alpha; half = point_size * 0.5; thresh = znear + radius (mode 0, one
 *   f32 addition) or znear (mode 1).
 * Setup, per particle (sim order (x, y, z)): (xe, ye, ze) = eye; d = -ze; sx = cx + (fx xe) / d; sy = cy - (fy ye) / d.  The particle
 *   is DROPPED whole when a coordinate is not finite (|c| <= FLT_MAX fails) or d >= thresh fails.
 * Particles, mode 0 (spheres of radius r = radius), per pixel and particle, the cloth block's sphere formulas with c = (xe, ye, -d):
 *   qa = (rx rx + ry ry) + 1; tc = ((rx cx + ry cy) - cz) / qa; q = (cx - tc rx, cy - tc ry, cz + tc); h2 = r r - ((qx qx + qy qy)
 *   + qz qz); hit when h2 >= 0; ts = tc - sqrt(h2 / qa), taken when ts >= znear.  The nearest ts wins, on equal depth bits the lower
 *   particle index.  Normal ((ts rx - cx) / r, (ts ry - cy) / r, (-ts - cz) / r).
 * Particles, mode 1 (points): with px = u + 0.5, py = v + 0.5 the particle covers the pixel when sx - half <= px < sx + half and
 *   sy - half <= py < sy + half (each bound one f32 operation); its depth there is d.  The nearest wins, then the lower index.
 * Primitives j = 0 .. n_prims-1 (position p, quaternion q = (w, x, y, z) of this frame, half sizes s_j from create).  Setup, per
 *   (frame, primitive): c = (q0, -q1, -q2, -q3); nq = sqrt(((c0 c0 + c1 c1) + c2 c2) + c3 c3) + 1e-12; iq = c / nq;
 *   qrot(iq, v): uv = (iq2 v2 - iq3 v1, iq3 v0 - iq1 v2, iq1 v1 - iq2 v0); w = (iq2 uv2 - iq3 uv1, iq3 uv0 - iq1 uv2, iq1 uv1 -
 *   iq2 uv0); out_a = v_a + 2 (iq0 uv_a + w_a)  (primitives.py:95-102).  Column k of A is qrot(iq, unit vector k); the camera in the
 *   local frame is o = qrot(iq, (P0 - p0, P2 - p1, P1 - p2)) (P is in the render frame; sim order swaps its last two).
 *   Per pixel: the ray in the render frame is D[c] = (R[0][c] rx + R[1][c] ry) - R[2][c], in sim order Ds = (D0, D2, D1); in the local
 *   frame dl_a = (A[a][0] Ds0 + A[a][1] Ds1) + A[a][2] Ds2; the point at depth t is o + t dl (o_a + t dl_a).
 *   prim_kind 0, box: tnear = -inf, tfar = +inf, axis = 0; for a = 0, 1, 2: when dl_a == 0 the ray misses unless |o_a| <= s_a and the
 *     axis is skipped; else t1 = (-s_a - o_a) / dl_a, t2 = (s_a - o_a) / dl_a, tn = min(t1, t2), tf = max(t1, t2); tn > tnear: tnear
 *     = tn, axis = a; tfar = min(tfar, tf).  Hit when tnear <= tfar and tnear >= znear, at depth tnear.  Local normal: -1 on `axis`
 *     when dl_axis > 0, else +1; 0 elsewhere.  A half size of 0 is a plate.
 *   prim_kind 1, cut hollow sphere s = (r, h, t) (container.py:8-16 as csrc/mpm_collide.h::container_sdf_x states it): w = sqrt(r r -
 *     h h); sdf(p): q0 = sqrt((p0 p0 + p2 p2) + 1e-12); q1 = p1; d0 = q0 - w; d1 = q1 - h; h q0 < w q1 ? sqrt((d0 d0 + d1 d1) + 1e-12)
 *     - t : |sqrt((q0 q0 + q1 q1) + 1e-12) - r| - t.  Bounding sphere rb = r + t: aa = (dl0 dl0 + dl1 dl1) + dl2 dl2; bq = (o0 dl0 +
 *     o1 dl1) + o2 dl2; tcb = -bq / aa; q = o + tcb dl; h2 = rb rb - ((q0 q0 + q1 q1) + q2 q2); miss unless h2 >= 0; hs = sqrt(h2 /
 *     aa); tout = tcb + hs; tt = max(tcb - hs, znear); miss unless tt <= tout; len = sqrt(aa).  Then at most K = 64 times: v = sdf(o
 *     + tt dl); v <= eps = 1e-4: hit at depth tt, stop; else tt = tt + v / len; tt <= tout fails: miss, stop.  No hit after K: miss.
 *     Local normal: n_a = sdf(p + step e_a) - sdf(p - step e_a) at p = o + tt dl with step = 1e-4, divided by sqrt((n0 n0 + n1 n1) +
 *     n2 n2) ((0, 0, 1) when that is 0).
 *   Normal to the eye frame: ns_c = (A[0][c] nl0 + A[1][c] nl1) + A[2][c] nl2; n_r = (R[r][0] ns0 + R[r][1] ns2) + R[r][2] ns1.
 * Nearest.  Mode 0: the pixel first holds its nearest sphere, if any.  Then the primitives in index order, then the ground, each
 *   taken when the pixel holds nothing yet or its depth < the depth held: an exact tie is kept by particle, then primitive, then ground.
 *   Mode 1: the same without the particles; then the pixel's nearest point is taken when the pixel holds nothing or d < the depth held.
 * Colour.  bc = min(max(base lit, 0), 1) per channel of the opaque winner (base: particle_color RGB, prim_color, ground_color), 1 when
 *   there is none.  A point that was taken is unlit: channel = alpha pc + oma bc.  u8 = (int)(min(max(channel, 0), 1) * 255 + 0.5).
 * Outputs, NOT mirrored, as py_render.py:140-145 and :169-174 return them: color [M,H,W,3] u8 RGB, depth [M,H,W] f32 (the nearest
 *   of everything, points included; 0 when nothing) and id [M,H,W] i32 (NULL: not written): >= 0 the particle index, -1 nothing, -3 the
 *   ground, -4 - j primitive j.
 * Unspecified image, never a fault: a non-finite primitive pose, coordinates beyond 1e18 in magnitude.
 *
 * ud_mpm_render_create: prim_sizes is a HOST array [n_prims,3] of half sizes (box) or (r, h, t) (cut hollow sphere), copied into the
 *   handle (NULL when n_prims = 0).  A null argument, width / height / n_particles / max_frames < 1, n_prims < 0, yfov outside (0, pi),
 *   znear <= 0, a degenerate look_at, mode or prim_kind outside {0, 1}, radius <= 0 in mode 0, point_size < 1: UD_ERR_INVALID.  width or
 *   height > 4096, n_particles > 2^20, n_prims > 16, max_frames > 65535 or max_frames * n_particles >= 2^31 - 256: UD_ERR_UNSUPPORTED.
 *   Arena: 20 B per particle and frame, 48 B per primitive and frame, allocated here for max_frames.
 * ud_mpm_render_frames: x [M,n_particles,3], prim_pos [M,n_prims,3], prim_rot [M,n_prims,4] (both NULL when n_prims = 0), device
 *   arrays.  Two launches (k_mr_setup, k_mr_tile), no allocation, no host synchronisation.  A null handle / x / color / depth
 *   (prim_pos / prim_rot with n_prims > 0), M < 1 or M > max_frames: UD_ERR_INVALID, nothing launched, no output touched.  Results
 *   are bit-identical from run to run.
 * ------------------------------------------------------------------------------------------------ */
typedef struct ud_mpm_render ud_mpm_render;
typedef struct ud_mpm_render_conf {
  int width;                  /* 640 */
  int height;                 /* 480 */
  double yfov;                /* pi / 3 */
  double znear;               /* 0.05 */
  double camera_pos[3];       /* (0.9, 0.5, 1.0), render frame; also the pose of both lights */
  double camera_target[3];    /* (0.6, 0.5, 0.0) */
  double camera_up[3];        /* (0, 0, 1) */
  double ground_min[2];       /* (-0.02, -0.04) */
  double ground_max[2];       /* (0.98, 0.96) */
  double ground_z;            /* -0.02 */
  float particle_color[4];    /* RGBA in [0, 1]; alpha is used in point mode only */
  float prim_color[3];        /* base colours, RGB in [0, 1] */
  float ground_color[3];
  int mode;                   /* 0 spheres, 1 points */
  double radius;              /* 0.008 (mode 0) */
  int point_size;             /* 1 pixel (mode 1) */
  int n_particles;            /* N of every call */
  int n_prims;                /* primitives per frame, >= 0 */
  int prim_kind;              /* 0 box, 1 cut hollow sphere */
  int max_frames;             /* arenas are allocated for this many frames; a call with more returns UD_ERR_INVALID */
} ud_mpm_render_conf;
int ud_mpm_render_create(const ud_mpm_render_conf* conf, const float* prim_sizes, ud_mpm_render** out);
int ud_mpm_render_destroy(ud_mpm_render* h);
int ud_mpm_render_frames(ud_mpm_render* h, int M, const float* x, const float* prim_pos, const float* prim_rot, unsigned char* color,
                         float* depth, int* id, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIDOM_HIP_H */
