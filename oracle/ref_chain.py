"""ORACLE reference chain (test infrastructure only): the APG gradient of the cloth envs, restated on the CPU oracle.

A cloth env's step_diff and the APG loss written out again, independently of ClothEnv.step_diff, APG.loss and the fused
glue, so that tests can compare the gradient the product computes end to end with one from a plain implementation:
    rollout       ClothRolloutFn: forward ClothOracle.rollout_fwd (f32, the env's operation order), backward
                  ClothOracle.rollout_bwd with the adjoint in f64 (R64: the f32 trajectory's adjoint, oc_cloth_rollout_bwd_mixed)
                  or f32 (R32)
    step_diff     cloth_env.py:205-228   pick-and-place expansion :134-173 (the XLA reciprocal rule for / 3 and / 20),
                  contact distance :206-209, chamfer util.py:138-153, e ** (-10 d), the aux term, 0.99 ** cur_step, get_obs :94-132
                  (cloth_env_para.py:130 for the stiffness column; fold_cloth_tshirt_env.py:69-111 for every tenth particle)
    APG loss      apg.py:177-215   policy MLP, NormalTanhDistribution sample, sigmoid squash, -mean(rewards)

Forward values are f32 and bit-identical to what the HIP env computes from the same inputs: every quantity that feeds the
rollout (macro actions, state) is computed in f32 with the kernels' arithmetic, and the gradient flows through an expression of
the same value in the chain's own dtype (`value.detach() + (expr - expr.detach())`).  Discrete choices (the argmins) are made
on the f32 distances, as jnp makes them; the continuous arithmetic after them is in the chain's dtype.

`mutate` (a set of names) plants one of the mistakes the GPU tests must be able to see; tests/test_ref_chain.py measures how far
each moves the gradient:
    contact_grad     the contact term's gradient dropped
    discount         0.99 ** (cur_step - 1): the discount of the step before
    prim0_grad       the expansion's cotangent on primitive0 zeroed
    chamfer_yx_grad  the goal -> cloth chamfer direction's gradient dropped
    obs_detach       the observation -> policy path cut

The MPM envs whip_rope and pour_water have their own chain further down (MpmStepFn, MpmRefEnv, MPM_MUTATIONS, bar_mpm): the HIP
step sums with float atomics and is not bit-equal to the oracle, so there each chain (R64: f64 throughout, R32: f32 throughout)
runs its own forward from the same f32 input values.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as Fn

from .pyoracle import ClothOracle, MpmOracle

# `/ 3`, `/ 20` as XLA executes them under jit: multiplication by the f32 reciprocal (cloth_env.py:148-163)
_R3 = np.float32(1) / np.float32(3)
_R20 = np.float32(1) / np.float32(20)
MUTATIONS = ("contact_grad", "discount", "prim0_grad", "chamfer_yx_grad", "obs_detach")
# the bar of tests/test_grad_chain_gpu.py, per compared tensor:  |HIP - R64|max <= KAPPA * |R32 - R64|max + REL_FLOOR * |R64|max
# (KAPPA: twice the largest ratio |HIP - R64| / |R32 - R64| measured on the MI355X, 1.92; that file's docstring lists them)
KAPPA = 4.0
REL_FLOOR = 1e-6


def bar(r64, r32):
    """what the product may differ from R64 by (see KAPPA)"""
    r64, r32 = (np.asarray(t, np.float64) for t in (r64, r32))
    return KAPPA * np.abs(r32 - r64).max() + REL_FLOOR * np.abs(r64).max()


def _f32(t):
    """the f32 values of a tensor that must hold f32 values (the forward of the chain runs on them)"""
    a = t.detach().cpu().numpy()
    a32 = a.astype(np.float32)
    assert np.array_equal(a32, a), "a forward value of the reference chain is not an f32 value"
    return a32


def _st(value32, expr):
    """value32's values, expr's gradient"""
    v = torch.as_tensor(value32, dtype=expr.dtype)
    return v + (expr - expr.detach())


class ClothRolloutFn(torch.autograd.Function):
    """lax.scan(step_jax) over the macro actions on the CPU oracle: (x, v, prim [B,2,4], k, mu, actions [T,B,8]) ->
    (x, v, prim[, x_list, v_list, prim_list]).  The adjoint runs in the dtype of x (f64: along the f32 trajectory)."""

    @staticmethod
    def forward(ctx, ref, x, v, prim, k, mu, actions):
        dt = x.dtype
        if ref.forward_f64:     # finite-difference checks only: forward and adjoint both in f64
            ins = [t.detach().numpy().astype(np.float64) for t in (x, v, prim, k, mu, actions)]
        else:
            ins = [_f32(t) for t in (x, v, prim, k, mu, actions)]
        o = ref.orc.rollout_fwd(*ins, want_lists=ref.want_lists, nthreads=ref.nthreads)
        ctx.ref, ctx.ins, ctx.dt = ref, ins, dt
        keys = ("x", "v", "prim") + (("x_list", "v_list", "prim_list") if ref.want_lists else ())
        return tuple(torch.from_numpy(o[q]).to(dt) for q in keys)

    @staticmethod
    def backward(ctx, *g):
        ref, dt = ctx.ref, ctx.dt
        npdt = np.float64 if dt == torch.float64 else np.float32
        x, v, prim, k, mu, actions = ctx.ins
        z = lambda t, like: np.zeros(like.shape, npdt) if t is None else t.detach().numpy().astype(npdt)
        gx, gv, gp = z(g[0], x), z(g[1], v), z(g[2], prim)
        T = actions.shape[0]
        lists = [None, None, None]
        if ref.want_lists:
            lists = [None if t is None else t.detach().numpy().astype(npdt) for t in g[3:6]]
        r = ref.orc.rollout_bwd(x, v, prim, k, mu, actions, gx, gv, gp, *lists, normalize=ref.normalize,
                                nthreads=ref.nthreads, adjoint_dtype=None if ref.forward_f64 else npdt)
        if "flips" in r:
            ref.flips += r["flips"]
        t = lambda q: torch.from_numpy(np.ascontiguousarray(r[q])).to(dt)
        return None, t("gx"), t("gv"), t("gprim"), t("gk"), t("gmu"), t("gactions")


class ClothRefEnv:
    """A cloth env's step_diff on the CPU oracle in the chain's dtype (torch.float64: R64, torch.float32: R32).
    State: dict x [B,P,3], v, primitive0 [B,4], primitive1, stiffness [B], mu [B] (tensors of the chain's dtype holding f32
    values) and cur_step (int numpy [B])."""

    def __init__(self, conf, mask, goal, max_steps, dtype=torch.float64, aux_reward=True, eval_min_max_stiff=None,
                 obs_stride=1, order=2, substeps=None, normalize=True, use_substep_obs=None, nthreads=1, mutate=()):
        self.dtype = dtype
        self.conf = conf
        self.substeps = int(getattr(conf, "substeps", 50) if substeps is None else substeps)
        self.orc = ClothOracle(np.asarray(mask), N=conf.N, gravity=conf.gravity, damping=conf.damping, dt=conf.dt,
                               max_v=conf.max_v, small_num=conf.small_num, substeps=self.substeps, order=order)
        self.goal32 = np.ascontiguousarray(goal, dtype=np.float32)
        self.goal = torch.from_numpy(self.goal32).to(dtype)
        self.max_steps, self.aux_reward = max_steps, aux_reward
        self.eval_min_max_stiff = eval_min_max_stiff
        self.obs_stride = obs_stride
        self.normalize = normalize
        self.want_lists = bool(conf.use_substep_obs if use_substep_obs is None else use_substep_obs)
        self.nthreads = nthreads
        self.mutate = set(mutate)
        assert self.mutate <= set(MUTATIONS), self.mutate
        self.forward_f64 = False    # ClothRolloutFn's forward in f64 too (finite-difference checks of its wiring)
        self.flips = 0              # grasp decisions the f64 adjoint sweep saw otherwise (it follows the f32 forward)
        self.check_pnp = None       # optional callback (actions32, primitive0_32, x32) -> (macro, contact) of the product, compared bit for bit

    @classmethod
    def from_env(cls, env, dtype=torch.float64, nthreads=1, mutate=()):
        """the reference of a constructed ClothEnv (its conf, mask, goal and the operation order its handle really runs:
        ClothSimulator.forward_order -- not the mode alone, bodies of 513-1024 particles run the reference order in every mode)"""
        sim = env.simulator
        return cls(env.conf, np.asarray(env.cloth_mask), env.goal.cpu().numpy(), env.max_steps, dtype=dtype, aux_reward=env.aux_reward,
                   eval_min_max_stiff=env.eval_min_max_stiff, obs_stride=10 if env.conf.task == "fold_tshirt" else 1,
                   order=sim.forward_order, substeps=sim.substeps, normalize=sim.normalize_grad, nthreads=nthreads,
                   mutate=mutate)

    def state_from(self, st, **leaves):
        """a reference state from a ClothState (device tensors); `leaves` replaces fields by tensors of the chain's dtype"""
        c = lambda t: torch.from_numpy(t.detach().cpu().numpy()).to(self.dtype)
        s = dict(x=c(st.x), v=c(st.v), primitive0=c(st.primitive0), primitive1=c(st.primitive1),
                 stiffness=c(st.stiffness.to(torch.float32)), mu=c(st.mu), cur_step=st.cur_step.cpu().numpy().astype(np.int64))
        s.update(leaves)
        return s

    squash = True       # apg.py:185: the cloth envs take sigmoid(tanh sample)

    def obs_of(self, s):
        return self.get_obs(s["x"], s["primitive0"], s["primitive1"], s["stiffness"])

    # -- get_obs (cloth_env.py:94-132) -----------------------------------------------------------------------------------
    def get_obs(self, x, primitive0, primitive1, stiffness):
        lead = x.shape[:-2]
        parts = [x[..., ::self.obs_stride, :].reshape(lead + (-1,)), primitive0, primitive1]
        if self.eval_min_max_stiff is not None:      # cloth_env_para.py:130
            lo, hi = float(self.eval_min_max_stiff[0]), float(self.eval_min_max_stiff[1])
            parts.append((stiffness[..., None] - lo) / (hi - lo))
        return torch.cat(parts, -1)

    # -- get_pnp_actions (cloth_env.py:134-173) and contact_distance (:206-209) --------------------------------------------
    def pnp(self, actions, primitive0, x):
        B = actions.shape[0]
        a32, p32, x32 = _f32(actions), _f32(primitive0), _f32(x)
        # f32 values, the kernels' arithmetic
        m32 = np.zeros((40, B, 8), np.float32)
        m32[0:3, :, 0] = (a32[:, 0] - p32[:, 0]) * _R3
        m32[0:3, :, 1] = (np.float32(0) - p32[:, 1]) * _R3
        m32[0:3, :, 2] = (a32[:, 2] - p32[:, 2]) * _R3
        m32[0:3, :, 3] = 1
        m32[3:13, :, 1] = np.float32(0.06) / np.float32(10)
        m32[13:33, :, 0] = (a32[:, 3] - a32[:, 0]) * _R20
        m32[13:33, :, 2] = (a32[:, 5] - a32[:, 2]) * _R20
        m32[33:40, :, 3] = 1
        d = a32[:, None, :3] - x32
        s32 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        idx = np.argmin(s32, 1)                                         # the first minimum
        c32 = np.sqrt(s32[np.arange(B), idx])
        if self.check_pnp is not None:
            macro_p, contact_p = self.check_pnp(a32, p32, x32)
            assert np.array_equal(macro_p, m32), "macro actions differ from the product's"
            assert np.array_equal(contact_p, c32), "contact distance differs from the product's"
        # the same expressions in the chain's dtype, for the gradient
        p0 = primitive0.detach() if "prim0_grad" in self.mutate else primitive0
        z = torch.zeros_like(actions[:, 0])
        down = torch.stack([(actions[:, 0] - p0[:, 0]) * float(_R3), (z - p0[:, 1]) * float(_R3),
                            (actions[:, 2] - p0[:, 2]) * float(_R3)], -1)
        move = torch.stack([(actions[:, 3] - actions[:, 0]) * float(_R20), z, (actions[:, 5] - actions[:, 2]) * float(_R20)], -1)
        g = torch.cat([down[None].expand(3, B, 3), torch.zeros((10, B, 3), dtype=actions.dtype),
                       move[None].expand(20, B, 3), torch.zeros((7, B, 3), dtype=actions.dtype)], 0)
        g = torch.cat([g, torch.zeros((40, B, 5), dtype=actions.dtype)], -1)
        macro = _st(m32, g)
        xi = x[torch.arange(B), torch.as_tensor(idx)]
        contact = torch.sqrt(((actions[:, :3] - xi) ** 2).sum(-1))
        return macro, contact

    # -- calc_chamfer (util.py:138-153) ------------------------------------------------------------------------------------
    def chamfer(self, x):
        x32, y32 = _f32(x), self.goal32
        B = x32.shape[0]
        ixy, iyx = [], []
        for b in range(B):
            d = x32[b][:, None, :] - y32[None]
            m = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) / np.float32(3)
            ixy.append(np.argmin(m, 1))
            iyx.append(np.argmin(m, 0))
        ixy, iyx = torch.as_tensor(np.stack(ixy)), torch.as_tensor(np.stack(iyx))
        bi = torch.arange(B)[:, None]
        y = self.goal
        x2y = torch.sqrt(((x - y[ixy]) ** 2).mean(-1)).mean(1)
        xs = x.detach() if "chamfer_yx_grad" in self.mutate else x
        y2x = torch.sqrt(((xs[bi, iyx] - y[None]) ** 2).mean(-1)).mean(1)
        return y2x + x2y

    # -- step_diff (cloth_env.py:201-231) ----------------------------------------------------------------------------------
    def step(self, actions, s):
        """-> (obs, reward, new state, obs_list)"""
        macro, contact = self.pnp(actions, s["primitive0"], s["x"])
        prim = torch.stack([s["primitive0"], s["primitive1"]], 1)
        out = ClothRolloutFn.apply(self, s["x"], s["v"], prim, s["stiffness"], s["mu"], macro)
        x, v, p = out[:3]
        cur = s["cur_step"] + 1
        new = dict(x=x, v=v, primitive0=p[:, 0], primitive1=p[:, 1], stiffness=s["stiffness"], mu=s["mu"], cur_step=cur)
        obs = self.get_obs(x, p[:, 0], p[:, 1], s["stiffness"])
        obs_list = None
        if self.want_lists:
            xl, pl = out[3], out[5]
            obs_list = self.get_obs(xl, pl[:, :, 0], pl[:, :, 1], s["stiffness"][None].expand(xl.shape[0], -1))
        reward = torch.exp(self.chamfer(x) * -10.0)
        if self.aux_reward:
            reward = reward + torch.exp(-(contact.detach() if "contact_grad" in self.mutate else contact))
        n = cur - 1 if "discount" in self.mutate else cur
        reward = reward * torch.as_tensor(0.99 ** n.astype(np.float64), dtype=self.dtype)
        return obs, reward, new, obs_list


# -- the APG loss (apg.py:177-215) ---------------------------------------------------------------------------------------
class PolicyRef:
    """the policy MLP (apg.py:353-358, swish between Dense layers) on a copy of the parameters in `dtype`"""

    def __init__(self, params, dtype):
        self.params = [torch.tensor(p.detach().cpu().numpy(), dtype=dtype, requires_grad=True) for p in params]

    def __call__(self, obs):
        h = obs
        n = len(self.params) // 2
        for i in range(n):
            h = Fn.linear(h, self.params[2 * i], self.params[2 * i + 1])
            if i < n - 1:
                h = h * torch.sigmoid(h)
        return h


def tanh_sample(logits, eps, min_std=0.001):
    """NormalTanhDistribution.sample (apg.py:98-100, :184): tanh(loc + (softplus(raw) + min_std) * eps)"""
    loc, raw = torch.chunk(logits, 2, dim=-1)
    return torch.tanh(loc + (Fn.softplus(raw) + min_std) * eps)


def apg_loss(env_ref, policy, state, noise, action_values=None):
    """-mean(rewards) of len(noise) scanned do_one_step calls.  action_values[t] (f32 [B,6]), when given, are the values the
    actions take (the product's, so that the forward is the product's bit for bit); the gradient flows through the
    reference policy's own expression.  Without them the chain's action values are used (a cloth chain needs f32 values there;
    the MPM chains always run on their own).  env_ref.obs_of(state) is the observation, env_ref.squash says whether the env takes
    sigmoid(sample) or the raw tanh sample (apg.py:185; core.py::squashes_actions)."""
    rewards, acts = [], []
    s = state
    for t in range(len(noise)):
        obs = env_ref.obs_of(s)
        if "obs_detach" in env_ref.mutate:
            obs = obs.detach()
        a = tanh_sample(policy(obs), torch.as_tensor(np.asarray(noise[t]), dtype=env_ref.dtype))
        if env_ref.squash:
            a = torch.sigmoid(a)
        if action_values is not None:
            a = _st(np.asarray(action_values[t], np.float32), a)
        acts.append(a)
        _, reward, s, _ = env_ref.step(a, s)
        rewards.append(reward)
    rewards = torch.stack(rewards)
    return -rewards.mean(), rewards, acts


def adam_first_step(params, grads, lr, max_gradient_norm, b1=0.9, b2=0.999, eps=1e-8):
    """clip_by_global_norm, then the first optax.adam step from zero moments (apg.py:217-267): the clipped gradient and the
    parameter update"""
    flat = torch.cat([g.reshape(-1) for g in grads])
    flat = torch.nan_to_num(flat)
    nrm = torch.linalg.vector_norm(flat)
    clipped = flat * (max_gradient_norm / nrm if nrm >= max_gradient_norm else 1.0)
    m = (1 - b1) * clipped / (1 - b1)
    v = (1 - b2) * clipped * clipped / (1 - b2)
    return clipped, -lr * m / (torch.sqrt(v) + eps)


def cloth_reset_state(conf, mask, B, key, dtype=torch.float64):
    """ClothEnv.reset without a GPU (cloth_simulator.py:339-364, cloth_env.py:181-185): the flat lattice, shifted in x and z by
    normal(split(key)[0], 2) * 0.05 in f32"""
    from unidom_amd.utils import prng
    N = conf.N
    c = 1.0 / N
    ii, jj = np.nonzero(np.asarray(mask))
    x = np.stack([ii * c, np.zeros_like(ii, dtype=np.float64), (N - jj) * c], -1).astype(np.float32)
    k = prng.split(np.asarray(key, dtype=np.uint32))[0]
    shift = prng.normal(k, 2) * np.float32(0.05)
    x[:, 0] += np.float32(shift[0])
    x[:, 2] += np.float32(shift[1])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.repeat(np.asarray(a, np.float32)[None], B, 0))).to(dtype)
    return dict(x=t(x), v=t(np.zeros_like(x)), primitive0=t([0.5, 0.5, 0.5, 0.01]), primitive1=t([1.0, 1.0, 1.0, 0.01]),
                stiffness=t(np.float32(conf.stiffness)), mu=t(np.float32(conf.mu)), cur_step=np.zeros(B, np.int64))


# == the MPM envs whip_rope and pour_water ================================================================================
#   step_diff     mpm_env.py:99-125 focus shift and un-shift, :130-167 scan of simulator.step, nan_to_num, reward :90-94, get_obs :57-76
#   actions       whip_rope_env.py:108-115, pour_water_env.py:77-90 (`/ 50.0`, `/ 500.0` as XLA executes them: the f32 reciprocal)
#   simulator     MpmOracle.step_fwd / step_bwd (mpm_simulator.py:413-429, the step-boundary clip :375-411)
# The product's step sums with float atomics, so nothing here is bit-equal to it: R64 is this chain in f64 throughout, R32 in f32
# throughout, both from the same f32 input values, and the bar is bar_mpm below.
_R50 = np.float32(1) / np.float32(50)
_R500 = np.float32(1) / np.float32(500)
MPM_MUTATIONS = ("shift_grad", "unshift_pos_grad", "carry_F_detach", "carry_pos_detach", "obs_v_detach", "obs_detach", "reward_mean3")
# what float-atomic order and the Jacobi SVD add over a sequential f32 sum: twice the largest residual
# (|HIP - R64|max - KAPPA |R32 - R64|max) / |R64|max measured on the MI355X, rounded up to one digit, never above 2e-2 (the relative
# tolerance the step-level tests hold the 70-substep adjoint to) and never raised.  It was 2e-2 while svd3 left its sweeps too early
# (residual 8.81e-3 on whip_rope's F0 gradient at the reset state, F = I); with the exit at round-off level that residual is -4.04e-3 and
# every asserted tensor's is negative (tests/test_grad_chain_mpm_gpu.py lists them): KAPPA |R32 - R64| alone covers the product.
FLOOR_MPM = 0.0


def bar_mpm(r64, r32):
    """what the product's MPM gradient may differ from R64 by: KAPPA |R32 - R64|max + FLOOR_MPM |R64|max"""
    r64, r32 = (np.asarray(t, np.float64) for t in (r64, r32))
    return KAPPA * np.abs(r32 - r64).max() + FLOOR_MPM * np.abs(r64).max()


class MpmStepFn(torch.autograd.Function):
    """one simulator.step on the CPU oracle in the dtype of x: (x, v, C, F, J, positions [B,P,S,3], rotations [B,P,S,4],
    sizes [B,P,3], friction, mu, lamda [B], action [B,6P]) -> (x, v, C, F, J, positions, rotations)"""

    @staticmethod
    def forward(ctx, ref, x, v, C, F, J, pos, rot, size, friction, mu, lamda, action):
        dt = x.dtype
        npdt = np.float64 if dt == torch.float64 else np.float32
        c = lambda t: np.ascontiguousarray(t.detach().numpy(), dtype=npdt)
        one = ref.n_prim == 1                   # the oracle takes no primitive axis then
        p = lambda t: c(t[:, 0]) if one else c(t)
        st = dict(x=c(x), v=c(v), C=c(C), F=c(F), J=c(J), ppos=p(pos), prot=p(rot), psize=p(size), friction=c(friction), mu=c(mu),
                  lamda=c(lamda), action=c(action))
        o = ref.orc.step_fwd(st, nthreads=ref.nthreads)
        ctx.ref, ctx.st, ctx.dt = ref, st, dt
        t = lambda a: torch.from_numpy(a).to(dt)
        q = lambda a: t(a[:, None]) if one else t(a)
        out = (t(o["x"]), t(o["v"]), t(o["C"]), t(o["F"]), t(o["J"]), q(o["ppos"]), q(o["prot"]))
        ctx.mark_non_differentiable(out[4], *((out[6],) if ref.position_control else ()))
        return out

    @staticmethod
    def backward(ctx, gx, gv, gC, gF, gJ, gpos, grot):
        ref, st = ctx.ref, ctx.st
        npdt = st["x"].dtype
        one = ref.n_prim == 1
        z = lambda g, like: np.zeros(like.shape, npdt) if g is None else np.ascontiguousarray(g.detach().numpy(), dtype=npdt)
        p = lambda g, like: z(None if g is None else (g[:, 0] if one else g), like)
        g = dict(gx=z(gx, st["x"]), gv=z(gv, st["v"]), gC=z(gC, st["C"]), gF=z(gF, st["F"]), gppos=p(gpos, st["ppos"]))
        if not ref.position_control:
            g["gprot"] = p(grot, st["prot"])
        r = ref.orc.step_bwd(st, g, clip=ref.clip, nthreads=ref.nthreads)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.dt)
        q = lambda a: t(a[:, None]) if one else t(a)
        grot_in = None if ref.position_control else q(r["gprot"])
        return (None, t(r["gx"]), t(r["gv"]), t(r["gC"]), t(r["gF"]), None, q(r["gppos"]), grot_in, None, t(r["gfriction"]),
                t(r["gmu"]), t(r["glamda"]), t(r["gaction"]))


class MpmRefEnv:
    """whip_rope's or pour_water's step_diff on the CPU oracle in the chain's dtype.  State: dict x [B,N,3], v, C, F [B,N,3,3],
    J [B,N], pos [B,P,S,3], rot [B,P,S,4], size [B,P,3], friction, mu, lamda [B] (tensors of the chain's dtype holding f32 values),
    cur_step (int numpy [B]) and carried (the state came out of a step: the carry mutations apply to it)."""

    squash = False      # apg.py:185: whip_rope and pour_water take the raw tanh sample

    def __init__(self, task, N, goal, n_grid, res, steps, dt, max_steps, p_rho=1.0, gravity=(0, -9.8, 0), material=None, hardness=None,
                 n_prim=1, sdf="box", prim_friction=0.1, prim_softness=666.0, position_control=True, clip=True, dtype=torch.float64,
                 nthreads=1, mutate=()):
        assert task in ("whip_rope", "pour_water"), task
        self.task, self.dtype, self.nthreads = task, dtype, nthreads
        self.n_prim, self.position_control, self.clip = n_prim, bool(position_control), bool(clip)
        self.orc = MpmOracle(N, n_grid=n_grid, res=tuple(res), steps=steps, dt=dt, p_rho=p_rho, gravity=gravity,
                             position_control=position_control, material=material, hardness=hardness, prim_friction=prim_friction,
                             prim_softness=prim_softness, n_prim=n_prim, sdf=sdf)
        self.goal = torch.from_numpy(np.ascontiguousarray(goal, dtype=np.float32)).to(dtype)
        assert self.goal.shape in ((N, 3), (1, 3))
        # jnp.array(conf.res) * 0.5 / conf.n_grid (mpm_env.py:102), an f32 value
        self.center = torch.from_numpy(np.asarray(res, np.float32) * np.float32(0.5) / np.float32(n_grid)).to(dtype)
        self.max_steps = max_steps
        self.mutate = set(mutate)
        assert self.mutate <= set(MPM_MUTATIONS), self.mutate

    @classmethod
    def from_env(cls, env, dtype=torch.float64, nthreads=1, mutate=()):
        """the reference of a constructed (and reset) WhipRopeEnv / PourWaterEnv: conf, goal, particle count, material, primitives,
        SDF kind, per-primitive friction / softness and the clip flag its simulator hands to the step's backward"""
        conf, sim = env.conf, env.simulator
        each = lambda v, one: list(v) if len(v) else one
        return cls(conf.task, sim.n_particles, env.goal.cpu().numpy(), conf.n_grid, conf.res, conf.steps, conf.dt, env.max_steps,
                   p_rho=conf.p_rho, gravity=conf.gravity, material=np.asarray(sim.material), hardness=np.asarray(sim.h),
                   n_prim=sim.n_primitive, sdf=sim.sdf_kind, prim_friction=each(sim.prim_friction_each, sim.prim_friction),
                   prim_softness=each(sim.prim_softness_each, sim.prim_softness), position_control=sim.use_position_control,
                   clip=sim.clip_grad, dtype=dtype, nthreads=nthreads, mutate=mutate)

    def state_from(self, st, **leaves):
        """a reference state from an MPMState (device tensors); `leaves` replaces fields by tensors of the chain's dtype"""
        c = lambda t: torch.from_numpy(t.detach().cpu().numpy()).to(self.dtype)
        B = st.x.shape[0]
        stack = lambda k: torch.stack([c(getattr(q, k)) for q in st.primitives], 1)
        s = dict(x=c(st.x), v=c(st.v), C=c(st.C), F=c(st.F), J=c(st.J), pos=stack("position"), rot=stack("rotation"), size=stack("size"),
                 friction=c(st.friction).reshape(B), mu=c(st.mu).reshape(B), lamda=c(st.lamda).reshape(B),
                 cur_step=st.cur_step.cpu().numpy().astype(np.int64), carried=False)
        s.update(leaves)
        return s

    # -- get_obs (mpm_env.py:57-76) ------------------------------------------------------------------------------------------
    def obs_of(self, s):
        B = s["x"].shape[0]
        v = s["v"].detach() if "obs_v_detach" in self.mutate else s["v"]
        return torch.cat([s["x"].reshape(B, -1), v.reshape(B, -1), s["pos"][:, 0].reshape(B, -1)], -1)

    # -- get_primitive_actions (whip_rope_env.py:108-115, pour_water_env.py:77-90) -> [T,B,6P] -----------------------------------
    def primitive_actions(self, a):
        if self.task == "whip_rope":
            a = a + 1e-12
            a = a * float(_R50)
            a = torch.cat([a[..., :3], torch.zeros_like(a[..., 3:])], -1)
            return a[None]
        a = torch.cat([a, torch.zeros_like(a)], -1)
        a = torch.cat([a[..., :6] * float(_R500), a[..., 6:]], -1)
        a = a + 1e-12
        a = torch.cat([a[..., :1], torch.zeros_like(a[..., :1]), a[..., 2:]], -1)
        return a[None]

    # -- step_diff (mpm_env.py:130-167) ----------------------------------------------------------------------------------------
    def step(self, actions, s):
        """-> (obs, reward, new state, None)"""
        m = self.mutate
        n2n = lambda t: torch.where(torch.isfinite(t), t, torch.nan_to_num(t.detach()))      # jnp.nan_to_num: a select
        x, v, C, F, J, pos, rot = (s[k] for k in ("x", "v", "C", "F", "J", "pos", "rot"))
        carried = s["carried"]
        # pre_step :99-114
        shift = self.center - x.mean(1)
        shift = torch.stack([shift[:, 0], torch.zeros_like(shift[:, 0]), shift[:, 2]], -1)
        if "shift_grad" in m:
            shift = shift.detach()
        acts = self.primitive_actions(actions)
        for t in range(acts.shape[0]):                       # lax.scan(simulator.step_jax, ...)
            if carried:
                F = F.detach() if "carry_F_detach" in m else F
                pos = pos.detach() if "carry_pos_detach" in m else pos
            if t == 0:
                x, pos = x + shift[:, None], pos + shift[:, None, None]
            x, v, C, F, J, pos, rot = MpmStepFn.apply(self, x, v, C, F, J, pos, rot, s["size"], s["friction"], s["mu"], s["lamda"], acts[t])
            carried = True
        cur = s["cur_step"] + 1
        assert (cur < self.max_steps).all(), "the chain has no auto_reset: stay inside the episode"
        # post_step :116-125, nan_to_num :150-154
        x = x - shift[:, None]
        pos = pos - shift[:, None, None]
        if "unshift_pos_grad" in m:
            pos = pos.detach()
        x, v, C, F, J = n2n(x), n2n(v), n2n(C), n2n(F), n2n(J)
        # reward_func :90-94, calc_l2 util.py:156-159
        sq = (x - self.goal[None]) ** 2
        reward = math.e ** (-torch.sqrt(sq.mean(-1)).mean(-1) * 10)
        if "reward_mean3" in m:
            wrong = math.e ** (-torch.sqrt(sq.sum(-1)).mean(-1) * 10)
            reward = reward.detach() + (wrong - wrong.detach())
        new = dict(s, x=x, v=v, C=C, F=F, J=J, pos=pos, rot=rot, cur_step=cur, carried=True)
        return self.obs_of(new), reward, new, None
