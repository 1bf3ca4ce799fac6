"""CPU: the MPM reference chain of tests/test_grad_chain_mpm_gpu.py checked on its own (oracle/ref_chain.py: MpmStepFn, MpmRefEnv).

Nothing of the product runs here.  Inputs: the recorded whip_rope states of tests/golden/whip_rope_demo0.npz with the gripper put on
rope particle 5 (position control, "rope"), and test_oracle_mpm._two_bowl_case(turning=False) -- 67 liquid particles between two
container primitives in soft contact ("bowls"), driven with pour_water's actions.
  finite differences   the f64 chain's gradient over two env steps equals central differences of its own forward
  conditioning         the rope cases are far from the noise: |R32 - R64|max <= 5 % of |R64|max
  mutations            each mistake planted through `mutate` moves a compared gradient by at least ten times bar_mpm
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import ref_chain as rc
from test_oracle_mpm import _two_bowl_case

NTHREADS = 4
ROPE_STATES = [0, 20, 40, 60]
E, NU = 100, 0.1                       # whip_rope_env.py:27-73
MU0, LA0 = E / (2 * (1 + NU)), E * NU / ((1 + NU) * (1 - 2 * NU))
LEAVES = ("x", "v", "F", "pos")


@pytest.fixture(scope="module")
def demo():
    return np.load(os.path.join(GOLDEN, "whip_rope_demo0.npz"))


@pytest.fixture(scope="module")
def goal():
    return np.load(os.path.join(GOLDEN, "goal_whip_rope.npy"))


def _rope(demo, goal, dtype, steps=70, clip=True, mutate=(), ks=ROPE_STATES, F_noise=0.0):
    """-> (reference env, state of f32 values in `dtype` whose x, v, F, pos are fresh leaves).  F_noise: the recorded F is almost
    isotropic, where the SVD's adjoint (1 / (s_i^2 - s_j^2), clamped) is not the derivative of anything; the finite-difference
    check moves it off that point as test_oracle_mpm._adjoint_case does."""
    ref = rc.MpmRefEnv("whip_rope", 67, goal, 64, (32, 32, 32), steps, 1e-4, 70, clip=clip, dtype=dtype, nthreads=NTHREADS, mutate=mutate)
    B = len(ks)
    leaf = lambda a: torch.tensor(np.asarray(a, np.float32), dtype=dtype, requires_grad=True)
    const = lambda a: torch.tensor(np.asarray(a, np.float32), dtype=dtype)
    pos = np.zeros((B, 1, steps, 3), np.float32)
    pos[:, 0, 0] = demo["x"][ks, 5]                      # the gripper on the rope: control touches occupied cells
    rot = np.zeros((B, 1, steps, 4), np.float32)
    rot[..., 0] = 1
    F = demo["F"][ks] + np.random.default_rng(1).normal(size=(B, 67, 3, 3)) * F_noise
    s = dict(x=leaf(demo["x"][ks]), v=leaf(demo["v"][ks]), C=const(demo["C"][ks]), F=leaf(F), J=const(demo["J"][ks]),
             pos=leaf(pos), rot=const(rot), size=const(np.full((B, 1, 3), 0.02)), friction=const(np.full(B, 0.1)),
             mu=const(np.full(B, MU0)), lamda=const(np.full(B, LA0)), cur_step=np.zeros(B, np.int64), carried=False)
    return ref, s


def _bowls(demo, goal, dtype, steps=23, clip=True, mutate=()):
    st, _ = _two_bowl_case(demo, steps, 40, 0, np.float32, turning=False)
    ref = rc.MpmRefEnv("pour_water", 67, goal, 64, (32, 32, 32), steps, 1e-4, 100, material=np.zeros(67), n_prim=2, sdf="container",
                       position_control=False, clip=clip, dtype=dtype, nthreads=NTHREADS, mutate=mutate)
    leaf = lambda a: torch.tensor(np.asarray(a, np.float32), dtype=dtype, requires_grad=True)
    const = lambda a: torch.tensor(np.asarray(a, np.float32), dtype=dtype)
    s = dict(x=leaf(st["x"]), v=leaf(st["v"]), C=const(st["C"]), F=leaf(st["F"]), J=const(st["J"]), pos=leaf(st["ppos"]),
             rot=const(st["prot"]), size=const(st["psize"]), friction=const(st["friction"]), mu=const(st["mu"]), lamda=const(st["lamda"]),
             cur_step=np.zeros(1, np.int64), carried=False)
    return ref, s


SETTINGS = {"rope": _rope, "bowls": _bowls}


def _actions(name, T, B):
    rng = np.random.default_rng(7 if name == "rope" else 8)
    return rng.uniform(-1, 1, size=(T, B, 6)).astype(np.float32)


def _cotangents(name, ref, s, T):
    """seeded random cotangents for the obs of every step and the final x, v, F, positions"""
    rng = np.random.default_rng(11 if name == "rope" else 12)
    B = s["x"].shape[0]
    obs = rng.normal(size=(T, B, ref.obs_of(s).shape[1]))
    return dict(obs=obs, **{k: rng.normal(size=tuple(s[k].shape)) for k in LEAVES})


def _step_loss(ref, s, A, cots, w):
    """T step_diff calls: sum of the rewards + w (<obs_t, c_t> for every step, <x, v, F, pos of the final state, c>)"""
    t64 = lambda a: torch.tensor(a, dtype=ref.dtype)
    loss = 0
    for t in range(A.shape[0]):
        obs, reward, s, _ = ref.step(A[t], s)
        loss = loss + reward.sum() + w * (obs * t64(cots["obs"][t])).sum()
    return loss + w * sum((s[k] * t64(cots[k])).sum() for k in LEAVES)


def _step_grads(name, demo, goal, dtype, mutate=(), T=2, w=1e-3, **kw):
    """-> dict of the gradients of _step_loss with respect to actions [T,B,6] and the initial x, v, F, pos"""
    ref, s = SETTINGS[name](demo, goal, dtype, mutate=mutate, **kw)
    A = torch.tensor(_actions(name, T, s["x"].shape[0]), dtype=dtype, requires_grad=True)
    cots = _cotangents(name, ref, s, T)
    g = torch.autograd.grad(_step_loss(ref, s, A, cots, w), [A] + [s[k] for k in LEAVES])
    return dict(zip(("actions",) + LEAVES, (t.double().numpy() for t in g)))


def _policy_params(obs_size, seed=3, hidden=32):
    """a small policy MLP obs -> hidden -> 2 x 6 (lecun-uniform kernels, small random biases), torch's [out, in] layout"""
    rng = np.random.default_rng(seed)
    sizes = [obs_size, hidden, 12]
    params = []
    for i in range(2):
        params.append(torch.tensor(rng.uniform(-1, 1, size=(sizes[i + 1], sizes[i])) * np.sqrt(3.0 / sizes[i]), dtype=torch.float32))
        params.append(torch.tensor(rng.normal(size=sizes[i + 1]) * 0.1, dtype=torch.float32))
    return params


def _apg_grad(name, demo, goal, dtype, mutate=(), T=2, **kw):
    """the flat policy gradient of rc.apg_loss over T steps"""
    ref, s = SETTINGS[name](demo, goal, dtype, mutate=mutate, **kw)
    B = s["x"].shape[0]
    pol = rc.PolicyRef(_policy_params(ref.obs_of(s).shape[1]), dtype)
    noise = np.random.default_rng(5).normal(size=(T, B, 6)).astype(np.float32)
    loss, _, _ = rc.apg_loss(ref, pol, s, noise)
    return torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss, pol.params)]).double().numpy()


@pytest.mark.parametrize("name", ["rope", "bowls"])
def test_chain_gradient_passes_directional_finite_differences(demo, goal, name):
    """R64 with clip=False (the step-boundary clip is not a derivative) and 2 substeps per step, T = 2 env steps, cotangents of
    weight 1 on the rewards, both observations and the final x, v, F and positions: for actions, x0, v0, F0 (and the primitive
    positions of the bowls) in turn, a random direction d, (L(. + h d) - L(. - h d)) / 2h against <grad, d>, to
    2e-5 max(1, |fd|, |an|) as test_oracle_mpm.test_adjoint_vs_finite_differences_f64.  This is the chain's own wiring: shift, carry
    between the two steps, un-shift, reward, obs."""
    T, kw = 2, dict(steps=2, clip=False, **(dict(F_noise=0.05) if name == "rope" else {}))
    ref, s0 = SETTINGS[name](demo, goal, torch.float64, **kw)
    B = s0["x"].shape[0]
    a0 = torch.tensor(_actions(name, T, B), dtype=torch.float64)
    cots = _cotangents(name, ref, s0, T)
    names = ("actions",) + LEAVES[:3] + (("pos",) if name == "bowls" else ())
    base = dict(actions=a0, **{k: s0[k].detach() for k in LEAVES})

    def L(vals):
        s = dict(s0, **{k: vals[k] for k in LEAVES})
        return _step_loss(ref, s, vals["actions"], cots, 1.0)

    leaves = {k: v.clone().requires_grad_(True) for k, v in base.items()}
    grads = dict(zip(leaves, torch.autograd.grad(L(leaves), list(leaves.values()))))
    rng = np.random.default_rng(2)
    for k in names:
        d = torch.tensor(rng.normal(size=tuple(base[k].shape)))
        if k == "pos":
            d[:, :, 1:] = 0                  # rows past the first are overwritten by forward kinematics
        if k == "actions" and name == "rope":
            assert (grads[k][..., 3:] == 0).all()
        h = 1e-6 * max(1.0, float(base[k].abs().max()))
        with torch.no_grad():
            fd = (float(L(dict(base, **{k: base[k] + h * d}))) - float(L(dict(base, **{k: base[k] - h * d})))) / (2 * h)
        an = float((grads[k] * d).sum())
        print(f"FD_MPM {name}/{k}: fd {fd:.9e}  an {an:.9e}  |fd-an| {abs(fd - an):.2e}")
        assert abs(fd - an) <= 2e-5 * max(1.0, abs(fd), abs(an)), (k, fd, an)


@pytest.mark.parametrize("T", [1, 3])
def test_rope_cases_are_well_conditioned(demo, goal, T):
    """-mean(rewards) of T steps of 70 substeps with the env's clip, recorded states 0/20/40/60: the f32 chain's gradient with
    respect to actions, x0, v0 and F0 is within 5 % of the f64 chain's (measured: see the print), a wide guard against a case that
    drifted into noise.  The start position of the gripper gets exactly zero."""
    g = {}
    for dtype in (torch.float64, torch.float32):
        ref, s = _rope(demo, goal, dtype)
        A = torch.tensor(_actions("rope", T, len(ROPE_STATES)), dtype=dtype, requires_grad=True)
        rewards, cur = [], s
        for t in range(T):
            _, r, cur, _ = ref.step(A[t], cur)
            rewards.append(r)
        loss = -torch.stack(rewards).mean()
        *g[dtype], gpos = torch.autograd.grad(loss, [A, s["x"], s["v"], s["F"], s["pos"]], allow_unused=True)
        g[dtype] = [t.double().numpy() for t in g[dtype]]
        # position control: the start position never reaches the particles, so the rewards give it no gradient at all (a cotangent
        # on the trajectory itself -- obs holds it -- passes straight through; the mutation test below has one)
        assert gpos is None or (gpos == 0).all()
    for k, a, b in zip(("actions", "x", "v", "F"), g[torch.float64], g[torch.float32]):
        rel = np.abs(b - a).max() / np.abs(a).max()
        print(f"COND_MPM rope T={T} {k}: |R64| {np.abs(a).max():.3e}  |R32-R64|/|R64| {rel:.2e}")
        assert np.abs(a).max() > 0 and rel <= 0.05, (k, rel)


def _step_grads_w1(name, demo, goal, dtype, mutate=(), **kw):
    """one step_diff with cotangents of weight 1 (not 1e-3) on obs and the final state"""
    return _step_grads(name, demo, goal, dtype, mutate=mutate, T=1, w=1.0, **kw)


KINDS = (("step", _step_grads), ("apg", _apg_grad), ("step_w1", _step_grads_w1))


def test_each_planted_mistake_moves_a_compared_gradient_far_past_the_gpu_bar(demo, goal):
    """For the rope (recorded states 0 and 40) and the bowls (B = 1): the APG flat gradient over 2 steps ("apg"), the step_diff leaf
    gradients (actions, x0, v0, F0, positions) over 2 steps with random cotangents of weight 1e-3 on obs and the final state and 1 on
    the rewards ("step": the weights of the GPU test), and over 1 step with weight 1 everywhere ("step_w1"), in R64, R32 and R64
    with each entry of MPM_MUTATIONS planted.  Each mistake must move at least one of them by >= 10 x bar_mpm(R64, R32), the bar
    tests/test_grad_chain_mpm_gpu.py holds the product to, evaluated with the final FLOOR_MPM = 0 (the bar is KAPPA |R32 - R64|max
    alone, 1e-5 to 1e-3 of these gradients).  Measured, in bars, the first compared gradient found past 10 (step, then apg, then step_w1; rope, then bowls):
        shift_grad        6.67e+03  rope/step/actions
        unshift_pos_grad  1.15e+05  rope/step/pos
        carry_F_detach    2.31e+04  rope/step/actions
        carry_pos_detach  1.09e+05  rope/step/pos
        obs_v_detach      8.21e+04  rope/step/actions
        obs_detach        1.7e+03   rope/apg/flat
        reward_mean3      1.47e+04  rope/step/actions
    (with FLOOR_MPM at 2e-2, as it was while svd3 left its sweeps too early, these were 14 to 50 bars, shift_grad reaching 10 only on
    bowls/step_w1/x.)
    With the floor at 2e-2 shift_grad was the weak one: the step is translation-equivariant up to grid artefacts, so the shift's cotangent on the way in and
    the one on the way out cancel but for those; with the GPU test's weights it moved the rope's x0 gradient by 1 to 8 of those bars
    only (T = 1 to 3), and reached 10 only where obs and the final state weigh as much as the reward."""
    kw = {"rope": dict(ks=[0, 40]), "bowls": {}}
    base = {}

    def unmutated(name, kind, fn):               # (R64 gradients, their bars), computed when first needed
        if (name, kind) not in base:
            g64, g32 = fn(name, demo, goal, torch.float64, **kw[name]), fn(name, demo, goal, torch.float32, **kw[name])
            if kind == "apg":
                g64, g32 = {"flat": g64}, {"flat": g32}
            base[name, kind] = (g64, {k: rc.bar_mpm(g64[k], g32[k]) for k in g64})
        return base[name, kind]

    found = {}
    for m in rc.MPM_MUTATIONS:
        best = (0.0, None)
        for kind, fn in KINDS:
            for name in SETTINGS:
                if best[0] >= 10 or (m == "obs_detach" and kind != "apg") or (m.startswith("carry") and kind == "step_w1"):
                    continue                     # found; only the APG loss has an observation -> policy path; one step carries nothing
                g64, bars = unmutated(name, kind, fn)
                gm = fn(name, demo, goal, torch.float64, mutate=(m,), **kw[name])
                gm = {"flat": gm} if kind == "apg" else gm
                for k in g64:
                    if bars[k] > 0:
                        best = max(best, (np.abs(gm[k] - g64[k]).max() / bars[k], f"{name}/{kind}/{k}"), key=lambda q: q[0])
        found[m] = best
        print(f"MUT_MPM {m}: {best[0]:.3g} bars at {best[1]}")
    for m, (f, where) in found.items():
        assert f >= 10, (m, f, where)
