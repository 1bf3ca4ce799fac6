"""GPU: the gradient whip_rope and pour_water compute end to end (MPMEnv.step_diff, the APG update) against the MPM reference chain of
oracle/ref_chain.py -- focus shift, get_primitive_actions, simulator.step on the CPU oracle, un-shift, nan_to_num, reward and
observation restated from the reference's lines, in f64 throughout (R64) and in f32 throughout (R32).

The HIP step sums with float atomics and is not bit-equal to the oracle, so each side runs its own forward from the same f32 inputs;
the forward values are held to the tolerances the suite already uses for these envs.  Each compared gradient must satisfy
    |HIP - R64|max <= KAPPA |R32 - R64|max + FLOOR_MPM |R64|max        (rc.bar_mpm; KAPPA = 4 as for cloth)
after the case itself passed the conditioning cap |R32 - R64|max <= 5 % of |R64|max.  FLOOR_MPM is twice the largest residual
(|HIP - R64|max - 4 |R32 - R64|max) / |R64|max of the table below, rounded up to one digit, never above 2e-2 and never raised: 0 now, see below.

The handles are the ones the envs build: whip_rope runs the one-workgroup kernels (launch plan 0), pour_water the many-workgroup
path with two container primitives and a liquid.

Measured on the MI355X (one run; whip_rope's one-workgroup kernels repeat these digits run after run, pour_water's positions moved
between ratio 2.05 and 2.38 over four runs):
    GRADCHAIN_MPM whip_rope/forward: x 7.06e-07 (tol 3.53e-06)  v rel 2.59e-06 (tol 1.00e-04)  reward 1.68e-07 (tol 1.23e-05)
    GRADCHAIN_MPM whip_rope/actions: |HIP-R64| 2.900e-08  |R32-R64| 3.459e-08  |R64| 1.885e-02  ratio 0.838  cond 1.83e-06  residual -5.80e-06
    GRADCHAIN_MPM whip_rope/x: |HIP-R64| 3.651e-06  |R32-R64| 3.295e-06  |R64| 1.799e-01  ratio 1.108  cond 1.83e-05  residual -5.30e-05
    GRADCHAIN_MPM whip_rope/v: |HIP-R64| 0.000e+00  |R32-R64| 0.000e+00  |R64| 0.000e+00  (exactly zero on every side: see the test)
    GRADCHAIN_MPM whip_rope/C: |HIP-R64| 2.200e-09  |R32-R64| 1.589e-09  |R64| 1.028e-06  ratio 1.385  cond 1.54e-03  residual -4.04e-03  (printed only)
    GRADCHAIN_MPM whip_rope/F: |HIP-R64| 2.200e-05  |R32-R64| 1.589e-05  |R64| 1.028e-02  ratio 1.385  cond 1.54e-03  residual -4.04e-03
    GRADCHAIN_MPM whip_rope/positions: |HIP-R64| 4.462e-09  |R32-R64| 4.462e-09  |R64| 2.318e-02  ratio 1.000  cond 1.93e-07  residual -5.78e-07
    GRADCHAIN_MPM pour_water/forward: x 5.53e-07 (tol 3.66e-06)  v rel 2.00e-03 (tol 5.37e-03)  reward 4.44e-08 (tol 9.00e-06)
    GRADCHAIN_MPM pour_water/actions: |HIP-R64| 1.288e-05  |R32-R64| 5.176e-06  |R64| 1.266e-03  ratio 2.488  cond 4.09e-03  residual -6.18e-03
    GRADCHAIN_MPM pour_water/x: |HIP-R64| 6.471e-05  |R32-R64| 9.570e-05  |R64| 1.197e-02  ratio 0.676  cond 8.00e-03  residual -2.66e-02
    GRADCHAIN_MPM pour_water/v: |HIP-R64| 2.874e-06  |R32-R64| 4.599e-06  |R64| 6.353e-04  ratio 0.625  cond 7.24e-03  residual -2.44e-02
    GRADCHAIN_MPM pour_water/C: |HIP-R64| 1.168e-08  |R32-R64| 1.817e-08  |R64| 2.287e-06  ratio 0.643  cond 7.95e-03  residual -2.67e-02  (printed only)
    GRADCHAIN_MPM pour_water/F: |HIP-R64| 7.003e-06  |R32-R64| 3.406e-06  |R64| 4.178e-03  ratio 2.056  cond 8.15e-04  residual -1.58e-03
    GRADCHAIN_MPM pour_water/positions: |HIP-R64| 2.420e-04  |R32-R64| 1.093e-04  |R64| 2.829e-02  ratio 2.214  cond 3.86e-03  residual -6.90e-03
    GRADCHAIN_MPM apg_whip_rope/raw: |HIP-R64| 7.247e-09  |R32-R64| 7.247e-09  |R64| 8.308e-03  ratio 1.000  cond 8.72e-07  residual -2.62e-06
    GRADCHAIN_MPM apg_whip_rope/clipped: |HIP-R64| 7.247e-09  |R32-R64| 7.247e-09  |R64| 8.308e-03  ratio 1.000  cond 8.72e-07  residual -2.62e-06
    GRADCHAIN_MPM apg_whip_rope/adam_update: |HIP-R64| 6.727e-07  |R32-R64| 5.904e-07  |R64| 1.000e-04  ratio 1.139  cond 5.90e-03  residual -1.69e-02
    GRADCHAIN_MPM apg_pour_water/raw: |HIP-R64| 7.680e-08  |R32-R64| 9.002e-08  |R64| 2.671e-04  ratio 0.853  cond 3.37e-04  residual -1.06e-03
    GRADCHAIN_MPM apg_pour_water/clipped: |HIP-R64| 7.680e-08  |R32-R64| 9.002e-08  |R64| 2.671e-04  ratio 0.853  cond 3.37e-04  residual -1.06e-03
    GRADCHAIN_MPM apg_pour_water/adam_update: |HIP-R64| 1.641e-06  |R32-R64| 3.278e-06  |R64| 1.000e-04  ratio 0.501  cond 3.28e-02  residual -1.15e-01
With svd3's sweeps left too early (normalised column products below 1e-4; the reset state's F is the identity, a cluster of three equal
singular values, where one Jacobi sweep squares nothing) whip_rope/F was the one positive residual among the asserted tensors,
   whip_rope/F: |HIP-R64| 1.542e-04  |R32-R64| 1.589e-05  |R64| 1.028e-02  ratio 9.706  cond 1.54e-03  residual 8.81e-03
and FLOOR_MPM was twice that, rounded up: 2e-2.  With the exit at round-off level (the table above, same session, same inputs) every
asserted tensor's residual is negative -- everything sits inside KAPPA |R32 - R64| alone -- and FLOOR_MPM is 0 by its rule.

What this bar can see (measured with FLOOR_MPM at 2e-2; the bar is tighter now): with the shift detached in step_diff_unfused's pre_step (planted once, by hand, not kept) the whip_rope x
gradient of this test's step_diff case missed it by a factor 1.25 (|HIP - R64| 4.53e-3 against a bar of 3.61e-3) and no other
leaf moved -- the step is translation-equivariant up to grid artefacts, so the two cotangents of the shift nearly cancel;
tests/test_ref_chain_mpm.py measures every planted mistake.
"""
import zlib

import numpy as np
import pytest
import torch

from oracle import ref_chain as rc

pytestmark = pytest.mark.gpu

NTHREADS = 16
CAP = 0.05


def _check(tag, hip, r64, r32, assert_bar=True, assert_cap=True):
    hip, r64, r32 = (np.asarray(t, np.float64) for t in (hip, r64, r32))
    assert np.isfinite(hip).all() and np.isfinite(r64).all(), tag
    e, e32, n = np.abs(hip - r64).max(), np.abs(r32 - r64).max(), np.abs(r64).max()
    print(f"GRADCHAIN_MPM {tag}: |HIP-R64| {e:.3e}  |R32-R64| {e32:.3e}  |R64| {n:.3e}  ratio {e / e32 if e32 > 0 else float('nan'):.3f}"
          f"  cond {e32 / n if n > 0 else float('nan'):.2e}  residual {(e - rc.KAPPA * e32) / n if n > 0 else float('nan'):.2e}")
    if n == 0:                  # a structural zero of the reference: the product must give exactly zero too
        assert e == 0, tag
        return
    if assert_cap:
        assert e32 <= CAP * n, (tag, "ill-conditioned case", e32, n)
    if assert_bar:
        assert e <= rc.bar_mpm(r64, r32), (tag, e, e32, n)


def _make_env(name, B):
    """the env as its registry entry builds it, reset, its handle on the path the issue names; for whip_rope the gripper is moved onto
    rope particle 5 (the reset leaves it 0.2 away, where control touches no occupied cell and no gradient reaches the actions)"""
    from unidom_amd.envs.registration import env_functions
    env = env_functions[name](batch_size=B, seed=1)
    _, st = env.reset(np.array([0, 7], np.uint32))
    sim = env.simulator
    assert sim.tuning == {} and sim.clip_grad
    if name == "whip_rope":
        assert sim.launch_plan(B) == 0 and sim.n_primitive == 1 and sim.use_position_control
        p = st.primitives[0]
        pos = p.position.clone()
        pos[:, 0] = st.x[:, 5]
        st = st._replace(primitives=[p._replace(position=pos)])
    else:
        assert sim.launch_plan(B) & 1 and sim.n_primitive == 2 and sim.sdf_kind == "container" and not sim.use_position_control
        assert (np.asarray(sim.material) == 0).all()
    return env, st


@pytest.mark.parametrize("name,B", [("whip_rope", 4), ("pour_water", 2)])
def test_env_step_diff_gradient_matches_the_reference_chain(name, B):
    """One step_diff from leaf actions, x, v, C, F and every primitive's positions; seeded random cotangents on the reward (weight 1)
    and on obs, the next x, v, F and primitive 0's positions (weight 1e-3).  Forward against R64; the gradients of actions, x, v, F
    and the positions against the bar (the input C's gradient is ~1e-5 of the others -- g2p overwrites C -- and is printed only).
    pour_water's v leaf sits near the conditioning cap and is reported instead of asserted when it exceeds it; no other leaf may.
    At whip_rope's reset state (the rope at rest on the floor) the gradient of v comes out exactly zero in R64, R32 and the product
    alike, and is held to that.  The start position of whip_rope's gripper gets nothing from the reward (position control); the
    cotangents on obs and on the trajectory pass straight through to it, so that structure is asserted on the reward alone."""
    env, st = _make_env(name, B)
    dev = env.device
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    npy = lambda t: t.detach().cpu().numpy()
    a = rng.uniform(-1, 1, size=(B, 6)).astype(np.float32)
    weights = [1.0] + [1e-3] * 5
    # HIP
    A = torch.tensor(a, device=dev, requires_grad=True)
    X, V, Cm, F = (t.detach().clone().requires_grad_(True) for t in (st.x, st.v, st.C, st.F))
    pos = [p.position.detach().clone().requires_grad_(True) for p in st.primitives]
    s = st._replace(x=X, v=V, C=Cm, F=F, primitives=[p._replace(position=q) for p, q in zip(st.primitives, pos)])
    obs, reward, done, info = env.step_diff(A, s)
    env.simulator.check_status()
    assert not bool(done.any())
    s1 = info["state"]
    outs = [reward, obs, s1.x, s1.v, s1.F, s1.primitives[0].position]
    cots = [rng.normal(size=tuple(o.shape)) for o in outs]
    # the rewards alone, for the structure of the position gradient
    pos_r = torch.autograd.grad(reward.sum(), pos, retain_graph=True, allow_unused=True)
    loss = sum(w * (o * torch.tensor(c, dtype=torch.float32, device=dev)).sum() for w, o, c in zip(weights, outs, cots))
    hip = [npy(g) for g in torch.autograd.grad(loss, [A, X, V, Cm, F] + pos)]
    hip = hip[:5] + [np.stack(hip[5:], 1)]
    env.simulator.check_status()
    # reference chain
    ref_g, ref_v, ref_pos_r = {}, {}, {}
    for dtype in (torch.float64, torch.float32):
        ref = rc.MpmRefEnv.from_env(env, dtype=dtype, nthreads=NTHREADS)
        leaf = lambda t: torch.tensor(t, dtype=dtype, requires_grad=True)
        leaves = [leaf(a)] + [leaf(npy(t)) for t in (st.x, st.v, st.C, st.F)] + [leaf(np.stack([npy(p.position) for p in st.primitives], 1))]
        rs = ref.state_from(st, x=leaves[1], v=leaves[2], C=leaves[3], F=leaves[4], pos=leaves[5])
        robs, rrew, rs1, _ = ref.step(leaves[0], rs)
        routs = [rrew, robs, rs1["x"], rs1["v"], rs1["F"], rs1["pos"][:, 0]]
        ref_pos_r[dtype] = torch.autograd.grad(rrew.sum(), leaves[5], retain_graph=True, allow_unused=True)[0]
        rloss = sum(w * (o * torch.tensor(c, dtype=dtype)).sum() for w, o, c in zip(weights, routs, cots))
        ref_g[dtype] = [g.double().numpy() for g in torch.autograd.grad(rloss, leaves)]
        ref_v[dtype] = {k: rs1[k].detach().double().numpy() for k in ("x", "v")} | {"reward": rrew.detach().double().numpy()}
    # forward
    v64, v32 = ref_v[torch.float64], ref_v[torch.float32]
    ex, ev = np.abs(npy(s1.x) - v64["x"]).max(), np.abs(npy(s1.v) - v64["v"]).max() / np.abs(v64["v"]).max()
    gx, gv = np.abs(v32["x"] - v64["x"]).max(), np.abs(v32["v"] - v64["v"]).max() / np.abs(v64["v"]).max()
    tol_x, tol_v = (5e-6 * np.abs(v64["x"]).max(), 1e-4) if name == "whip_rope" else (3 * gx + 2e-6, 3 * gv + 1e-4)
    er = np.abs(npy(reward) - v64["reward"]).max()
    tol_r = (10 * tol_x + 1e-6) * np.abs(v64["reward"]).max()      # reward = e ** (-10 l2), |d l2| <= |d x|max; one f32 rounding
    print(f"GRADCHAIN_MPM {name}/forward: x {ex:.2e} (tol {tol_x:.2e})  v rel {ev:.2e} (tol {tol_v:.2e})  reward {er:.2e} (tol {tol_r:.2e})")
    assert ex <= tol_x and ev <= tol_v and er <= tol_r, (ex, tol_x, ev, tol_v, er, tol_r)
    # gradients
    r64, r32 = ref_g[torch.float64], ref_g[torch.float32]
    for i, leaf_name in enumerate(("actions", "x", "v", "C", "F", "positions")):
        tag = f"{name}/{leaf_name}"
        if leaf_name == "C":
            _check(tag, hip[i], r64[i], r32[i], assert_bar=False, assert_cap=False)
        elif name == "pour_water" and leaf_name == "v" and np.abs(r32[i] - r64[i]).max() > CAP * np.abs(r64[i]).max():
            _check(tag + " (past the conditioning cap: reported only)", hip[i], r64[i], r32[i], assert_bar=False, assert_cap=False)
        else:
            _check(tag, hip[i], r64[i], r32[i])
    # structure
    if name == "whip_rope":       # the last three action components are overwritten with zeros; position control: the start position
        assert (hip[0][:, 3:] == 0).all() and (r64[0][:, 3:] == 0).all()      # never reaches the particles, so the reward gives it nothing
        assert all(g is None or (g == 0).all() for g in pos_r) and (ref_pos_r[torch.float64] is None or (ref_pos_r[torch.float64] == 0).all())
    else:                         # no vertical motion of the bowl
        assert (hip[0][:, 1] == 0).all() and (r64[0][:, 1] == 0).all()


@pytest.mark.parametrize("name,B,ep_len", [("whip_rope", 4, 2), ("pour_water", 2, 3)])
def test_apg_update_matches_the_reference_chain(name, B, ep_len):
    """APG(env, ep_len, learning_rate=1e-4, max_gradient_norm=0.3, seed=0) with the noise learner.draw_noise draws: the raw flat
    policy gradient before the clip, the clipped gradient and the Adam step of one minimize() against the reference chain on the
    same initial parameters, each chain on its own action values.  pour_water at ep_len 3 is in because its three tensors
    meet the 5 % conditioning cap measured here (raw and clipped 3.4e-4, the Adam step 3.3e-2: an entry whose gradient is near
    Adam's eps moves by a good part of the learning rate); the cap is asserted on every run."""
    from unidom_amd.algorithms.apg.core import APG
    from unidom_amd.utils import prng
    assert not torch.backends.cuda.matmul.allow_tf32
    env, st = _make_env(name, B)
    learner = APG(env, ep_len, learning_rate=1e-4, max_gradient_norm=0.3, seed=0)
    assert not learner.squash
    _, key_grad = prng.split(learner.key)
    _, noise = learner.draw_noise(key_grad, ep_len)
    noise = noise.cpu().numpy()
    params0 = [p.detach().clone() for p in learner.params]
    seen = {}
    step_fn = learner.sync.step

    def step():
        seen["raw"] = learner.flat_grad.detach().cpu().numpy().copy()
        r = step_fn()
        seen["clipped"] = learner.flat_grad.detach().cpu().numpy().copy()
        return r

    learner.sync.step = step
    learner.minimize(st)
    env.simulator.check_status()
    update = torch.cat([(p.detach() - q).reshape(-1) for p, q in zip(learner.params, params0)]).cpu().numpy()
    ref = {}
    for dtype in (torch.float64, torch.float32):
        renv = rc.MpmRefEnv.from_env(env, dtype=dtype, nthreads=NTHREADS)
        assert not renv.squash
        pol = rc.PolicyRef(params0, dtype)
        rloss, _, _ = rc.apg_loss(renv, pol, renv.state_from(st), noise)
        grads = torch.autograd.grad(rloss, pol.params)
        clipped, upd = rc.adam_first_step(pol.params, grads, 1e-4, 0.3)
        ref[dtype] = (torch.cat([g.reshape(-1) for g in grads]).double().numpy(), clipped.double().numpy(), upd.double().numpy())
    for i, (tag, hip) in enumerate((("raw", seen["raw"]), ("clipped", seen["clipped"]), ("adam_update", update))):
        _check(f"apg_{name}/{tag}", hip, ref[torch.float64][i], ref[torch.float32][i])
