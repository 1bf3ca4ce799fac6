"""GPU: the gradient the product computes end to end (env step_diff, the APG update) against the reference chain of
oracle/ref_chain.py -- the same operation restated on the CPU oracle, with the adjoint in f64 (R64) and in f32 (R32).

Each compared tensor must satisfy   |HIP - R64|max <= KAPPA |R32 - R64|max + REL_FLOOR |R64|max   (KAPPA = 4, REL_FLOOR = 1e-6):
the product's gradient is no less accurate than a plain f32 implementation of the same operation.  The forward the reference
runs is the product's bit for bit (the state after each step is compared, and the macro actions and contact distances are
checked against the fused kernel's on every call), so what is measured is the adjoint alone.  The f64 adjoint sweeps followed
the f32 forward's grasp decisions without a single disagreement (flips = 0) in every case.

Measured |HIP - R64|max / |R32 - R64|max on the MI355X (gradients of actions / x0 / v0 / primitive0):
    fold_cloth1 (mode 0, order v2)       0.48 / 1.05 / 1.05 / 1.49
    fold_cloth1 (kernel_mode 3)          1.00 / 0.06 / 0.06 / 1.00
    unfold_cloth1 (mu = 3, no lists)     0.62 / 0.79 / 0.79 / 1.21
    fold_tshirt (3573 particles)         0.88 / 0.32 / 1.92 / 1.45
    fold_cloth1_para (32 envs)           0.65 / 0.68 / 0.68 / 1.00
    APG headline (raw / clipped / Adam step)   0.89 / 0.015 / 1.24
The largest, 1.92, sets KAPPA = 4 (oracle/ref_chain.py).
"""
import zlib

import numpy as np
import pytest
import torch

from oracle import ref_chain as rc

pytestmark = pytest.mark.gpu

NTHREADS = 16


def _check(tag, hip, r64, r32):
    hip, r64, r32 = (np.asarray(t, np.float64) for t in (hip, r64, r32))
    assert np.isfinite(hip).all() and np.isfinite(r64).all(), tag
    e, e32, n = np.abs(hip - r64).max(), np.abs(r32 - r64).max(), np.abs(r64).max()
    print(f"GRADCHAIN {tag}: |HIP-R64| {e:.3e}  |R32-R64| {e32:.3e}  |R64| {n:.3e}  ratio {e / e32 if e32 > 0 else float('nan'):.3f}")
    assert n > 0, tag
    assert e <= rc.bar(r64, r32), (tag, e, e32, n)


def _pnp_check(env):
    from unidom_amd.envs.basic import _fused

    def f(a32, p32, x32):
        t = lambda a: torch.tensor(a, device=env.device)
        with torch.no_grad():
            m, c = _fused.pnp_and_contact(t(a32), t(p32), t(x32))
        return m.cpu().numpy(), c.cpu().numpy()

    return f


def _make_env(name, B):
    from unidom_amd.envs.registration import env_functions
    if name == "fold_cloth1_mode3":
        from unidom_amd.envs.fold_cloth1_env import DefaultConf
        conf = DefaultConf()
        conf.kernel_mode = 3
        env = env_functions["fold_cloth1"](batch_size=B, conf=conf, seed=0, aux_reward=True)
        assert env.simulator.mode == 3
        return env
    if name == "fold_cloth1_para":    # bench.py's fold_cloth1_para line
        return env_functions[name](batch_size=B, aux_reward=True, stiffness=1300, eval_min_max_stiff=[10, 1800])
    np.random.seed(0)                 # unfold_cloth1 folds the cloth at reset with np.random picks
    return env_functions[name](batch_size=B, aux_reward=True)


@pytest.mark.parametrize("name,B", [("fold_cloth1", 4), ("fold_cloth1_mode3", 4), ("unfold_cloth1", 2), ("fold_tshirt", 2),
                                    ("fold_cloth1_para", 32)])
def test_env_step_diff_gradient_matches_the_reference_chain(name, B):
    """One step_diff from leaf actions and leaf initial x, v, primitive0, random cotangents on reward, obs, the final state and
    (use_substep_obs) obs_list: the gradients of all four leaves against R64 / R32."""
    env = _make_env(name, B)
    _, st = env.reset(np.array([0, 5], np.uint32))
    dev = env.device
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x0 = st.x.cpu().numpy()
    a = np.zeros((B, 6), np.float32)
    for b in range(B):                                  # pick near a particle, place up to 0.15 away, y = 0
        p = x0[b, rng.integers(0, x0.shape[1])]
        a[b, [0, 2]] = p[[0, 2]] + rng.normal(size=2) * 0.01
        a[b, [3, 5]] = a[b, [0, 2]] + rng.uniform(-0.15, 0.15, size=2)
    lists = bool(env.conf.use_substep_obs)
    # HIP
    A = torch.tensor(a, device=dev, requires_grad=True)
    X, V, P0 = (t.detach().clone().requires_grad_(True) for t in (st.x, st.v, st.primitive0))
    obs, reward, _, info = env.step_diff(A, st._replace(x=X, v=V, primitive0=P0))
    s1 = info["state"]
    outs = [reward, obs, s1.x, s1.v, s1.primitive0, s1.primitive1] + ([info["obs_list"]] if lists else [])
    cots = [rng.normal(size=tuple(o.shape)) for o in outs]
    loss = sum((o * torch.tensor(c, dtype=torch.float32, device=dev)).sum() for o, c in zip(outs, cots))
    hip = [g.cpu().numpy() for g in torch.autograd.grad(loss, [A, X, V, P0])]
    # reference chain
    ref_g = {}
    for dtype in (torch.float64, torch.float32):
        ref = rc.ClothRefEnv.from_env(env, dtype=dtype, nthreads=NTHREADS)
        ref.check_pnp = _pnp_check(env)
        leaves = [torch.tensor(t, dtype=dtype, requires_grad=True) for t in (a, x0, st.v.cpu().numpy(), st.primitive0.cpu().numpy())]
        s = ref.state_from(st, x=leaves[1], v=leaves[2], primitive0=leaves[3])
        robs, rrew, rs1, robs_list = ref.step(leaves[0], s)
        np.testing.assert_array_equal(rs1["x"].detach().numpy().astype(np.float32), s1.x.detach().cpu().numpy())
        np.testing.assert_array_equal(rs1["v"].detach().numpy().astype(np.float32), s1.v.detach().cpu().numpy())
        routs = [rrew, robs, rs1["x"], rs1["v"], rs1["primitive0"], rs1["primitive1"]] + ([robs_list] if lists else [])
        rloss = sum((o * torch.tensor(c, dtype=dtype)).sum() for o, c in zip(routs, cots))
        ref_g[dtype] = [g.double().numpy() for g in torch.autograd.grad(rloss, leaves)]
        assert ref.flips == 0, (dtype, ref.flips)
    r64, r32 = ref_g[torch.float64], ref_g[torch.float32]
    for i, leaf in enumerate(("actions", "x0", "v0", "primitive0")):
        _check(f"{name}/{leaf}", hip[i], r64[i], r32[i])
    # the place height never reaches the loss; the pick height only through the contact term
    assert (hip[0][:, 4] == 0).all() and (r64[0][:, 4] == 0).all()
    np.testing.assert_array_equal(hip[0][:, 1] == 0, r64[0][:, 1] == 0)


def test_apg_headline_update_matches_the_reference_chain():
    """bench.py's headline update: fold_cloth1, 4 envs, ep_len 3, APG(env, 3, learning_rate=1e-4, max_gradient_norm=0.3, seed=0),
    the noise learner.draw_noise draws for it.  The raw flat policy gradient before the clip, the clipped gradient and the Adam
    step of one minimize() against the reference chain on the same parameters, fed the product's action values."""
    from unidom_amd.algorithms.apg.core import APG
    from unidom_amd.envs.registration import env_functions
    from unidom_amd.utils import prng
    assert not torch.backends.cuda.matmul.allow_tf32
    env = env_functions["fold_cloth1"](batch_size=4, seed=0, aux_reward=True)
    learner = APG(env, 3, learning_rate=1e-4, max_gradient_norm=0.3, seed=0)
    _, st = env.reset(prng.split(prng.PRNGKey(0), 1)[0])
    _, key_grad = prng.split(learner.key)
    _, noise = learner.draw_noise(key_grad, 3)
    noise = noise.cpu().numpy()
    params0 = [p.detach().clone() for p in learner.params]
    seen = {}
    loss_fn, step_fn = learner.loss, learner.sync.step

    def loss(state, key=None, deterministic_noise=None):
        out = loss_fn(state, key, deterministic_noise)
        seen["actions"] = [t.detach().cpu().numpy() for t in out[1][2]]
        return out

    def step():
        seen["raw"] = learner.flat_grad.detach().cpu().numpy().copy()
        r = step_fn()
        seen["clipped"] = learner.flat_grad.detach().cpu().numpy().copy()
        return r

    learner.loss, learner.sync.step = loss, step
    learner.minimize(st)
    update = torch.cat([(p.detach() - q).reshape(-1) for p, q in zip(learner.params, params0)]).cpu().numpy()
    ref = {}
    for dtype in (torch.float64, torch.float32):
        renv = rc.ClothRefEnv.from_env(env, dtype=dtype, nthreads=NTHREADS)
        renv.check_pnp = _pnp_check(env)
        pol = rc.PolicyRef(params0, dtype)
        rloss, _, _ = rc.apg_loss(renv, pol, renv.state_from(st), noise, seen["actions"])
        grads = torch.autograd.grad(rloss, pol.params)
        clipped, upd = rc.adam_first_step(pol.params, grads, 1e-4, 0.3)
        ref[dtype] = (torch.cat([g.reshape(-1) for g in grads]).double().numpy(), clipped.double().numpy(), upd.double().numpy())
        assert renv.flips == 0
    for i, (tag, hip) in enumerate((("raw", seen["raw"]), ("clipped", seen["clipped"]), ("adam_update", update))):
        _check(f"apg_fold_cloth1/{tag}", hip, ref[torch.float64][i], ref[torch.float32][i])
