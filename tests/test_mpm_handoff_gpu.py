"""GPU: the MPM many-workgroup backward chooses restore or recompute per env on the device (ud_mpm_step_bwd clip bit 2).

The forward leaves one word per env in the checkpoint (non-zero = that env's grid checkpoint is incomplete: status bit 0); with clip
bit 2 the backward restores the grid of every env whose word is clear and recomputes p2g + grid op for the others, in the same call,
and reports value 8 in status[] for the envs it recomputed.  SimpleMPMSimulator.device_handoff turns that on in the Python mirror (no
side stream, no pinned buffer, no event between the two calls), which is what lets APG.capture take such a simulator.

Base case: the rope at n_grid 128 (N = 798, 3 substeps) with a pool of 1 record per particle and substep = 2394 records per env.  The
compact rope needs ~0.58 cells per particle and moves 1e-5 in three substeps at dt = 1e-4: every seed fits.  "Scattered" = the env's
particles drawn uniformly from [0.1, 0.4)^3: 798 stencils of 27 cells spread over 38^3 cells overflow the pool with certainty.
Reference = a handle with grid_ckpt_cells = 0 on the same inputs, at the 2e-5 the existing fall-back tests hold this comparison to."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from test_mpm_gpu import _rel, _scaled_case, _tune, make_collide_sim, run_hip, run_hip_collide

pytestmark = pytest.mark.gpu

KEYS = ("x", "v", "gx", "gv", "gC", "gF", "gppos", "gaction")
SCALARS = ("gfriction", "gmu", "glamda")
TOL = 2e-5


def _sim_cls():
    from unidom_amd.engine.mpm_simulator import SimpleMPMSimulator
    assert hasattr(SimpleMPMSimulator, "device_handoff")
    return SimpleMPMSimulator


def _scatter(st, envs):
    st = {k: v.copy() for k, v in st.items()}
    for b in envs:
        st["x"][b] = np.random.default_rng(2).uniform(0.1, 0.4, size=st["x"][b].shape).astype(np.float32)
    return st


_refs = {}


def _reference(B, flagged, clip=True):
    """The recomputing backward (grid_ckpt_cells = 0) on the base case with `flagged` envs scattered, under the kernel selection in force;
    computed once per (selection, B, flagged, clip) and shared."""
    key = (tuple(sorted(_sim_cls().default_tuning.items())), B, tuple(flagged), clip)
    if key not in _refs:
        ref_sim, st, g, _ = _scaled_case(3, 0, B=B, grid_ckpt_cells=0)
        _refs[key] = run_hip(ref_sim, _scatter(st, flagged), g=g, clip=clip)
    return _refs[key]


def _agree(got, ref, keys=KEYS + SCALARS, what=""):
    for key in keys:
        r = _rel(got[key], ref[key])
        print(what, key, r)
        assert np.isfinite(got[key]).all() and r < TOL, (key, r, what)


def _flags(sim):
    return (sim.last_status["fwd"].cpu().numpy() & 1).tolist(), ((sim.last_status["bwd"].cpu().numpy() & 8) // 8).tolist()


def _handoff_case(B):
    sim, st, g, _ = _scaled_case(3, 0, B=B, grid_ckpt_cells=1)
    sim.device_handoff = True
    return sim, st, g


@pytest.mark.parametrize("backward", ["two_launch", "four_kernel"])
@pytest.mark.parametrize("forward", ["multi_kernel", "cluster"])
def test_mixed_batch_restores_and_recomputes_per_env(forward, backward, monkeypatch):
    """Env 1 scattered, envs 0 and 2 compact: behind either forward (the multi-kernel one flags the env from lg_grid, the cluster one from
    its record writer) and through either restoring backward (two launches per substep, or four) all three envs match the reference;
    the forward's bit 0 and the backward's value 8 are [0, 1, 0]; nothing was staged through the host.  The same call again on the same
    handle (both passes handed their grids back all-zero), then the compact rope back in env 1: nothing recomputes, the result still
    matches, and the device counter has seen two recomputed env-steps.  Without the feature bit 2 is discarded and env 1 is restored
    from an incomplete checkpoint."""
    _sim_cls()
    kw = dict(cluster=-1) if forward == "multi_kernel" else dict(cluster=1, cluster_part_lanes=64)
    if backward == "four_kernel":
        kw["bwd_two_launch"] = -1
    _tune(monkeypatch, **kw)
    sim, st, g = _handoff_case(3)
    assert (sim.launch_plan(3) & 2 != 0) == (forward == "cluster") and (sim.launch_plan(3) & 4 != 0) == (backward == "two_launch")
    mixed = _scatter(st, [1])
    for again in (0, 1):
        got = run_hip(sim, mixed, g=g, clip=True)
        assert _flags(sim) == ([0, 1, 0], [0, 1, 0]), again
        _agree(got, _reference(3, [1]), what=again)
        assert sim._staged == [] and sim._flag_stream is None and sim.grid_ckpt_overflows == 0
    got = run_hip(sim, st, g=g, clip=True)
    assert _flags(sim) == ([0, 0, 0], [0, 0, 0])
    _agree(got, _reference(3, []))
    assert sim.grid_recomputed_env_steps() == 2


@pytest.mark.parametrize("B,flagged", [(3, [0]), (3, [2]), (3, [0, 1, 2]), (9, [1, 8])])
def test_wherever_the_flagged_env_sits(B, flagged, multi_kernel_path_):
    """First, last and every env of a batch of 3; envs 1 and 8 of 9 -- eight or more envs in a group take the XCD block order, which
    interleaves the envs over the block ids (the selector must test the decoded env), and 9 is no multiple of 8."""
    _sim_cls()
    sim, st, g = _handoff_case(B)
    want = [int(b in flagged) for b in range(B)]
    for again in (0, 1):
        got = run_hip(sim, _scatter(st, flagged), g=g, clip=True)
        assert _flags(sim) == (want, want), again
        _agree(got, _reference(B, flagged), what=again)
    assert sim.grid_recomputed_env_steps() == 2 * len(flagged)


@pytest.fixture
def multi_kernel_path_(monkeypatch):
    _tune(monkeypatch, cluster=-1)


def _collide_batch(S, B):
    from conftest import GOLDEN
    import os
    from test_oracle_mpm import _collide_case
    demo = np.load(os.path.join(GOLDEN, "whip_rope_demo0.npz"))
    cases = [_collide_case(demo, S, 40, 1, b, np.float32) for b in range(B)]
    st = {k: np.concatenate([c[0][k] for c in cases], 0) for k in cases[0][0]}
    g = {k: np.concatenate([c[1][k] for c in cases], 0) for k in cases[0][1]}
    st["x"][1] = np.random.default_rng(2).uniform(0.1, 0.4, size=st["x"][1].shape).astype(np.float32)   # env 1 scattered
    return st, g


def _stencil_cells(x, n_grid=64, res=32):
    base = (x * np.float32(n_grid) - np.float32(0.5)).astype(np.int32)
    cells = {(b[0] + i, b[1] + j, b[2] + k) for b in base for i in range(3) for j in range(3) for k in range(3)}
    return len({c for c in cells if all(0 <= c[d] < res for d in range(3))})


@pytest.mark.parametrize("grid_ckpt_cells", [1, 8])
def test_soft_contact_with_collide_records(grid_ckpt_cells, multi_kernel_path_):
    """Soft contact (a rotated, turning box; the forward leaves collide records beside the grid checkpoint and the restoring grid-op
    adjoint reads them): 67 particles, 3 substeps, B = 3 with env 1 scattered, against the grid_ckpt_cells = 0 handle, gprot included,
    clip on.  A pool of 1 record per particle and substep (201 records) is too small for the compact rope as well -- its stencils cover
    more cells than that in one substep -- so every env recomputes; a pool of 8 (1608 records) holds the compact envs (counted on the
    host below, from the positions) and not the scattered one, which is the mixed case with collide records.  In both the backward's
    report must equal the forward's flag, and env 1 is flagged."""
    _sim_cls()
    S = 3
    st, g = _collide_batch(S, 3)
    sim = make_collide_sim(S, 3)
    sim.grid_ckpt_cells = grid_ckpt_cells
    sim._make_handle()
    sim.device_handoff = True
    ref = run_hip_collide(make_collide_sim(S, 3), st, g, True)
    cells = [_stencil_cells(st["x"][b]) for b in range(3)]       # per substep, at the start of the step
    budget = S * grid_ckpt_cells * 67
    for again in (0, 1):
        got = run_hip_collide(sim, st, g, True)
        fwd, rep = _flags(sim)
        assert fwd == rep and fwd[1] == 1, (fwd, rep)
        if grid_ckpt_cells == 8:
            # a quarter on top for cells the motion adds: |v| dt S = 6e-4, four hundredths of a cell
            assert S * cells[0] * 5 // 4 < budget and S * cells[2] * 5 // 4 < budget and cells[1] > budget, (cells, budget)
            assert fwd == [0, 1, 0]
        else:
            assert min(cells) > budget and fwd == [1, 1, 1], (cells, budget)
        _agree(got, ref, keys=KEYS + ("gprot",) + SCALARS, what=(grid_ckpt_cells, again))


class _Rec(list):
    """status_log that remembers what was appended (check_status folds and empties the log)"""
    def __init__(self):
        super().__init__()
        self.seen = []

    def append(self, t):
        self.seen.append(t)
        super().append(t & ~8)     # as the mirror does under device_handoff: value 8 is a report, check_status must not raise on it


def _run_with_clip(monkeypatch, sim, st, g, clip, run=run_hip):
    """run_hip with the backward's clip argument replaced; returns the result and the backward's raw status[]"""
    from unidom_amd import _lib
    L = _lib.lib()
    real = L.ud_mpm_step_bwd

    def call(*a):
        a = list(a)
        a[14] = C.c_int(clip)
        return real(*a)
    sim.status_log = _Rec()
    log = sim.status_log
    with monkeypatch.context() as m:
        m.setattr(L, "ud_mpm_step_bwd", call)
        res = run(sim, st, g, True)
    return res, log.seen[-1].cpu().numpy()


def test_the_bits(multi_kernel_path_, monkeypatch):
    """clip = 1 | 2 | 4: bit 1 wins, every env recomputes and says so.  Bit 2 where there is no grid checkpoint to choose from (a
    grid_ckpt_cells = 0 handle; the one-workgroup path) changes nothing and reports nothing.  Without device_handoff the mirror still
    carries the flag through the host and counts it there."""
    _sim_cls()
    run = lambda sim, st, g, clip: run_hip(sim, st, g=g, clip=clip)
    sim, st, g, _ = _scaled_case(3, 0, B=3, grid_ckpt_cells=1)
    mixed = _scatter(st, [1])
    got, status = _run_with_clip(monkeypatch, sim, mixed, g, 1 | 2 | 4, run)
    assert status.tolist() == [8, 8, 8]
    _agree(got, _reference(3, [1]))
    sim0, _, _, _ = _scaled_case(3, 0, B=3, grid_ckpt_cells=0)
    got, status = _run_with_clip(monkeypatch, sim0, mixed, g, 1 | 4, run)
    assert status.tolist() == [0, 0, 0]
    _agree(got, _reference(3, [1]))
    # one workgroup per env: 67 particles, position control
    import os
    from conftest import GOLDEN
    from test_mpm_gpu import make_sim
    from test_oracle_mpm import _adjoint_case
    demo = np.load(os.path.join(GOLDEN, "whip_rope_demo0.npz"))
    st1, g1 = _adjoint_case(demo, 3, 40, 1, 0, np.float32)
    sim1 = make_sim(3, 1)
    assert sim1.launch_plan(1) == 0
    want = run_hip(sim1, st1, g=g1, clip=True)
    got, status = _run_with_clip(monkeypatch, sim1, st1, g1, 1 | 4, run)
    assert status.tolist() == [0]
    for key in KEYS[2:] + SCALARS:
        assert np.isfinite(got[key]).all() and _rel(got[key], want[key]) < TOL, key
    # the host path, untouched
    simh, _, _, _ = _scaled_case(3, 0, B=3, grid_ckpt_cells=1)
    assert simh.device_handoff is False
    got = run_hip(simh, mixed, g=g, clip=True)
    assert simh.grid_ckpt_overflows == 1 and simh.grid_recomputed_env_steps() == 0 and simh._flag_stream is not None
    _agree(got, _reference(3, [1]))


@pytest.mark.parametrize("env_groups,B", [(1, 3), (0, 3), (2, 4)])
def test_replay_sees_what_the_capture_did_not(env_groups, B, monkeypatch):
    """One forward + backward captured into a HIP graph with the compact rope in every env: the replay restores every env.  Then the
    scattered cloud goes into env 1's static input and the SAME graph is replayed: the forward flags env 1 and the backward recomputes
    it -- the decision is taken on the device at replay time, not baked in at capture.  Once on one stream group (no fork / join events
    inside the capture), once with the default tuning (one group as well at three envs), and once with four envs in two groups: the
    forward and both passes of the backward then fork onto a side stream and join back inside the capture, re-recording the same
    events (lg_fork / lg_join), which is what a 32-env shape_rope or scaled-rope update does."""
    _sim_cls()
    from unidom_amd.engine.mpm_simulator import _Step
    _tune(monkeypatch, cluster=-1, **({"env_groups": 1} if env_groups else {}))
    sim, st, g = _handoff_case(B)
    mixed = _scatter(st, [1])
    ref_c, ref_m = _reference(B, []), _reference(B, [1])
    none, one = [0] * B, [0, 1] + [0] * (B - 2)
    dev = sim.device
    work = torch.cuda.Stream(dev)
    names = ("x", "v", "C", "F", "ppos", "friction", "mu", "lamda", "action")
    with torch.cuda.stream(work):
        t = lambda a, r=False: torch.tensor(np.asarray(a, np.float32), device=dev, requires_grad=r)
        ins = {k: t(st[k], True) for k in names}
        J, prot, psize = t(st["J"]), t(st["prot"]), t(st["psize"])
        G = {k: t(v) for k, v in g.items()}

        def once():
            out = _Step.apply(sim, ins["x"], ins["v"], ins["C"], ins["F"], J, ins["ppos"], prot, psize, ins["friction"], ins["mu"],
                              ins["lamda"], ins["action"])
            loss = (out[0] * G["gx"]).sum() + (out[1] * G["gv"]).sum() + (out[2] * G["gC"]).sum() + (out[3] * G["gF"]).sum() + \
                (out[5] * G["gppos"]).sum()
            grads = torch.autograd.grad(loss, [ins[k] for k in names])
            return out, grads
        for _ in range(3):
            once()
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=work):
            out, grads = once()
            fwd_s, bwd_s = sim.last_status["fwd"], sim.last_status["bwd"]

        def replay():
            graph.replay()
            torch.cuda.synchronize(dev)
            res = dict(x=out[0], v=out[1])
            res.update({"g" + k: v for k, v in zip(names, grads)})
            res = {k: v.detach().cpu().numpy() for k, v in res.items()}
            return res, (fwd_s.cpu().numpy() & 1).tolist(), ((bwd_s.cpu().numpy() & 8) // 8).tolist()
        keys = ("x", "v", "gx", "gv", "gC", "gF", "gppos", "gaction", "gfriction", "gmu", "glamda")
        before = sim.grid_recomputed_env_steps()
        got, fwd, rep = replay()
        assert (fwd, rep) == (none, none)
        _agree(got, ref_c, keys=keys, what="compact")
        with torch.no_grad():
            ins["x"][1].copy_(t(mixed["x"][1]))
        got, fwd, rep = replay()
        assert (fwd, rep) == (one, one)
        _agree(got, ref_m, keys=keys, what="env 1 scattered")
        assert sim.grid_recomputed_env_steps() == before + 1
    sim.check_status()


def _pour_water_updates(mode, handoff=True):
    from unidom_amd.algorithms.apg.core import APG
    from unidom_amd.envs.registration import env_functions
    lr = 1e-4
    env = env_functions["pour_water"](batch_size=4, seed=0, aux_reward=True)
    env.simulator.device_handoff = handoff
    _, st = env.reset(np.array([0, 3], np.uint32))
    assert env.simulator._h_large and env.simulator.grid_ckpt_cells > 0
    learner = APG(env, 2, learning_rate=lr, max_gradient_norm=0.3, seed=0)
    w0 = [p.detach().clone() for p in learner.params]
    if mode == "graph":
        learner.capture(st)
        assert all(torch.equal(a, b) for a, b in zip(w0, learner.params))
    ms = [(learner.minimize_captured() if mode == "graph" else learner.minimize(st)) for _ in range(3)]
    torch.cuda.synchronize()
    env.simulator.check_status()
    d = torch.cat([(p.detach() - a).reshape(-1) for p, a in zip(learner.params, w0)])
    return float(ms[-1]["loss"]), float(ms[-1]["grad_norm"]), d


# What two EAGER pour_water learners from the same seed differ by after three updates (1x MI355X; float atomics order their sums by
# arrival), as (relative loss, relative gradient norm, share of parameters further apart than a tenth of one Adam step).  Measured over
# six pairs of minimize() learners: gradient norm 6.1e-7, 1.7e-6, 3.2e-6, 2.5e-5, 2.8e-5; loss 0 or one f32 ulp (1.49e-8 at |loss| = 0.24;
# the loss enters as |difference| / max(1, |loss|)); share 0 in every pair.  The largest of each stands for "their difference".
EAGER_SPREAD = (1.49e-8, 2.8e-5, 0.0)


def test_captured_many_workgroup_update_is_the_eager_update():
    """APG.capture takes a many-workgroup simulator with a grid checkpoint once device_handoff is on: pour_water, 4 envs, 2 steps per
    episode, one update = one HIP graph.  capture() leaves the parameters untouched; after three updates from the same seed, loss and
    gradient norm agree with an eager learner and the parameters have moved.  The bars are four times what two eager learners from the
    same seed differ by (EAGER_SPREAD above, measured on this commit): 6e-8 in loss, 1.1e-4 in gradient norm, no parameter further
    apart than a tenth of a step.  Measured, captured against eager, over seven pairs: loss 0 or 1.49e-8, gradient norm 4.2e-6 .. 3.2e-5,
    share 0."""
    _sim_cls()
    lr = 1e-4
    dev = torch.device("cuda", 0)
    work = torch.cuda.Stream(dev)
    with torch.cuda.stream(work):
        le, ge, de = _pour_water_updates("eager")
        lg, gg, dg = _pour_water_updates("graph")
    seen = (abs(le - lg) / max(1.0, abs(le)), abs(ge - gg) / ge, float(((de - dg).abs() > 0.1 * lr).float().mean()))
    print("graph-vs-eager (loss, grad norm, share off):", seen)
    assert math.isfinite(le) and math.isfinite(lg)
    assert float(de.abs().max()) > lr and float(dg.abs().max()) > lr            # the parameters did move
    for i in range(3):
        assert seen[i] <= 4 * EAGER_SPREAD[i], (i, seen)


def test_capture_refuses_the_host_path_and_takes_device_handoff():
    """The refusal and its message stay for a simulator that stages its flags through the host; with device_handoff the same env
    captures, leaves the parameters as they were, and its replayed updates move them (finite loss and gradient norm)."""
    _sim_cls()
    from unidom_amd.algorithms.apg.core import APG
    from unidom_amd.envs.registration import env_functions
    dev = torch.device("cuda", 0)
    work = torch.cuda.Stream(dev)
    with torch.cuda.stream(work):
        env = env_functions["pour_water"](batch_size=4, seed=0, aux_reward=True)
        _, st = env.reset(np.array([0, 3], np.uint32))
        with pytest.raises(RuntimeError, match="stages grid-checkpoint flags through the host"):
            APG(env, 2, learning_rate=1e-4, max_gradient_norm=0.3, seed=0).capture(st)
        lg, gg, dg = _pour_water_updates("graph")
    assert math.isfinite(lg) and math.isfinite(gg) and gg > 0 and float(dg.abs().max()) > 1e-4
