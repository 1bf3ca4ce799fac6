"""Shared by tests/test_cloth_adjoint_bits_gpu.py, tests/test_cloth_adjoint_bits_cases.py and tools/record_cloth_adjoint_bits.py (a
plain module, no fixtures): the cases whose adjoint outputs tests/golden/cloth_adjoint_bits.npz records bit for bit.

The inputs are those `_reference` of tests/test_cloth_adjoint_f64_gpu.py draws (same `BODIES`, `TWEAKS`, seed by body / S / B / T, so
the same arrays): one particle, 63 and 65 particles (one wave with a padding lane; a second wave with one live lane) and fold_cloth1's
512-particle patch (8 full waves), at (S, T) = (1, 1) and (3, 2), B = 3, normalisation on and off, cotangents on the per-macro-step
lists or on the final state only, mode 0 -- cloth_rollout_bwd_fast_kernel in every case.  `_reference` itself is not called: it also
demands ground contact, and after ONE substep only the one-particle body (which starts on the ground) has any; every case grasps, and
every (3, 2) case touches the ground (tests/test_cloth_adjoint_bits_cases.py asserts both on the CPU oracle).

In all of those gripper 1 stays at (1, 1, 1) and holds nothing (tests/conftest.py::make_cloth_case), so the adjoint's wave-uniform
branch on ballot(m1) only ever takes its empty side.  The `two_grippers` cases add what that branch needs: gripper 1 is put on a
particle of the body's first wave, with a move and a suction of its own, so that it holds particles of some waves and of none in
others (asserted on the oracle's grasp sets by the same CPU test)."""
import zlib

import numpy as np

import cloth_adjoint_bar as cab

GOLDEN = "cloth_adjoint_bits.npz"
BODY_NAMES = ("one_particle", "rect7x9", "rect5x13", "patch16x32")
ST = ((1, 1), (3, 2))
B = 3
# (body, S, T, normalize, lists, two_grippers)
CASES = [(body, S, T, normalize, lists, False) for body in BODY_NAMES for (S, T) in ST for normalize in (True, False) for lists in (True, False)]
CASES += [(body, S, T, normalize, True, True) for body in ("rect5x13", "patch16x32") for (S, T) in ST for normalize in (True, False)]
_IN = {}


def case_id(body, S, T, normalize, lists, two):
    return f"{body}{'+g1' if two else ''}-S{S}T{T}-{'norm' if normalize else 'raw'}-{'lists' if lists else 'final'}"


def _two_grippers(case, seed):
    x, v, prim, k, mu, actions = case
    rng = np.random.default_rng(seed)
    P = x.shape[1]
    for b in range(B):
        p = rng.integers(0, min(P, 64))
        prim[b, 1, :3] = x[b, p] + np.float32([0, 0.002, 0])
    actions[..., 4:7] = (rng.normal(size=actions[..., 4:7].shape) * 0.3).astype(np.float32)
    actions[..., 7] = rng.uniform(0.2, 0.8, size=actions[..., 7].shape).astype(np.float32)
    return case


def inputs(body, S, T, lists, two=False):
    """-> (conf, mask, P, case, cotangents): `_reference`'s draws, in its order"""
    key = (body, S, T, lists, two)
    if key not in _IN:
        from test_cloth_adjoint_f64_gpu import BODIES, TWEAKS
        make, over, P = BODIES[body]
        mask = make()
        conf = cab.make_conf(substeps=S, **over)
        name = f"{body}/S{S}/B{B}/T{T}"
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        case = TWEAKS.get(body, lambda c: c)(cab.make_case(rng, conf, mask, B, T))
        g = cab.cotangents(rng, B, T, P, lists=lists)
        if two:
            case = _two_grippers(case, zlib.crc32((name + "/g1").encode()))
        _IN[key] = (conf, mask, P, case, g)
    return _IN[key]


def oracle_forward(body, S, T, two=False):
    """-> (grasp sets bool [substeps, B, 2, P], y of every substep's input [substeps, B, P]) of the order-2 CPU oracle"""
    conf, mask, P, case, _ = inputs(body, S, T, True, two)
    fwd = cab.make_oracle(conf, mask, 2).rollout_fwd(*case, want_lists=True, want_grasp=True, want_ckpt=True, nthreads=cab.NTHREADS)
    grasp = np.asarray(fwd["grasp"]).reshape(-1, B, 2, P) != 0
    y = fwd["ckpt"][..., :P * 3].reshape(-1, B, P, 3)[..., 1]
    return grasp, y


def waves_held(grasp, gripper):
    """-> bool [substeps, B, waves]: the gripper holds at least one particle of the wave"""
    g = grasp[:, :, gripper, :]
    P = g.shape[-1]
    nw = -(-P // 64)
    pad = np.zeros(g.shape[:2] + (nw * 64,), bool)
    pad[..., :P] = g
    return pad.reshape(g.shape[:2] + (nw, 64)).any(-1)


def run(body, S, T, normalize, lists, two):
    """the adjoint outputs (cab.KEYS) of the case on the GPU, float32"""
    from test_cloth_adjoint_f64_gpu import _sim
    from test_cloth_gpu import _run_hip
    _, _, _, case, g = inputs(body, S, T, lists, two)
    sim = _sim(body, 0, S, B)
    h = _run_hip(sim, *case, g=g, want_lists=True, normalize=normalize)
    sim.check_status()
    return {q: np.ascontiguousarray(h[q], np.float32) for q in cab.KEYS}
