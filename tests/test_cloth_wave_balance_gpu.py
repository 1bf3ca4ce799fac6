"""GPU: the one-workgroup cloth rollout kernels (csrc/cloth_v2.hip, cloth_fast_bwd.hip) at the body sizes where their per-wave
issue-priority code takes different paths.

A wave of a body of 257-512 padded particles that shares its SIMD with an earlier-dispatched wave (wave w >= 4, partner w - 4) runs a
copy of the substep loop that raises and drops its issue priority inside every barrier interval; every other wave runs the copy
without.  Nothing of that may move a bit.  Bodies: 256 particles (4 waves: no wave has a partner), 257 (5 waves: one SIMD holds two),
448 (7 waves: three SIMDs), 512 (8 waves: all four).  Both grippers hold particles, each in a few waves only (asserted), so that
waves of both loop copies see grasped and free particles and the adjoint's per-wave gripper-1 branch goes both ways in one workgroup.

Forward: bit for bit against ClothOracle(order=2) -- final state, per-macro-step lists, the grasp set of every substep, and with
checkpoints the recorded x, v and primitives of EVERY substep -- for T in {1, 2} x S in {1, 2, 3} (the unrolled pair, its odd tail,
a macro-step edge behind either), through all four forward kernels (checkpoints on / off x grasp sets on / off).
Adjoint: (T, S) in {(1,1), (2,1), (2,3), (3,2)}, normalize on and off, with and without the per-macro-step cotangent lists, held to
the f64 adjoint with the bar of tests/cloth_adjoint_bar.py exactly as tests/test_cloth_adjoint_f64_gpu.py does.
"""
import zlib

import numpy as np
import pytest
import torch

import cloth_adjoint_bar as cab
from test_cloth_gpu import _run_hip

pytestmark = pytest.mark.gpu

B = 3


def _rect_plus_one():
    m = cab.rect_mask(80, 16, 16)
    m[8 + 16, 8] = 1     # one particle more, last in particle order: the only live lane of wave 4
    return m


# body -> (mask builder, particles, waves)
BODIES = {
    "p256": (lambda: cab.rect_mask(80, 16, 16), 256, 4),
    "p257": (_rect_plus_one, 257, 5),
    "p448": (lambda: cab.rect_mask(80, 14, 32), 448, 7),
    "p512": (lambda: cab.rect_mask(80, 16, 32, 32, 32), 512, 8),
}
_REF = {}     # computed once per key, only read after


def _case(body, S, T):
    """make_cloth_case on the body, then gripper 1 as well: on a particle of the LAST wave in env 0, of wave 0 in env 1, nowhere in env 2;
    gripper 0 sits where make_cloth_case drew it.  Both move and have a suction between 0 and 1.  Every seventh particle starts on the
    ground, so that the friction block runs in a rollout of one substep too."""
    key = ("case", body, S, T)
    if key not in _REF:
        make, P, waves = BODIES[body]
        mask = make()
        assert int(mask.sum()) == P and -(-P // 64) == waves
        conf = cab.make_conf(substeps=S)
        rng = np.random.default_rng(zlib.crc32(f"wave_balance/{body}/S{S}/T{T}".encode()))
        x, v, prim, k, mu, actions = cab.make_case(rng, conf, mask, B, T)
        x[:, ::7, 1] = 0                                   # particles on the ground from the first record on: (T, S) = (1, 1) has no other
        for b, p in ((0, P - 1), (1, 5)):
            prim[b, 1, :3] = x[b, p] + np.float32([0, 0.002, 0])
        actions[..., 4:7] = (rng.normal(size=(T, B, 3)) * 0.3).astype(np.float32)
        actions[..., 7] = rng.uniform(0.2, 0.9, size=(T, B)).astype(np.float32)
        _REF[key] = (conf, mask, [x, v, prim, k, mu, actions])
    return _REF[key]


def _forward_reference(body, S, T):
    key = ("fwd", body, S, T)
    if key not in _REF:
        conf, mask, case = _case(body, S, T)
        P, waves = BODIES[body][1:]
        fwd = cab.make_oracle(conf, mask, 2).rollout_fwd(*case, want_lists=True, want_grasp=True, want_ckpt=True, nthreads=cab.NTHREADS)
        ck = fwd["ckpt"]                                   # (B, T, S, 6 P + 8): the INPUT state of every substep
        np.testing.assert_array_equal(ck[:, 0, 0, :3 * P].reshape(B, P, 3), case[0])      # the layout this file assumes
        np.testing.assert_array_equal(ck[:, 0, 0, 3 * P:6 * P].reshape(B, P, 3), case[1])
        np.testing.assert_array_equal(ck[:, 0, 0, 6 * P:].reshape(B, 2, 4), case[2])
        held = fwd["grasp"].any(axis=(0, 1))               # (B, 2, P)
        for g in (0, 1):
            per_wave = [held[0, g, w * 64:(w + 1) * 64].any() for w in range(waves)]
            assert any(per_wave) and not all(per_wave), (body, g, per_wave, "env 0: the gripper must hold particles of some waves only")
        assert held[0, 1, (waves - 1) * 64:].any() and held[1, 1, :64].any() and not held[2, 1].any()
        _REF[key] = fwd
    return _REF[key]


def _sim(body, S):
    from unidom_amd.engine.cloth_simulator import ClothSimulator
    make, P, _ = BODIES[body]
    sim = ClothSimulator(cab.make_conf(substeps=S), B, lambda x, v, i, j: v, make(), mode=0)
    assert sim.mode == 0 and sim.n_particles == P and sim.forward_order == 2 and not sim.several_workgroups
    return sim


def _records(ckpt, P, T, S):
    """the forward's checkpoint arena -> x, v (B, T S, P, 3) and primitives (B, T S, 2, 4) of every substep's input"""
    Pp = -(-P // 64) * 64
    rec = 6 * Pp + 8
    n = B * (T * S + 1) * rec
    assert ckpt.numel() >= n
    r = ckpt[:n].cpu().numpy().reshape(B, T * S + 1, rec)[:, :T * S]
    planes = r[..., :6 * Pp].reshape(B, T * S, 6, Pp)[..., :P]
    return np.moveaxis(planes[:, :, :3], 2, -1), np.moveaxis(planes[:, :, 3:], 2, -1), r[..., 6 * Pp:].reshape(B, T * S, 2, 4)


@pytest.mark.parametrize("ckpt", [True, False])
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("body", list(BODIES))
def test_forward_bit_exact_every_substep(body, T, S, ckpt):
    from unidom_amd.engine.cloth_simulator import _Rollout
    P = BODIES[body][1]
    case = _case(body, S, T)[2]
    fwd = _forward_reference(body, S, T)
    sim = _sim(body, S)
    t = lambda a: torch.tensor(a, device=sim.device, requires_grad=ckpt)
    for grasp in (True, False):          # the four kernels: (checkpoints, grasp sets) on / off
        sim.record_grasp = grasp
        try:
            if ckpt:
                out = _Rollout.apply(sim, *(t(a) for a in case), True)
            else:
                with torch.no_grad():
                    out = _Rollout.apply(sim, *(t(a) for a in case), True)
        finally:
            sim.record_grasp = False
        assert (out[0].grad_fn is not None) == ckpt and (sim.last_grasp is not None) == grasp
        for q, o in zip(cab.FWD_KEYS, out):
            np.testing.assert_array_equal(o.detach().cpu().numpy(), fwd[q], err_msg=f"{q} (grasp sets {grasp})")
        if grasp:
            np.testing.assert_array_equal(sim.last_grasp.cpu().numpy(), fwd["grasp"])
        if ckpt:
            hx, hv, hp = _records(out[0].grad_fn.saved_tensors[0], P, T, S)
            ck = fwd["ckpt"].reshape(B, T * S, 6 * P + 8)
            np.testing.assert_array_equal(hx, ck[..., :3 * P].reshape(B, T * S, P, 3), err_msg="x of every substep")
            np.testing.assert_array_equal(hv, ck[..., 3 * P:6 * P].reshape(B, T * S, P, 3), err_msg="v of every substep")
            np.testing.assert_array_equal(hp, ck[..., 6 * P:].reshape(B, T * S, 2, 4), err_msg="primitives of every substep")
    sim.check_status()


def _adjoint_reference(body, S, T, normalize, lists):
    key = ("adj", body, S, T, normalize, lists)
    if key not in _REF:
        conf, mask, case = _case(body, S, T)
        P = BODIES[body][1]
        rng = np.random.default_rng(zlib.crc32(f"wave_balance/cot/{body}/S{S}/T{T}".encode()))
        g = cab.cotangents(rng, B, T, P, lists=lists)
        _REF[key] = (g,) + cab.reference(cab.make_oracle(conf, mask, 2), case, g, normalize=normalize)
    return _REF[key]


@pytest.mark.parametrize("lists", [True, False])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("T,S", [(1, 1), (2, 1), (2, 3), (3, 2)])
@pytest.mark.parametrize("body", list(BODIES))
def test_adjoint_within_the_f64_bar(body, T, S, normalize, lists):
    case = _case(body, S, T)[2]
    g, fwd, r64, r32 = _adjoint_reference(body, S, T, normalize, lists)
    sim = _sim(body, S)
    h = _run_hip(sim, *case, g=g, want_lists=True, normalize=normalize)
    cab.assert_forward_bit_exact(h, fwd)
    tag = f"{body}/S{S}/T{T}/{'norm' if normalize else 'raw'}/{'lists' if lists else 'final'}"
    zero = tuple(q for q in cab.KEYS if not np.asarray(r64[q]).any() and not np.asarray(r32[q]).any())   # 0 against 0: HIP must be exactly 0
    cab.assert_adjoint_within_bar(tag, h, r64, r32, zero=zero)
    sim.check_status()
