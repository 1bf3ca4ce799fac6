"""GPU: the one-workgroup cloth rollout kernels on bodies whose last wave has ONE live lane and shares its SIMD
(tests/cloth_bwd_ragged_cases.py: 257 particles = five waves, 449 = eight waves with P != Pp).

Adjoint (cloth_rollout_bwd_fast_ragged_kernel / _ragged_raw_kernel, csrc/cloth_fast_bwd.hip: the kernels of a body with padding lanes;
a body that fills its waves runs the same loop without the `live` selects and is held by tests/test_cloth_adjoint_bits_gpu.py and
tests/test_cloth_bwd_unroll_bits_gpu.py at 512 particles): every output is the recorded bits of
tests/golden/cloth_bwd_ragged_bits.npz, written by tools/record_cloth_adjoint_bits.py --cases cloth_bwd_ragged_cases against a build
of the commit BEFORE these tests were added, on an MI355X.  The kernel's roundings are written out in its source, so nothing a later
change does to its loop (kernels split by P == Pp, an unrolled substep loop, a carried grasp threshold, a rotated back-edge) may move
a bit here: padding lanes, the lone live lane of a wave that runs the priority hand-over copy, the first substep's own threshold and a
gripper-1 branch taken by the ragged wave alone are what those changes touch and the older recorded cases do not reach.

Forward (cloth_rollout_fwd_v2_kernel with checkpoints, cloth_rollout_fwd_v2_eval_kernel without): final state, per-macro-step lists
and the x, v and primitive row of every recorded substep bit for bit against ClothOracle(order=2), same bodies, S in {1, 2, 3} x
T in {1, 2}; and one launch whose constants fail cloth_isv_consts_ok (small_num below 2^-96), so that the `_anyc` kernels run the same
loop."""
import os

import numpy as np
import pytest
import torch

import cloth_adjoint_bar as cab
import cloth_bwd_ragged_cases as cc

pytestmark = pytest.mark.gpu

_REF = {}     # oracle forwards, computed once per key, only read after


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", cc.GOLDEN))


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: cc.case_id(*c))
def test_adjoint_outputs_are_the_recorded_bits(golden, case):
    h = cc.run(*case)
    bad = []
    for q in cab.KEYS:
        got, want = h[q].view(np.uint32), golden[f"{cc.case_id(*case)}/{q}"].view(np.uint32)
        assert got.shape == want.shape, (q, got.shape, want.shape)
        n = int((got != want).sum())
        if n:
            d = np.abs(h[q].astype(np.float64) - want.view(np.float32).astype(np.float64)).max()
            print(f"BITS {cc.case_id(*case)}/{q}: {n} of {got.size} words differ, max |diff| {d:.3e}")
            bad.append(q)
    assert not bad, f"differing tensors: {bad}"


def _records(ckpt, P, T, S):
    """the forward's checkpoint arena -> x, v (B, T S, P, 3) and primitives (B, T S, 2, 4) of every substep's input"""
    B = cc.B
    Pp = -(-P // 64) * 64
    rec = 6 * Pp + 8
    n = B * (T * S + 1) * rec
    assert ckpt.numel() >= n
    r = ckpt[:n].cpu().numpy().reshape(B, T * S + 1, rec)[:, :T * S]
    planes = r[..., :6 * Pp].reshape(B, T * S, 6, Pp)[..., :P]
    return np.moveaxis(planes[:, :, :3], 2, -1), np.moveaxis(planes[:, :, 3:], 2, -1), r[..., 6 * Pp:].reshape(B, T * S, 2, 4)


def _forward(body, S, T, **extra):
    """both forward kernels of the launch's family against the oracle of the same constants"""
    from unidom_amd.engine.cloth_simulator import _Rollout
    P = cc.BODIES[body][1]
    B = cc.B
    conf, mask, _, case, _ = cc.inputs(body, S, T)
    key = (body, S, T, tuple(sorted(extra.items())))
    if key not in _REF:
        oconf = cab.make_conf(substeps=S, **extra)
        _REF[key] = cab.make_oracle(oconf, mask, 2).rollout_fwd(*case, want_lists=True, want_ckpt=True, nthreads=cab.NTHREADS)
    fwd = _REF[key]
    sim = cc.sim_of(body, S, **extra)
    for ckpt in (True, False):
        t = lambda a: torch.tensor(a, device=sim.device, requires_grad=ckpt)
        if ckpt:
            out = _Rollout.apply(sim, *(t(a) for a in case), True)
        else:
            with torch.no_grad():
                out = _Rollout.apply(sim, *(t(a) for a in case), True)
        assert (out[0].grad_fn is not None) == ckpt and sim.last_grasp is None
        for q, o in zip(cab.FWD_KEYS, out):
            np.testing.assert_array_equal(o.detach().cpu().numpy(), fwd[q], err_msg=f"{q} (checkpoints {ckpt})")
        if ckpt:
            hx, hv, hp = _records(out[0].grad_fn.saved_tensors[0], P, T, S)
            ck = fwd["ckpt"].reshape(B, T * S, 6 * P + 8)
            np.testing.assert_array_equal(hx, ck[..., :3 * P].reshape(B, T * S, P, 3), err_msg="x of every substep")
            np.testing.assert_array_equal(hv, ck[..., 3 * P:6 * P].reshape(B, T * S, P, 3), err_msg="v of every substep")
            np.testing.assert_array_equal(hp, ck[..., 6 * P:].reshape(B, T * S, 2, 4), err_msg="primitives of every substep")
    sim.check_status()


@pytest.mark.parametrize("T", cc.T_GRID)
@pytest.mark.parametrize("S", cc.S_GRID)
@pytest.mark.parametrize("body", list(cc.BODIES))
def test_forward_bit_exact_every_substep(body, S, T):
    _forward(body, S, T)


def test_forward_bit_exact_with_constants_outside_the_isv_range():
    """small_num = 1e-30 < 2^-96: cloth_isv_consts_ok refuses the launch's constants and the `_anyc` kernels run"""
    assert 1e-30 < 2.0 ** -96
    _forward("p449", 3, 2, small_num=1e-30)
