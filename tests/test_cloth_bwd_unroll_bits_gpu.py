"""The one-workgroup cloth adjoint (csrc/cloth_fast_bwd.hip) at substep counts that the 40 cases of test_cloth_adjoint_bits_gpu.py do not
reach: S in {2, 3, 5} x T in {1, 2} (tests/cloth_bwd_unroll_cases.py says what each is for), on a ragged and on a full body (P < Pp and
P == Pp), normalised and raw, and once with gripper 1 holding.

tests/golden/cloth_bwd_unroll_bits.npz (534 KB, almost all of it the twelve 512-particle cases' gx and gv) holds every adjoint output
of these cases as raw f32, recorded by tools/record_cloth_adjoint_bits.py --cases cloth_bwd_unroll_cases on an MI355X from the kernel
with one substep per loop trip.  Any rework of that loop -- unrolling, a carried grasp threshold, kernels per body shape -- has to
return these words; the bar is equality of every word."""
import os

import numpy as np
import pytest

import cloth_adjoint_bar as cab
import cloth_bwd_unroll_cases as uc


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", uc.GOLDEN))


@pytest.mark.gpu
@pytest.mark.parametrize("case", uc.CASES, ids=lambda c: uc.case_id(*c))
def test_adjoint_outputs_are_the_recorded_bits_at_every_loop_parity(golden, case):
    h = uc.run(*case)
    bad = []
    for q in cab.KEYS:
        got, want = h[q].view(np.uint32), golden[f"{uc.case_id(*case)}/{q}"].view(np.uint32)
        assert got.shape == want.shape, (q, got.shape, want.shape)
        n = int((got != want).sum())
        if n:
            d = np.abs(h[q].astype(np.float64) - want.view(np.float32).astype(np.float64)).max()
            print(f"BITS {uc.case_id(*case)}/{q}: {n} of {got.size} words differ, max |diff| {d:.3e}")
            bad.append(q)
    assert not bad, f"differing tensors: {bad}"


def test_the_cases_reach_what_they_are_for():
    """CPU oracle: every case grasps with gripper 0; the two-gripper case has gripper 1 holding a particle in some substep and none in
    another wave of the same substep (the adjoint's wave-uniform branch takes both sides)."""
    ids = [uc.case_id(*c) for c in uc.CASES]
    assert len(set(ids)) == len(ids)
    assert {(c[1], c[2]) for c in uc.CASES} == {(S, T) for S in (2, 3, 5) for T in (1, 2)}
    for body, S, T in {(c[0], c[1], c[2]) for c in uc.CASES if not c[5]}:
        grasp, _ = uc.oracle_forward(body, S, T)
        assert grasp[:, :, 0, :].any(), (body, S, T)
    body, S, T = next((c[0], c[1], c[2]) for c in uc.CASES if c[5])
    grasp, _ = uc.oracle_forward(body, S, T, True)
    held = uc.cc.waves_held(grasp, 1)
    assert held.any() and (held.any(-1) & ~held.all(-1)).any()
