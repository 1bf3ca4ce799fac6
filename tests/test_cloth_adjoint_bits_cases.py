"""CPU: what the cases of tests/cloth_adjoint_bits_cases.py exercise, checked on the order-2 oracle's forward (no GPU): every case
grasps; every (3, 2) case and the one-particle body put a particle on the ground (the friction block of the adjoint runs); and in
every two-gripper case gripper 1 holds particles of some waves and of none in others at some substep, so both sides of the
wave-uniform ballot branch of cloth_rollout_bwd_fast_kernel are in the recorded bits."""
import numpy as np
import pytest

import cloth_adjoint_bar as cab
import cloth_adjoint_bits_cases as cc

SHAPES = sorted({(c[0], c[1], c[2], c[5]) for c in cc.CASES})


@pytest.mark.parametrize("body,S,T,two", SHAPES)
def test_case_grasps_touches_the_ground_and_splits_the_ballot(body, S, T, two):
    grasp, y = cc.oracle_forward(body, S, T, two)
    assert grasp[:, :, 0].any(), "gripper 0 must hold something"
    if (S, T) == (3, 2) or body == "one_particle":
        assert (y[:S * T] <= np.float32(cab.Conf.small_num)).any(), "a substep's input must have a particle on the ground"
    if two:
        w = cc.waves_held(grasp, 1)
        assert (w.any(-1) & ~w.all(-1)).any(), "gripper 1 must hold particles in one wave and none in another"
    else:
        assert not grasp[:, :, 1].any()


def test_golden_file_has_exactly_the_cases():
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", cc.GOLDEN))
    want = {f"{cc.case_id(*c)}/{q}" for c in cc.CASES for q in cab.KEYS}
    assert set(z.files) == want
    assert all(z[n].dtype == np.float32 for n in z.files)
