"""CPU: the cases of tests/cloth_bwd_ragged_cases.py are what their names say, checked on the order-2 oracle's forward (no GPU): the
bodies have the wave layout the kernels' per-wave code depends on; every case grasps and has particles on the ground at every substep's
input; `+g1last` has gripper 1 on particles of the LAST wave only (in some env at some substep it holds that wave's one live lane and
nothing of any other wave); `+r0big` has a first-substep grasp threshold of its own, and it decides otherwise than the later one would."""
import os

import numpy as np
import pytest

import cloth_adjoint_bar as cab
import cloth_bwd_ragged_cases as cc

SHAPES = sorted({(c[0], c[1], c[2], c[4]) for c in cc.CASES})


def test_bodies_have_a_one_lane_last_wave_on_a_shared_simd():
    for body, (make, P, waves) in cc.BODIES.items():
        mask = make()
        assert int(mask.sum()) == P and P % 64 == 1 and -(-P // 64) == waves
        assert 4 < waves <= 8, "the last wave must share its SIMD with wave (waves - 5): two waves per SIMD start at the fifth wave"
    assert cc.BODIES["p257"][2] == 5 and cc.BODIES["p449"][2] == 8      # one paired SIMD; every SIMD paired, P != Pp = 512


@pytest.mark.parametrize("body,S,T,variant", SHAPES)
def test_case_is_what_its_name_says(body, S, T, variant):
    P, waves = cc.BODIES[body][1:]
    case = cc.inputs(body, S, T, variant)[3]
    fwd = cc.oracle_forward(body, S, T, variant)
    for q in cab.FWD_KEYS:
        assert np.isfinite(fwd[q]).all(), q
    grasp = np.asarray(fwd["grasp"])                                     # (T, S, B, 2, P)
    assert grasp[:, :, :, 0].any(), "gripper 0 must hold something"
    y = fwd["ckpt"][..., :3 * P].reshape(cc.B, T * S, P, 3)[..., 1]
    assert (y <= np.float32(cab.Conf.small_num)).any(-1).all(), "every substep's input must have a particle on the ground"
    w1 = cc.waves_held(grasp, 1)                                         # (substeps, B, waves)
    if variant == "g1last":
        last_only = w1[..., -1] & ~w1[..., :-1].any(-1)
        assert last_only.any(), "gripper 1 must hold the last wave's live lane and nothing of another wave, somewhere"
        assert not w1[..., 0].any(), "gripper 1 stays away from the front of the body"
    else:
        assert not w1.any()
    r0 = case[2][:, 0, 3]
    if variant == "r0big":
        assert (r0 > 1).all() and (np.clip(r0, 0, 1) != r0).all(), "the first substep's threshold must differ from the later ones'"
        first = grasp.reshape((T * S,) + grasp.shape[2:])[0, :, 0]       # (B, P)
        d = np.linalg.norm(case[0].astype(np.float64) - case[2][:, None, 0, :3].astype(np.float64), axis=-1)
        assert first.all() and (d > 1.0 + 1e-3).all() and (d < float(cc.R0_BIG) - 1e-3).all(), \
            "every particle lies between the two radii: held on the first substep, and by the later threshold it would not be"
        assert not grasp.reshape((T * S,) + grasp.shape[2:])[1, :, 0].all()
    else:
        assert (r0 <= 1).all()


def test_golden_file_has_exactly_the_cases():
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", cc.GOLDEN))
    want = {f"{cc.case_id(*c)}/{q}" for c in cc.CASES for q in cab.KEYS}
    assert set(z.files) == want
    assert all(z[n].dtype == np.float32 for n in z.files)
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", cc.GOLDEN)) < 561 * 1024
