"""CPU: the inputs of tests/test_cloth_decisions_gpu.py reach every value a decision word can take (tests/cloth_decisions_cases.py),
judged on the order-2 CPU oracle's forward alone -- its checkpoint records through the NumPy restatement of the words, and its own
grasp sets, which the restatement's mask bits must reproduce."""
import numpy as np
import pytest

import cloth_decisions_cases as dc

_W = {}


def _words(body, S, T, variant=""):
    key = (body, S, T, variant)
    if key not in _W:
        _W[key] = dc.oracle_words(body, S, T, variant)
    return _W[key]


@pytest.mark.parametrize("body", dc.BODY_NAMES)
def test_mask_bits_are_the_oracles_grasp_sets(body):
    w, grasp = _words(body, 3, 2)
    P = grasp.shape[-1]
    f = dc.fields(w)
    np.testing.assert_array_equal(np.moveaxis(f["m0"][..., :P], 0, 1) != 0, grasp[:, :, 0])
    np.testing.assert_array_equal(np.moveaxis(f["m1"][..., :P], 0, 1) != 0, grasp[:, :, 1])


@pytest.mark.parametrize("body", dc.BODY_NAMES)
def test_every_code_is_reached(body):
    w, grasp = _words(body, 3, 2)
    P = grasp.shape[-1]
    f = dc.fields(w)
    live = {q: a[:, :, :P] for q, a in f.items()}
    if P > 1:
        assert set(np.unique(live["m0"])) == {0, 1} and set(np.unique(live["m1"])) == {0, 1}
    else:   # the lone particle: gripper 0 displaces it out of gripper 1's reach
        assert set(np.unique(live["m0"])) == {0, 1}
    assert set(np.unique(live["dx"])) == {0, 1, 2}, "outside, on a bound, inside"
    held = (live["m0"] | live["m1"]) != 0
    assert (live["dx"][held] == 0).any(), "a held particle displaced out of [0, 1]"
    assert (live["dx"][~held][..., 1] == 1).any() if P > 1 else True, "a free particle exactly on the ground"
    assert set(np.unique(live["dv"])) == {0, 1}, "the velocity clip active and not"
    assert set(np.unique(f["prim"][:, :, :8])) == {0, 1, 2}, "a primitive component outside, on a bound, inside"
    assert not f["prim"][:, :, 8:].any(), "the primitive code lives in lanes 0-7"
    pad = w[:, :, P:]
    assert not (pad[:, :, max(8 - P, 0):]).any(), "padding lanes hold 0"
    assert not (pad & np.uint32((1 << dc.PRIM) - 1)).any(), "padding lanes hold 0 in every particle field"


@pytest.mark.parametrize("body", ("p257", "p449", "patch16x32"))
def test_gripper_1_holds_particles_of_some_waves_only(body):
    w, grasp = _words(body, 3, 2)
    m1 = dc.fields(w)["m1"][0]                                    # env 0: [T S, Pp]
    by_wave = m1.reshape(m1.shape[0], -1, 64).any(-1)
    assert by_wave.shape[1] > 1 and by_wave.any() and not by_wave.all(1).any()


@pytest.mark.parametrize("body", ("rect7x9", "p449"))
def test_input_radius_above_one_grasps_in_the_first_substep_only(body):
    """the first substep's threshold (radius 1.25 as given) holds particles that the later ones (radius clipped to 1) do not"""
    w, grasp = _words(body, 3, 2, "r0big")
    P = grasp.shape[-1]
    m0 = dc.fields(w)["m0"][..., :P]
    np.testing.assert_array_equal(np.moveaxis(m0, 0, 1) != 0, grasp[:, :, 0])
    x, prim = dc.inputs(body, 3, 2, "r0big")[3][0], dc.inputs(body, 3, 2, "r0big")[3][2]
    dist = np.linalg.norm(x.astype(np.float64) - prim[:, None, 0, :3], axis=-1)
    assert (dist > 1.0).all() and (dist < 1.25).all(), "out of reach of the clipped radius, within the radius as given"
    assert m0[:, 0].all(), "the first substep holds every particle"
    assert (m0[:, 1:] == 0).any(), "the later threshold decides on its own"
    assert (dc.fields(w)["prim"][:, 0, 3] == 0).all() and (dc.fields(w)["prim"][:, 1:, 3] == 1).all(), "radius 1.25 outside, then on the bound"


def test_grasp_thr_is_tight():
    for r in (0.0, 0.01, 0.5, 1.0, 1.25, 3.0e-20, np.float32(0.0125)):
        t = dc.grasp_thr(r)
        assert np.sqrt(t) <= np.float32(r) < np.sqrt(np.nextafter(t, np.float32(np.inf)))
    assert dc.grasp_thr(-1.0) == -1 and dc.grasp_thr(np.nan) == -1 and np.isinf(dc.grasp_thr(np.inf))
