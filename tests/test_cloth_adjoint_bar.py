"""CPU: what the f64 bar of tests/cloth_adjoint_bar.py sees that the older max-norm tolerances do not.

The kernel-level adjoint tests used to compare with `|HIP - R32|max / |R32|max < tol`, tol between 2e-4 and 1e-2, against the
oracle's f32 adjoint.  Over a short horizon (7 substeps, 3 macro steps) an adjoint computed with a time step that is wrong by 1e-5
relative stays below the loosest of those tolerances on every tensor -- and is several bars away from the f64 adjoint R64 on the
state, stiffness and friction gradients.  (At 50 substeps the system amplifies the same error to 5 % - 47 %; short horizons are where
the old tolerances were blind.)  The unperturbed f32 adjoint passes the bar, by construction with a ratio of 1.
"""
import numpy as np
import pytest

import cloth_adjoint_bar as cab
from conftest import fold_cloth1_mask

LOOSEST_OLD_TOL = 5e-3      # tests/test_cloth_gpu.py: `_rel(h, o) < 5e-3` (the 2000-substep cases; the short ones use 2e-4 ... 1e-3)


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


@pytest.mark.parametrize("order", [1, 2])
def test_a_time_step_off_by_1e_5_passes_the_old_tolerance_and_fails_the_f64_bar(order):
    B, T, S = 3, 3, 7
    mask = fold_cloth1_mask()
    conf = cab.make_conf(substeps=S)
    rng = np.random.default_rng(107)
    case = cab.make_case(rng, conf, mask, B, T)
    g = cab.cotangents(rng, B, T, int(mask.sum()))
    fwd, r64, r32 = cab.reference(cab.make_oracle(conf, mask, order), case, g, nthreads=4)
    wrong = cab.make_oracle(cab.make_conf(substeps=S, dt=conf.dt * (1 + 1e-5)), mask, order)
    gl = (g["gx_list"], g["gv_list"], g["gprim_list"])
    bad = wrong.rollout_bwd(*case, g["gx"], g["gv"], g["gprim"], *gl, nthreads=4, adjoint_dtype=np.float32)
    # the old check passes it, on every tensor
    for q in cab.KEYS:
        assert _rel(bad[q], r32[q]) < LOOSEST_OLD_TOL, (q, _rel(bad[q], r32[q]))
    # the bar does not
    rep = cab.adjoint_bar_report(f"dt_off_by_1e-5/order{order}", bad, r64, r32)
    for q in ("gx", "gv", "gk", "gmu"):
        assert rep[q][0] > 1.0, (q, rep[q])
    with pytest.raises(AssertionError, match="over the bar"):
        cab.assert_adjoint_within_bar(f"dt_off_by_1e-5/order{order}", bad, r64, r32)
    # and the true f32 adjoint passes
    ok = cab.assert_adjoint_within_bar(f"true_f32/order{order}", r32, r64, r32)
    assert all(v[0] < 1.0 for v in ok.values())


def test_the_bar_is_applied_per_env_to_the_state_gradients():
    """an error confined to the env with the smallest gradient is judged against that env's own maxima, not the tensor's"""
    rng = np.random.default_rng(0)
    r64 = {q: rng.normal(size=s) for q, s in (("gx", (3, 5, 3)), ("gv", (3, 5, 3)), ("gprim", (3, 2, 4)), ("gactions", (2, 3, 8)), ("gk", (3,)), ("gmu", (3,)))}
    r64["gx"][1] *= 1e-3
    r32 = {q: a + 1e-7 * np.abs(a).max() * rng.normal(size=a.shape) for q, a in r64.items()}
    r32["gx"][1] = r64["gx"][1] * (1 + 1e-7)
    hip = {q: a.copy() for q, a in r32.items()}
    cab.assert_adjoint_within_bar("synthetic/true", hip, r64, r32)
    hip["gx"][1] = r64["gx"][1] * (1 + 1e-4)      # 1e-7 of the whole tensor's maximum: inside a whole-tensor bar, far outside env 1's
    assert np.abs(hip["gx"] - r64["gx"]).max() < cab.rc.bar(r64["gx"], r32["gx"])
    with pytest.raises(AssertionError, match="over the bar"):
        cab.assert_adjoint_within_bar("synthetic/env1", hip, r64, r32)
