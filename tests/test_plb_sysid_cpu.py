"""CPU: the host side of the PLB identification loop (unidom_amd/algorithms/plb_identify.py): the reference's Adam with its three learning
rates and the solver's pin / clip / floor against hand-computed steps and the NumPy twin (tests/plb_sysid_twin.py); MoveConf against the
values of sim2sim/plb/envs/move.yml; the command line's arguments; the new C entry points in the binding's symbol list."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tests import plb_sysid_twin as tw


def test_adam_twin_first_steps_by_hand():
    # step 1: m = 0.1 g, m_cap = g; v = 0.001 g^2, v_cap = g^2: the step is lr g / (|g| + eps).  A constant gradient repeats it:
    # step 2: m = 0.19 g, m_cap = 0.19 g / (1 - 0.81) = g; v = 0.001999 g^2, v_cap = v / (1 - 0.998001) = g^2
    g = np.array([[-2e-6, -1.5e-2, 4e-6], [1e-7, 2e-2, 0.0]])
    p0 = np.array([[3000.0, 0.3995, 200.0], [9000.0, 0.2005, 200.0]])
    lr = np.array([100.0, 100.0 / 50000, 100.0])
    unit = g / (np.abs(g) + 1e-8)
    opt = tw.AdamTwin(p0, lr=100.0)
    p1 = opt.step(g)
    assert np.allclose(p1, p0 - lr * unit, rtol=1e-15, atol=0)
    assert abs(p1[0, 0] - (3000 + 100 * 2e-6 / 2.01e-6)) < 1e-9 and abs(p1[1, 0] - (9000 - 100 * 1e-7 / 1.1e-7)) < 1e-9
    assert p1[1, 2] == 200.0                                      # a zero gradient moves nothing
    c1 = tw.constrain(p1)
    assert c1[0, 1] == 0.4 and c1[1, 1] == 0.2                    # nu left [0.2, 0.4] by 0.002 and was clipped
    assert np.all(c1[:, 2] == 200.0) and c1[0, 0] == p1[0, 0]     # yield stress pinned, E free
    p2 = opt.step(g)
    assert np.all(np.abs(p2 - (p0 - 2 * lr * unit)) <= 1e-14 * np.abs(p0))   # the optimiser went on from its own, unclipped parameters
    assert abs(p2[0, 1] - (0.3995 + 2 * 0.002 * 1.5e-2 / (1.5e-2 + 1e-8))) < 1e-15
    # real2sim: E is clipped as well; the floor catches what is left
    c = tw.constrain(np.array([[100.0, 0.3, -5.0], [20000.0, 0.3, 1.0]]), pin=(None, None, None), bounds=((500.0, 10700.0), (0.2, 0.4), (None, None)))
    assert np.array_equal(c, np.array([[500.0, 0.3, 0.01], [10700.0, 0.3, 1.0]]))


def test_parameter_adam_and_constrain_are_the_twin():
    import torch
    from unidom_amd.algorithms import plb_identify as pi
    rng = np.random.default_rng(0)
    p0 = np.array([[3000.0, 0.38, 200.0], [9000.0, 0.22, 200.0], [600.0, 0.399, 200.0]])
    ref, opt = tw.AdamTwin(p0, lr=100.0), pi.ParameterAdam(torch.tensor(p0), lr=100.0)
    for it in range(5):
        g = rng.normal(size=p0.shape) * np.array([1e-6, 1e-2, 1e-6])
        a, b = ref.step(g), opt.step(torch.tensor(g))
        assert np.abs(b.numpy() - a).max() <= 1e-12 * np.abs(a).max(), it
        for pin, bounds in (((None, None, 200.0), pi.SIM2SIM_BOUNDS), ((None, None, 200.0), pi.REAL2SIM_BOUNDS), ((None, None, None), pi.SIM2SIM_BOUNDS)):
            assert np.array_equal(pi.constrain(b, pin, bounds).numpy(), tw.constrain(b.numpy(), pin, bounds))
    assert pi.YIELD_STRESS == 200.0 and pi.REAL2SIM_BOUNDS[0] == (500.0, 10700.0) and pi.SIM2SIM_BOUNDS[1] == (0.2, 0.4) == pi.REAL2SIM_BOUNDS[1]


def test_truth_and_candidates_are_the_references_draws():
    from unidom_amd.algorithms import plb_identify as pi
    np.random.seed(7)
    E, nu = np.random.uniform(500, 10500), np.random.uniform(0.2, 0.4)
    np.random.seed(123)
    before = np.random.get_state()[1].copy()
    assert pi.draw_truth(7) == (E, nu)
    c = pi.draw_candidates(7, 3)
    assert np.array_equal(np.random.get_state()[1], before)      # the caller's stream is left alone
    for b in range(3):
        np.random.seed(7 + 10000000 + b)
        assert c[b, 0] == np.random.uniform(2000, 8000) and c[b, 1] == np.random.uniform(0.2, 0.4) and c[b, 2] == 200.0


def test_move_conf_is_move_yml():
    from unidom_amd.engine.plb_simulator import MoveConf, PlbConf
    c = MoveConf()
    # SIMULATOR of move.yml; E, nu, quality, dtype from default_config.py
    assert (c.yield_stress, c.gravity, c.ground_friction) == (1762.2, (0.0, -0.4, 0.0), 0.5)
    assert (c.E, c.nu, c.quality, c.dim, c.dtype) == (5e3, 0.35, 1.0, 3, "float64")
    # SHAPES
    assert (c.n_particles, c.box_width, c.box_init_pos) == (1000, (0.5, 0.028, 0.028), (0.5, 0.0125, 0.5))
    # PRIMITIVES: one Sphere
    assert (c.prim_kind, c.prim_radius, c.prim_init_pos) == ((0,), (0.025,), ((0.745, 0.02, 0.5),))
    assert c.action_scale == (0.005, 0.005, 0.005) and c.action_dim == 3 and not c.rot_state
    assert c.action_scale_on_host is True and PlbConf.action_scale_on_host is False
    assert not hasattr(c, "mu") and not hasattr(c, "lam")        # the file's mu / lam are read by nothing
    assert "mu" in MoveConf.__doc__ and "lam" in MoveConf.__doc__


def test_command_line_arguments():
    from unidom_amd.algorithms.plb_identify import build_parser
    ap = build_parser()
    a = ap.parse_args(["--env", "move", "--horizon", "5", "--iters", "3", "--num_envs", "2"])
    assert (a.env, a.horizon, a.iters, a.num_envs, a.seed, a.targets, a.lr) == ("move", 5, 3, 2, 0, None, 100.0)
    a = ap.parse_args(["--env", "writer", "--seed", "4", "--targets", "rec.npy"])
    assert (a.env, a.seed, a.targets) == ("writer", 4, "rec.npy")
    with pytest.raises(SystemExit):
        ap.parse_args(["--env", "torus"])


def test_new_entry_points_are_declared_and_bound():
    from unidom_amd import _lib
    src = open(os.path.join(ROOT, "include", "unidom_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    new = ["ud_plb_density_seq_work_bytes", "ud_plb_density_seq_sign_bytes", "ud_plb_density_seq_fwd", "ud_plb_density_seq_bwd", "ud_plb_chamfer"]
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SYMBOLS, name
    assert re.search(r"size_t\s+ud_plb_density_seq_work_bytes\s*\(\s*const ud_plb\*\s*h,\s*long M\)", src)
