"""GPU: every branch of the cloth dispatch (csrc/cloth.hip, ud_cloth_rollout_fwd / _bwd) at the smallest body that reaches it, the
forward bit for bit against the CPU oracle in the order the dispatch really runs (ClothSimulator.forward_order) and the adjoint
against the oracle's f64 adjoint along that f32 trajectory.

Every case:  forward (final state, per-macro-step lists, the grasp set of every substep) equal to ClothOracle(order) bit for bit;
every adjoint output within   |HIP - R64|max <= KAPPA |R32 - R64|max + REL_FLOOR |R64|max   (KAPPA = 4, REL_FLOOR = 1e-6 of
oracle/ref_chain.py; gx / gv once per env, the others over the whole tensor: tests/cloth_adjoint_bar.py); the f64 sweep followed
every grasp decision of the f32 forward; the case grasps and touches the ground, so gk and gmu are not 0 against 0 (the one-particle
body has no spring: there gk must be exactly 0); sim.check_status() at the end.  B = 3, T = 2 or 3, 7 substeps unless the name says
otherwise; cotangents on the final state and on the per-macro-step lists.

What reaches which kernel (Pp = particles padded to whole waves):
    Pp <= 512           1 / 63 / 65 particles and the 512-particle patch: cloth_rollout_fwd_v2 (mode 0), _fwd_ref (mode 3), the
                        literal <512> pair (mode 1), cloth_rollout_bwd_fast (modes 0, 3)
    512 < Pp <= 1024    513 / 697 / 1024 particles: cloth_rollout_fwd_kernel<1024> + cloth_rollout_bwd_kernel<1024> in modes 0, 1
                        and 2 alike -- reference order, literal adjoint (mode 3 is refused)
    Pp > 1024           1025 / 1101 / 1400 (tall strip) / 4096 particles on several workgroups (3, 3, 3, 8 parts; launch_envs of a
                        4096-env call is smaller than 4096), modes 0 (order 2) and 3 (order 1); mode 1 and the wide strip (a
                        spring spans 281 indices > 256: no halo, modes 0 / 2 / 3 without one_workgroup_per_env) on the
                        one-workgroup kernels cloth_big_fwd / _bwd (launch_envs(B) == B), reference order
`launch_envs(64) < 64` tells several workgroups from one only for bodies of five parts or more: a launch holds
8 * floor((CUs / 8) / parts) envs, 80 at three parts on 256 CUs.  The tests therefore assert the exact figure for 64 envs and
`launch_envs(4096) < 4096`, which holds for every body on several workgroups (a launch never holds more envs than the chip has CUs).

NOT MEASURED YET: the ratios |HIP - R64|max / |R32 - R64|max of these kernels on the MI355X.  Every case prints them (one ADJBAR line
per tensor under `pytest -s`); the CPU oracle passes every case's validity checks (finite, grasp, ground contact, flips = 0,
|R64|max > 0).  The table of ratios per kernel family, the committed log and the kernel trace of a band case
(`rocprofv3 --kernel-trace --stats` of test_band_ragged_disk_loop_edges, which must name cloth_rollout_fwd_kernel<1024> and
cloth_rollout_bwd_kernel<1024>) are still owed; KAPPA stays the project's 4 until a measured ratio says otherwise.
"""
import zlib

import numpy as np
import pytest
import torch

import cloth_adjoint_bar as cab
from test_cloth_gpu import _run_hip

pytestmark = pytest.mark.gpu

B3 = 3


def _big(N, dt):   # fold_cloth_tshirt_env.py:19-33 at the lattice of the body
    return dict(N=N, dt=dt, stiffness=5000, mu=0.9)


def _tshirt_mask():
    import os
    import unidom_amd.envs as envs
    return np.load(os.path.join(os.path.dirname(envs.__file__), "others", "tshirt_mask.npy")).astype(np.float32)


# body -> (mask builder, conf overrides, particles)
BODIES = {
    "one_particle": (lambda: cab.rect_mask(80, 1, 1, 40, 40), {}, 1),
    "rect7x9": (lambda: cab.rect_mask(80, 7, 9), {}, 63),
    "rect5x13": (lambda: cab.rect_mask(80, 5, 13), {}, 65),
    "patch16x32": (lambda: cab.rect_mask(80, 16, 32, 32, 32), {}, 512),         # fold_cloth1's
    "rect19x27": (lambda: cab.rect_mask(80, 19, 27), {}, 513),
    "disk697": (lambda: cab.disk_mask(80, 40, 37, 14.9), {}, 697),
    "rect32x32": (lambda: cab.rect_mask(80, 32, 32), {}, 1024),
    "rect25x41": (lambda: cab.rect_mask(80, 25, 41), {}, 1025),
    "disk1101": (lambda: cab.disk_mask(180, 90, 87, 18.7), _big(180, 0.5e-3), 1101),
    "rect64x64": (lambda: cab.rect_mask(80, 64, 64), {}, 4096),
    "strip_wide": (lambda: cab.slice_mask(300, 100, 105, 10, 290), _big(300, 0.25e-3), 1400),
    "strip_tall": (lambda: cab.slice_mask(300, 10, 290, 100, 105), _big(300, 0.25e-3), 1400),
    "tshirt": (_tshirt_mask, _big(180, 0.5e-3), 3573),
}


def _one_particle_on_the_ground(case):
    """A lone particle that a gripper carries (suction 0: v <- 0 v, x follows the gripper) has no velocity cotangent at all, and one
    in the air has no friction: gv and gmu would be 0 against 0.  So the particle starts on the ground (y = 0: the friction block
    runs every substep, with the drawn tangential velocity) under gripper 0, and every macro action has full suction (v <- 1 v, x
    stays): the grasp set is still recorded and differentiated (the suction cotangent), and it changes when the gripper moves off."""
    x, v, prim, k, mu, actions = case
    x[:, :, 1] = 0
    prim[:, 0, :3] = x[:, 0] + np.float32([0, 0.002, 0])
    actions[..., 3] = 1
    return case


TWEAKS = {"one_particle": _one_particle_on_the_ground}
_REF = {}     # (body, order, S, B, T, normalize, lists) -> (case, cotangents, oracle forward, R64, R32): computed once, only read after


def _reference(body, order, S, B, T, normalize, lists):
    key = (body, order, S, B, T, normalize, lists)
    if key not in _REF:
        make, over, P = BODIES[body]
        mask = make()
        assert int(mask.sum()) == P
        conf = cab.make_conf(substeps=S, **over)
        rng = np.random.default_rng(zlib.crc32(f"{body}/S{S}/B{B}/T{T}".encode()))     # the same inputs in every mode and order
        case = TWEAKS.get(body, lambda c: c)(cab.make_case(rng, conf, mask, B, T))
        g = cab.cotangents(rng, B, T, P, lists=lists)
        _REF[key] = (case, g) + cab.reference(cab.make_oracle(conf, mask, order), case, g, normalize=normalize)
    return _REF[key]


def _sim(body, mode, S, B, **extra):
    from unidom_amd.engine.cloth_simulator import ClothSimulator
    make, over, P = BODIES[body]
    conf = cab.make_conf(substeps=S, **over, **extra)
    sim = ClothSimulator(conf, B, lambda x, v, i, j: v, make(), mode=mode)
    assert sim.mode == mode and sim.n_particles == P
    return sim


def _parts(P):
    return -(-P // 512)


def _check_path(sim, several):
    """several workgroups per env or one, as the case expects, by ud_cloth_launch_envs"""
    P = sim.n_particles
    n_cu = torch.cuda.get_device_properties(sim.device).multi_processor_count
    assert sim.several_workgroups == several
    if several:
        per = 8 * ((n_cu // 8) // _parts(P))
        assert sim.launch_envs(4096) == per < 4096 and sim.launch_envs(64) == min(64, per), (per, sim.launch_envs(64))
        if per < 64:
            assert sim.launch_envs(64) < 64
    else:
        assert sim.launch_envs(4096) == 4096 and sim.launch_envs(64) == 64


def _run(body, mode, order, several, S=7, B=B3, T=2, normalize=True, lists=True, zero=(), **extra):
    sim = _sim(body, mode, S, B, **extra)
    assert sim.forward_order == order, (sim.forward_order, order)
    _check_path(sim, several)
    case, g, fwd, r64, r32 = _reference(body, order, S, B, T, normalize, lists)
    h = _run_hip(sim, *case, g=g, want_lists=True, normalize=normalize)
    cab.assert_forward_bit_exact(h, fwd)
    tag = f"{body}/mode{mode}/S{S}/B{B}/T{T}/{'norm' if normalize else 'raw'}/{'lists' if lists else 'final'}"
    rep = cab.assert_adjoint_within_bar(tag, h, r64, r32, zero=zero)
    sim.check_status()
    return h, rep


MODE_ORDER_SMALL = [(0, 2), (1, 1), (3, 1)]


# -- Pp <= 512 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,order", MODE_ORDER_SMALL)
@pytest.mark.parametrize("body", ["one_particle", "rect7x9", "rect5x13"])
def test_bodies_of_one_wave_and_one_particle_more(body, mode, order):
    """1 particle (no neighbour: no spring force, gk exactly 0), 63 (one wave with a padding lane), 65 (a second wave with one live
    lane): the block reductions of the adjoint with one and two waves, tables of padding lanes."""
    _run(body, mode, order, False, zero=("gk",) if body == "one_particle" else ())


@pytest.mark.parametrize("mode,order,normalize,lists,B", [
    (1, 1, True, True, 3), (1, 1, False, True, 3), (1, 1, True, False, 3),          # mode 1's literal adjoint
    (0, 2, True, True, 3), (0, 2, False, True, 3), (0, 2, True, False, 3),
    (3, 1, True, True, 3), (3, 1, False, True, 3), (3, 1, True, False, 3),
    (0, 2, True, True, 32), (3, 1, True, True, 32)])                                # 32 envs in one launch
def test_patch_of_512_particles_meets_the_f64_bar(mode, order, normalize, lists, B):
    """The adjoint cases tests/test_cloth_gpu.py holds to 2e-4 ... 1e-2 of the f32 oracle, at 7 substeps against the f64 bar."""
    _run("patch16x32", mode, order, False, B=B, T=3 if B == 3 else 2, normalize=normalize, lists=lists)


# -- 512 < Pp <= 1024: mode 1's kernels in every mode ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_band_first_size_runs_reference_order_in_modes_0_1_2(mode):
    """513 particles (Pp = 576), the first size of cloth_rollout_{fwd,bwd}_kernel<1024>: modes 0, 1 and 2 all give the order-1
    oracle's bits (include/unidom_hip.h, "Bodies of 513-1024 particles") and the literal adjoint within the bar."""
    _run("rect19x27", mode, 1, False)


def test_band_is_not_order_v2_and_mode_3_is_refused():
    """the order-2 restatement lands elsewhere on the same inputs (so the bit-exact check above tells the orders apart), and mode 3
    has no kernel in the band"""
    from unidom_amd import _lib
    case, g, fwd1 = _reference("rect19x27", 1, 7, B3, 2, True, True)[:3]
    make, over, _ = BODIES["rect19x27"]
    fwd2 = cab.make_oracle(cab.make_conf(**over), make(), 2).rollout_fwd(*case)
    assert not np.array_equal(fwd2["v"], fwd1["v"])
    with pytest.raises(_lib.UnidomError, match="status -2"):
        _sim("rect19x27", 3, 7, B3)


@pytest.mark.parametrize("S,T,normalize,lists", [(7, 2, True, True), (7, 3, False, True), (7, 2, True, False), (1, 2, True, True),
                                                 (1, 3, False, False), (2, 3, True, False), (2, 2, False, True)])
def test_band_ragged_disk_loop_edges(S, T, normalize, lists):
    """697 particles (Pp = 704, 7 padding lanes in the last of 11 waves), mode 0: the un-normalised adjoint, one and two substeps
    per macro step (the forward's step-parity LDS buffers and the adjoint's reduction slots across macro steps), cotangents on the
    final state only."""
    _run("disk697", 0, 1, False, S=S, T=T, normalize=normalize, lists=lists)


@pytest.mark.parametrize("mode,S", [(0, 7), (2, 7), (1, 50)])
def test_band_full_workgroup_of_1024_lanes(mode, S):
    """1024 particles: 16 full waves, no padding lane; once over 2 x 50 substeps."""
    _run("rect32x32", mode, 1, False, S=S)


# -- Pp > 1024 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,order,several", [(0, 2, True), (3, 1, True), (1, 1, False)])
def test_smallest_body_on_several_workgroups(mode, order, several):
    """1025 particles (Pp = 1088): three parts, the last one with ONE live particle (and 63 padding lanes in its only wave that
    matters); mode 1 keeps the body on one workgroup, reference order."""
    _run("rect25x41", mode, order, several)


@pytest.mark.parametrize("mode,order", [(0, 2), (3, 1)])
def test_ragged_last_part(mode, order):
    """1101 particles of a disk on the 180 lattice: three parts, 77 live particles in the last, rows of varying length"""
    _run("disk1101", mode, order, True)


@pytest.mark.parametrize("mode,order,several", [(0, 2, True), (3, 1, True), (1, 1, False)])
def test_largest_body(mode, order, several):
    """4096 particles: eight full parts, the most ud_cloth_create accepts for several workgroups; mode 1: four particles in every
    lane of the one-workgroup kernels"""
    _run("rect64x64", mode, order, several)


def test_one_particle_more_than_the_largest_body_is_refused():
    from unidom_amd import _lib
    from unidom_amd.engine.cloth_simulator import ClothSimulator
    mask = cab.rect_mask(80, 64, 65)
    assert int(mask.sum()) == 4160
    m = cab.rect_mask(80, 64, 64)
    m[8 + 64, 8] = 1                     # 4097
    for bad in (mask, m):
        with pytest.raises(_lib.UnidomError, match=r"status -2.*P=%d" % int(bad.sum())):
            ClothSimulator(cab.make_conf(), 1, lambda x, v, i, j: v, bad)


@pytest.mark.parametrize("mode", [0, 2, 3])
def test_body_whose_springs_span_more_than_the_widest_halo(mode):
    """5 rows of 280 particles: a spring to the next row spans 281 particle indices > 256, the body does not qualify for several
    workgroups, and modes 0, 2 and 3 run the one-workgroup reference-order kernels without one_workgroup_per_env being asked."""
    assert cab.spring_span(BODIES["strip_wide"][0]()) == 281
    _run("strip_wide", mode, 1, False)


@pytest.mark.parametrize("mode,order", [(0, 2), (3, 1)])
def test_same_particle_count_with_short_springs_qualifies(mode, order):
    """the strip turned by a quarter: 280 rows of 5, span 6, three parts"""
    assert cab.spring_span(BODIES["strip_tall"][0]()) == 6
    _run("strip_tall", mode, order, True)


@pytest.mark.parametrize("mode,order", [(3, 1), (0, 2)])
def test_tshirt_call_cut_into_two_launches_every_env(mode, order):
    """38 T-shirt envs (7 parts each) at 3 substeps: two launches (32 + 6 on 256 CUs); gx and gv within the bar in EVERY env,
    whichever launch it ran in"""
    B = 38
    sim = _sim("tshirt", mode, 3, B)
    assert sim.launch_envs(B) < B
    del sim
    _run("tshirt", mode, order, True, S=3, B=B, T=2)
