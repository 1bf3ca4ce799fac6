"""Shared by tests/test_cloth_bwd_ragged_bits_gpu.py, tests/test_cloth_bwd_ragged_cases.py and tools/record_cloth_adjoint_bits.py
(--cases cloth_bwd_ragged_cases): bodies whose last wave is ragged AND shares its SIMD, which the recorded adjoint bits of
tests/cloth_adjoint_bits_cases.py (1 / 63 / 65 / 512 particles) and tests/cloth_bwd_unroll_cases.py (65 / 512) do not reach:

    p257:  five waves.  Wave 4 shares its SIMD with wave 0 and runs the hand-over copy of the substep loop (WavePrio, csrc/cloth_common.h)
           with ONE live lane; waves 1-3 have no partner.
    p449:  eight waves, P != Pp = 512.  Every SIMD is paired and the last wave has one live lane.

S in {1, 2, 3} x T in {1, 2} (a lone substep, a pair, a pair and a tail; with and without a macro-step edge behind them), normalised
and raw, per-macro-step cotangents on, B = 2 envs (the golden file stays below that of cloth_adjoint_bits.npz with every case kept).
Every case starts every seventh particle on the ground, so that the friction block runs in a rollout of one substep too.

Three more cases, (S, T) = (3, 2), normalised:
    +g1last (both bodies): gripper 1 sits on the LAST particle, the one live lane of the last wave, and holds particles of that wave
           only -- the wave-uniform ballot(m1) branch of the adjoint is taken by the ragged wave alone.
    +r0big (p449): the rollout's input radius of gripper 0 is above 1 and its position off the body, so the first substep's grasp
           threshold (from the radius as given) differs from every later one's (from clip(radius, 0, 1)) and so do the grasp sets.
tests/test_cloth_bwd_ragged_cases.py asserts all of that on the CPU oracle."""
import zlib

import numpy as np

import cloth_adjoint_bar as cab

GOLDEN = "cloth_bwd_ragged_bits.npz"
B = 2


def _rect_plus_one(rows, cols):
    def make():
        m = cab.rect_mask(80, rows, cols)
        m[8 + rows, 8] = 1     # one particle more, last in particle order: the only live lane of the last wave
        return m
    return make


# body -> (mask builder, particles, waves)
BODIES = {"p257": (_rect_plus_one(16, 16), 257, 5), "p449": (_rect_plus_one(16, 28), 449, 8)}
S_GRID, T_GRID = (1, 2, 3), (1, 2)
R0_BIG = np.float32(1.25)
# (body, S, T, normalize, variant)
CASES = [(body, S, T, normalize, "") for body in BODIES for S in S_GRID for T in T_GRID for normalize in (True, False)]
CASES += [("p257", 3, 2, True, "g1last"), ("p449", 3, 2, True, "g1last"), ("p449", 3, 2, True, "r0big")]
_IN, _SIM = {}, {}


def case_id(body, S, T, normalize, variant):
    return f"{body}{'+' + variant if variant else ''}-S{S}T{T}-{'norm' if normalize else 'raw'}"


def inputs(body, S, T, variant=""):
    """-> (conf, mask, P, [x, v, prim, k, mu, actions], cotangents); the same arrays whenever it is asked again"""
    key = (body, S, T, variant)
    if key not in _IN:
        make, P, waves = BODIES[body]
        mask = make()
        assert int(mask.sum()) == P and -(-P // 64) == waves
        conf = cab.make_conf(substeps=S)
        rng = np.random.default_rng(zlib.crc32(f"ragged/{body}/S{S}/T{T}".encode()))
        x, v, prim, k, mu, actions = cab.make_case(rng, conf, mask, B, T)
        g = cab.cotangents(rng, B, T, P, lists=True)
        x[:, ::7, 1] = 0
        if variant == "g1last":
            for b in range(B):
                prim[b, 1, :3] = x[b, P - 1] + np.float32([0, 0.002, 0])
            r2 = np.random.default_rng(zlib.crc32(f"ragged/{body}/S{S}/T{T}/g1".encode()))
            actions[..., 4:7] = (r2.normal(size=(T, B, 3)) * 0.3).astype(np.float32)
            actions[..., 7] = r2.uniform(0.2, 0.8, size=(T, B)).astype(np.float32)
        elif variant == "r0big":
            # 1.1 above the particle it was drawn on: inside the input radius (1.25), and after the first substep has clipped the
            # primitive into the unit cube and its radius to 1, the later thresholds decide on their own
            prim[:, 0, 1] += np.float32(1.1)
            prim[:, 0, 3] = R0_BIG
        else:
            assert variant == ""
        _IN[key] = (conf, mask, P, [x, v, prim, k, mu, actions], g)
    return _IN[key]


def oracle_forward(body, S, T, variant=""):
    """the order-2 CPU oracle's forward of the case, with grasp sets (T, S, B, 2, P) and the input record of every substep"""
    conf, mask, P, case, _ = inputs(body, S, T, variant)
    return cab.make_oracle(conf, mask, 2).rollout_fwd(*case, want_lists=True, want_grasp=True, want_ckpt=True, nthreads=cab.NTHREADS)


def waves_held(grasp, gripper):
    """grasp (T, S, B, 2, P) -> bool [substeps, B, waves]: the gripper holds at least one particle of the wave"""
    g = np.asarray(grasp)
    g = g.reshape((-1,) + g.shape[2:])[:, :, gripper, :] != 0
    P = g.shape[-1]
    nw = -(-P // 64)
    pad = np.zeros(g.shape[:2] + (nw * 64,), bool)
    pad[..., :P] = g
    return pad.reshape(g.shape[:2] + (nw, 64)).any(-1)


def sim_of(body, S, **extra):
    key = (body, S, tuple(sorted(extra.items())))
    if key not in _SIM:
        from unidom_amd.engine.cloth_simulator import ClothSimulator
        make, P, _ = BODIES[body]
        sim = ClothSimulator(cab.make_conf(substeps=S, **extra), B, lambda x, v, i, j: v, make(), mode=0)
        assert sim.mode == 0 and sim.n_particles == P and sim.forward_order == 2 and not sim.several_workgroups
        _SIM[key] = sim
    return _SIM[key]


def run(body, S, T, normalize, variant):
    """the adjoint outputs (cab.KEYS) of the case on the GPU, float32"""
    from test_cloth_gpu import _run_hip
    _, _, _, case, g = inputs(body, S, T, variant)
    sim = sim_of(body, S)
    h = _run_hip(sim, *case, g=g, want_lists=True, normalize=normalize)
    sim.check_status()
    return {q: np.ascontiguousarray(h[q], np.float32) for q in cab.KEYS}
