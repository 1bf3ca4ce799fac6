"""GPU: the decision words behind the cloth checkpoint (csrc/cloth_common.h, cloth_decisions_kernel of csrc/cloth_fast_bwd.hip).

Decisions: the forward through ClothSimulator with gradients on, in every mode whose forward can precede the one-workgroup fast adjoint
(0: v2, 2: fast, 3: reference order); every word behind the records equals, exactly, the NumPy float32 restatement
(tests/cloth_decisions_cases.py) applied to THAT checkpoint's own records and the actions -- so the comparison does not depend on which
forward wrote them.  Bodies of 1, 63, 65, 257, 449 and 512 particles, T in {1, 2}, S in {1, 2, 3}, B = 2, inputs that reach every code
(tests/test_cloth_decisions_cases.py asserts that on the CPU oracle), and the input-radius-above-one variant.

Threshold: ud_cloth_ckpt_bytes is records plus words up to MAX_B envs and the records formula above; a 63-particle body at MAX_B and at
MAX_B + 1 envs (the adjoint that reads the words / the one that re-derives the decisions) gives, for envs 0-1, gradients bit-equal to a
B = 2 call on the same inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import cloth_adjoint_bar as cab
import cloth_decisions_cases as dc

pytestmark = pytest.mark.gpu

MAX_B = 32     # UD_CLOTH_DEC_MAX_B of csrc/cloth_common.h
MODES = (0, 2, 3)


def _sim(body, S, mode, B=dc.B):
    from unidom_amd.engine.cloth_simulator import ClothSimulator
    conf, mask, P, _ = dc.inputs(body, S, 1)
    sim = ClothSimulator(conf, B, lambda x, v, i, j: v, mask, mode=mode)
    assert sim.mode == mode and sim.n_particles == P and not sim.several_workgroups
    return sim


def _bytes(sim, B, T):
    from unidom_amd import _lib
    return int(_lib.lib().ud_cloth_ckpt_bytes(sim._h, C.c_int(B), C.c_int(T)))


def _decisions(body, S, T, mode, variant=""):
    from unidom_amd.engine.cloth_simulator import _Rollout
    conf, mask, P, case = dc.inputs(body, S, T, variant)
    B, Pp = dc.B, -(-P // 64) * 64
    sim = _sim(body, S, mode)
    out = _Rollout.apply(sim, *(torch.tensor(a, device=sim.device, requires_grad=True) for a in case), False)
    ckpt = out[0].grad_fn.saved_tensors[0]
    sim.check_status()
    rec, n = 6 * Pp + 8, T * S
    floats = B * (n + 1) * rec
    assert ckpt.numel() == floats + B * n * Pp and 4 * ckpt.numel() == _bytes(sim, B, T)
    r = ckpt[:floats].cpu().numpy().reshape(B, n + 1, rec)
    planes = r[..., :6 * Pp].reshape(B, n + 1, 6, Pp)[..., :P]
    x = np.moveaxis(planes[:, :n, :3], 2, -1)
    v_next = np.moveaxis(planes[:, 1:, 3:], 2, -1)
    prim = r[:, :n, 6 * Pp:].reshape(B, n, 2, 4)
    got = ckpt[floats:].view(torch.int32).cpu().numpy().view(np.uint32).reshape(B, n, Pp)
    want = dc.decision_words(x, v_next, prim, case[5], S, Pp, conf.max_v)
    bad = np.argwhere(got != want)
    if len(bad):
        b, m, i = bad[0]
        print(f"WORDS {body} S{S} T{T} mode {mode}: {len(bad)} of {got.size} differ; first at env {b} record {m} lane {i}: "
              f"got {got[b, m, i]:#010x} want {want[b, m, i]:#010x}")
    assert not len(bad)
    f = dc.fields(got)
    assert f["m0"].any() and (f["dx"] <= 2).all() and (f["prim"] <= 2).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", dc.T_GRID)
@pytest.mark.parametrize("S", dc.S_GRID)
@pytest.mark.parametrize("body", dc.BODY_NAMES)
def test_words_equal_the_restatement_on_the_checkpoints_own_records(body, S, T, mode):
    _decisions(body, S, T, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("body", ("rect7x9", "p449"))
def test_words_with_an_input_radius_above_one(body, mode):
    _decisions(body, 3, 2, mode, "r0big")


# -- the threshold on B ----------------------------------------------------------------------------------------------------------
_BODY, _S, _T = "rect7x9", 3, 2
_G = {}


def _grads(B):
    """the adjoint outputs of B envs, env e = env e % 2 of the B = 2 case (inputs and cotangents)"""
    if B not in _G:
        from test_cloth_gpu import _run_hip
        conf, mask, P, case = dc.inputs(_BODY, _S, _T)
        g = cab.cotangents(np.random.default_rng(12), dc.B, _T, P, lists=True)
        env = np.arange(B) % dc.B
        tile = lambda a, axis: np.ascontiguousarray(np.take(a, env, axis=axis))
        x, v, prim, k, mu, actions = case
        big = [tile(x, 0), tile(v, 0), tile(prim, 0), tile(k, 0), tile(mu, 0), tile(actions, 1)]
        gb = {q: tile(a, 1 if q.endswith("_list") else 0) for q, a in g.items()}
        sim = _sim(_BODY, _S, 0, B)
        h = _run_hip(sim, *big, g=gb, want_lists=True, normalize=True)
        sim.check_status()
        _G[B] = {q: np.ascontiguousarray(h[q], np.float32) for q in cab.KEYS}
    return _G[B]


@pytest.mark.parametrize("B", (MAX_B, MAX_B + 1))
def test_envs_0_and_1_at_the_threshold_and_above_equal_a_two_env_call(B):
    small, big = _grads(dc.B), _grads(B)
    for q in cab.KEYS:
        part = big[q][:, :dc.B] if q == "gactions" else big[q][:dc.B]
        np.testing.assert_array_equal(part.view(np.uint32), small[q].view(np.uint32), err_msg=q)
    assert np.abs(small["gx"]).max() > 0 and np.abs(small["gactions"]).max() > 0


def test_checkpoint_size_grows_by_the_words_up_to_the_threshold_only():
    P = dc.inputs(_BODY, _S, _T)[2]
    Pp, n = -(-P // 64) * 64, _T * _S
    records = lambda B: 4 * B * (n + 1) * (6 * Pp + 8)
    sim = _sim(_BODY, _S, 0, MAX_B + 1)
    for B in (1, 2, MAX_B):
        assert _bytes(sim, B, _T) == records(B) + 4 * B * n * Pp
    assert _bytes(sim, MAX_B + 1, _T) == records(MAX_B + 1)
    literal = _sim(_BODY, _S, 1, 2)                    # mode 1: the literal adjoint reads no words
    assert _bytes(literal, 2, _T) == records(2)
