"""The cases of tests/plb_edge_cases.py on the CPU, through the twin alone: every case reaches the edge it is named for, no compared gradient is
trivially zero (or the case names it as a structural zero), no input sits on a tie of a clamp, and the reference itself is well-conditioned --
the twin run again with the particles in another order (another summation order on the grid) agrees within 1e-8 relative in max-norm on every
leaf, two orders below the 1e-6 the kernels are held to in tests/test_plb_edges_gpu.py, so a miss there is not conditioning."""
import numpy as np
import pytest

import plb_edge_cases as pc

COND = 1e-8


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-300)


@pytest.mark.parametrize("tag", pc.STEP_TAGS)
def test_step_case_is_tie_free_nontrivial_and_well_conditioned(tag):
    case = pc.step_case(tag)
    x, v, Cm, F, prim, soft, act, E, nu, ys = case.inputs
    assert x.shape == (case.B, case.N, 3) and act.shape == (case.B, 3) and len(set(ys[:2])) == 2
    # no tie: |raw action| != 1, pos + pv never ON a bound, no particle starts ON a position clamp
    conf = pc.twin_conf(case)
    pos, un = pc.trajectory(case)
    assert (np.abs(act) != 1.0).all()
    assert (un != np.array(conf.upper_bound)).all() and (un != np.array(conf.lower_bound)).all()
    assert (x > 0).all() and (x < pc.X_MAX).all()
    outs, grads = pc.twin_step(case)
    sel = slice(None) if case.pick is None else list(case.pick)
    np.testing.assert_array_equal(outs[4], pos[sel, -1])
    assert all(np.isfinite(o).all() for o in outs) and all(np.isfinite(g).all() for g in grads.values())
    # the body is on the floor and sphere 0 in it
    for name in pc.LEAVES:
        top = np.abs(grads[name]).max()
        assert (top == 0.0) == (name in case.zero + case.cancel), (name, top)
    if "ys" not in case.zero:
        assert np.abs(grads["ys"][1]) > 0                                  # env 1 went through the return mapping
    # conditioning of the reference, prim_pos: along an axis the bound clamp never stops, the start position's gradient is the cotangent of the
    # final position and nothing else -- autograd forms it as (w + G) - G with G the sticky contact's sums, so it shows how large those are
    if case.w[4] is not None:
        free = ((un >= np.array(conf.lower_bound)) & (un <= np.array(conf.upper_bound))).all(1)[sel]      # [B, 2, 3]
        w4 = case.w[4][sel]
        assert free[:, 1].all() and np.abs((grads["prim"] - w4)[free]).max() < COND * np.abs(w4).max()
    # ... and everything: another particle order
    perm = np.random.default_rng(case.N).permutation(case.N)
    outs2, grads2 = pc.twin_step(case, perm=perm)
    worst = max([_rel(b, a) for a, b in zip(outs, outs2)] + [_rel(grads2[k], grads[k]) for k in pc.LEAVES if k not in case.zero + case.cancel])
    print(f"PLBEDGE-TWIN {tag}: order sensitivity {worst:.1e}")
    assert worst < COND, worst
    for k in case.zero + case.cancel:
        assert np.abs(grads2[k]).max() == 0.0
    assert not case.cancel or pc.CANCEL_BAR(case, grads) > 0


def test_clip_case_clips_and_the_primitive_travels():
    case = pc.step_case("clip")
    act = case.inputs[6]
    pos, un = pc.trajectory(case)
    np.testing.assert_array_equal(pos[:, 1:], un)                            # the bounds are never active: the primitive is free
    assert abs(pos[0, -1, 0, 0] - pos[0, 0, 0, 0] - 1.0) < 1e-15 and abs(pos[1, -1, 0, 2] - pos[1, 0, 0, 2] + 1.0) < 1e-15
    g = pc.twin_step(case)[1]["act"]
    clipped = np.abs(act) > 1
    assert clipped.sum() == 2 and clipped[0, 0] and clipped[1, 2]
    assert (g[clipped] == 0.0).all() and (np.abs(g[~clipped]) > 0).all()
    # the GPU test holds g_action env by env here (the unclipped env's is 100 times the others'): so is the twin's own sensitivity to the order
    g2 = pc.twin_step(case, perm=np.random.default_rng(1).permutation(case.N))[1]["act"]
    assert max(_rel(g2[b], g[b]) for b in range(case.B)) < COND


def test_bound_case_keeps_the_primitive_on_its_bound_in_every_substep():
    case = pc.step_case("bound")
    hi = case.conf_kw["upper_bound"][0]
    pos, un = pc.trajectory(case)
    assert (pos[:, :, 0, 0] == hi).all() and (un[:, :, 0, 0] > hi).all()     # starts on it, pushed strictly beyond it, stays on it
    assert (np.abs(case.inputs[6]) < 1).all()                                # not through the action clip
    x = case.inputs[0]
    assert (x[..., 0] < hi).any() and (x[..., 0] > hi).any()                 # the bound lies inside the body
    _, g = pc.twin_step(case)
    assert (g["act"][:, 0] == 0.0).all() and (np.abs(g["act"][:, 1:]) > 0).all()
    # pinned, the sphere hands its cells (hi - pos) / dt: the start position is read by substep 0's contact and by nothing else
    assert (np.abs(g["prim"][:, 0, 0]) > 1e3 * np.abs(case.w[4][:, 0, 0])).all()


def test_xclamp_case_ends_on_the_position_clamp_and_its_cotangent_passes_through_g2p_alone():
    case = pc.step_case("xclamp")
    p = pc.XCLAMP_P
    outs, grads = pc.twin_step(case)
    assert (pc.X_MAX - case.inputs[0][:, p, 0] < 1e-5).all() and (pc.X_MAX - case.inputs[0][:, p, 0] > 0).all()
    assert (outs[0][:, p, 0] == pc.X_MAX).all()                              # bit for bit
    assert (outs[0] == pc.X_MAX).sum() == case.B and (outs[0] == 0.0).sum() == 0   # and nobody else on a clamp
    assert (outs[1][:, p, 0] > 0.1).all()                                    # still moving outward: the last substep clamped too
    # the clamped output has no sensitivity at all: its cotangent changes no gradient
    w = [wi.copy() for wi in case.w]
    w[0][:, p, 0] += 10.0
    _, g2 = pc.twin_step(case, w=w)
    for k in pc.LEAVES:
        np.testing.assert_array_equal(g2[k], grads[k])
    # while the cotangent of its y does
    w[0][:, p, 1] += 10.0
    _, g3 = pc.twin_step(case, w=w)
    assert np.abs(g3["x"][:, p] - grads["x"][:, p]).max() > 1e-3


def test_part_and_launch_shapes_are_the_ones_named():
    parts = lambda N: (-(-N // 32), N - 32 * (-(-N // 32) - 1))               # (parts, particles in the last)
    assert [parts(N) for N in pc.PART_SIZES] == [(1, 1), (1, 5), (1, 32), (2, 1), (2, 5), (2, 32)]
    assert parts(1000) == (32, 8) and parts(1024) == (32, 32) and parts(1025) == (33, 1)
    assert sorted(pc.step_case(t).S % 3 for t in pc.RING_TAGS) == [0, 1, 1, 2] and [pc.step_case(t).S for t in pc.SMAX_TAGS] == [128, 129]
    big = pc.step_case(pc.LAUNCH_TAG)
    assert big.B == 19 and set(big.pick) == {0, 7, 8, 15, 16, 18}
    for a in big.inputs[:5] + big.inputs[6:]:                                # every env has its own inputs
        assert len({a[b].tobytes() for b in range(big.B)}) == big.B


@pytest.mark.parametrize("tag", pc.LOSS_TAGS)
def test_loss_case_reaches_its_edge_and_is_well_conditioned(tag):
    case = pc.loss_case(tag)
    d = pc.contact_distances(case)                                           # [3, 2, N]
    assert case.x.shape == (3, case.N, 3) and pc.LOSS_GL[1] == 0.0
    inside = np.zeros(d.shape, bool)
    for b, p, pi in case.inside:
        inside[b, pi, p] = True
    np.testing.assert_array_equal(d == 0.0, inside)                          # exactly the named particles are inside a sphere
    if not case.soft:                                                        # a unique positive minimum, or a minimum of 0
        srt = np.sort(d, -1)
        assert ((srt[..., 0] == 0.0) | (case.N == 1) | (srt[..., min(1, case.N - 1)] - srt[..., 0] > 1e-6)).all()
        assert ((srt[..., 0] == 0.0) == inside.any(-1)).all()
    total, parts, gx, gp = pc.twin_loss(case)
    assert np.isfinite(total).all() and np.isfinite(gx).all() and np.isfinite(gp).all()
    assert np.abs(gx[0]).max() > 0 and np.abs(gx[2]).max() > 0 and (gx[1] == 0.0).all() and (gp[1] == 0.0).all()   # g_loss[1] = 0
    assert (np.abs(gp).max() == 0.0) == ("prim" in case.zero)
    if tag == "insideboth_hard":
        assert (parts[:, 0] == 0.0).all()
    if tag == "inside0_hard":
        assert (gp[[0, 2], 0] == 0.0).all() and (np.abs(gp[[0, 2], 1]).max(-1) > 0).all()
    if tag == "inside0_soft":                                                # the particle inside passes nothing from the contact of sphere 0 ...
        assert (np.abs(gp[[0, 2], 0]).max(-1) > 0).all() and (parts[:, 0] > 0).all()   # ... the others do
    perm = np.random.default_rng(case.N).permutation(case.N)
    total2, parts2, gx2, gp2 = pc.twin_loss(case, perm)
    worst = max(_rel(total2, total), _rel(parts2, parts), _rel(gx2, gx), 0.0 if "prim" in case.zero else _rel(gp2, gp))
    assert worst < COND, worst
