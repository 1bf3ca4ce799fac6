"""The cases of tests/mpm_det_edge_cases.py on the CPU: every case reaches the edge it is named for (in the kernels' own integer arithmetic), the
mode's source built for the CPU follows the independent oracle's forward at the project's bars, and the adjoint reference of
tests/test_mpm_det_edges_gpu.py is sound -- finite, non-trivial on every compared leaf (or the leaf is listed as an exact zero), and its own f32
form within F32_BAR = 5e-4 of it on every key: what f32 alone costs at these shapes stays 10 x under the 5e-3 the kernels are held to.

Measured (worst over the cases): checker against oracle x 1.1e-7, v 4.6e-7, C 1.1e-6, F 1.2e-6; the oracle's f32 adjoint against its f64 adjoint
2.4e-4 (gx of past_upper; 9.3e-5 without that case, gx of n2)."""
import numpy as np
import pytest

import mpm_det_edge_cases as dc


def test_irregular_means_what_the_kernels_mean():
    """Irregular particles (bucket key -1) come from the upper edge of `res` alone.  The corner cases have none: their particles with
    x inv_dx < 0.5 truncate to base 0 (34 / 28 of them in `corner`, all 160 in `all_irregular`, by its y axis) and are bucketed like any other."""
    st = {tag: dc.stencil_stats(dc.case(tag)) for tag in dc.ALL_TAGS}
    n_irr = {tag: [s["n_irr"] for s in v] for tag, v in st.items()}
    assert n_irr["corner"] == [0, 0] and [s["low"] for s in st["corner"]] == [34, 28]
    assert n_irr["all_irregular"] == [0, 0] and [s["low"] for s in st["all_irregular"]] == [160, 160]
    assert n_irr["crowded"] == [0, 0] and n_irr["crowded_corner"] == [0, 0] and n_irr["bucket_boundary"] == [0, 0]
    # regular and irregular mixed, in both envs; every particle irregular (no bucket at all); a crowded bucket merged with irregular particles
    for tag in ("upper_edge", "four_boxes_upper_edge", "upper_corner", "crowded_upper"):
        assert all(0 < n < dc.case(tag).N for n in n_irr[tag]), (tag, n_irr[tag])
    assert n_irr["upper_edge"] == [82, 91] and n_irr["crowded_upper"] == [28, 34]
    for tag in ("all_irregular_upper", "past_upper"):
        assert n_irr[tag] == [160, 160] and all(s["max_bucket"] == 0 for s in st[tag]), tag
    # DET_K = 8 register slots: the tail loop, alone and merged; the boundary itself
    assert [s["max_bucket"] for s in st["crowded"]] == [18, 21] and [s["max_bucket"] for s in st["crowded_corner"]] == [70, 78]
    assert all(s["max_bucket"] > 2 * dc.DET_K for s in st["crowded_upper"])
    assert all(s["buckets"] == [dc.DET_K - 1, dc.DET_K, dc.DET_K + 1] for s in st["bucket_boundary"])
    # gather cells outside the scatter set: a clamped gather reads a cell nobody scatters to -- only where particles lie past res in a thin body
    assert [s["gather_only"] for s in st["past_upper"]] == [23, 26]
    assert all(s["gather_only"] == 0 for tag in dc.ALL_TAGS if tag != "past_upper" for s in st[tag])
    # several offsets of one clamped particle gather from the same cell (MODE 1 of the cell sums selects by cell_gather)
    assert all(s["offsets_per_cell"] == 27 for s in st["upper_corner"]) and all(s["offsets_per_cell"] == 3 for s in st["upper_edge"])
    # the backward's limit of listed cells, from both sides; an odd count; the largest body
    assert [s["touched"] for s in st["cells_32751"]] == [32751] and [s["touched"] for s in st["cells_32778"]] == [32778]
    assert 32751 <= dc.DET_SORT_CELLS < 32778
    assert all(s["touched"] == 27 for s in st["n1"] + st["n1_s1"])
    assert dc.case("n8192").N == dc.DET_MAX_PARTICLES and st["n8192"][0]["touched"] > dc.DET_SORT_CELLS
    assert [dc.case(t).N for t in dc.SMALL] == [1, 1, 2, 3, 64, 65] and dc.case("n1_s1").S == 1


@pytest.mark.parametrize("tag", dc.ALL_TAGS)
def test_case_is_built_as_stated(tag):
    c = dc.case(tag)
    assert c.B == (1 if tag in ("cells_32751", "cells_32778", "n8192") else 2)
    assert set(np.unique(c.material)) <= {1, 2} and c.hard.min() >= 0.5 and c.hard.max() <= 2.0
    if c.N >= 24:
        assert set(np.unique(c.material)) == {1, 2} and c.hard.max() - c.hard.min() > 0.5
    assert (c.st["x"] > 0).all() and (c.st["friction"] == np.float32(0.3)).all()
    rot = c.st["action"].reshape(c.B, c.P, 6)[..., 3:]
    assert (np.abs(rot).min() > 0) if tag in dc.TURNING else (rot == 0).all()
    assert ("gprot" in c.g) == (not c.pc) and c.P == (1 if c.pc else (2 if tag == "turning_boxes_crowded_corner" else 4))
    assert dc.case(tag) is c                                      # the same arrays whenever it is asked again
    for t2 in dc.REUSE:                                            # cases that share a handle share its particle tables
        assert np.array_equal(dc.case(t2).material, dc.case("corner").material) and np.array_equal(dc.case(t2).hard, dc.case("corner").hard)


@pytest.mark.parametrize("tag", dc.ALL_TAGS)
def test_same_order_source_follows_the_independent_oracle(tag):
    chk, ref = dc.checker(tag), dc.oracle_fwd(tag)
    for key, bar in dc.FWD_BARS.items():
        assert np.isfinite(chk[key]).all() and np.isfinite(ref[key]).all(), key
        print(tag, key, dc.rel(chk[key], ref[key]))
        assert dc.rel(chk[key], ref[key]) < bar, (tag, key, dc.rel(chk[key], ref[key]))


@pytest.mark.parametrize("tag", dc.BACKWARD_TAGS)
def test_adjoint_reference_is_finite_nontrivial_and_f32_stays_close(tag):
    c = dc.case(tag)
    ref, f32 = dc.oracle_bwd(tag), dc.oracle_bwd(tag, np.float32)
    assert sorted(dc.ZEROS) == sorted(dc.BACKWARD_TAGS)
    for key in dc.compared_keys(c):
        assert np.isfinite(ref[key]).all() and np.isfinite(f32[key]).all(), key
        live, zero = dc.split_zero(c, key, ref[key])
        if zero is not None:
            assert (zero == 0).all(), (tag, key)
            assert (dc.split_zero(c, key, f32[key])[1] == 0).all(), (tag, key)
        if live is not None:
            assert np.abs(live).max() > 0, (tag, key, "identically zero but not listed in ZEROS")
            got = dc.split_zero(c, key, f32[key])[0]
            print(tag, key, dc.rel(got, live))
            assert dc.rel(got, live) <= dc.F32_BAR, (tag, key, dc.rel(got, live))
