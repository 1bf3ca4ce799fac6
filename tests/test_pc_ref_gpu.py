"""GPU: the ud_pc_* kernels (csrc/pc_group.hip) against what the reference's own sampling / grouping kernels wrote for the cases of
tests/pc_ref_cases.py (the committed fixture tests/golden/pc_ref_cases.npz; tests/test_pc_ref_cpu.py holds the NumPy specification to
the same numbers and, where the reference can be built, the fixture to the reference).

The expectations are the CPU file's with the kernel in the specification's place: the reference's bits wherever the contract
promises them -- every cloud of at most 512 points, every cloud without exact ties (3100 points, past the reference's shared-memory
copy and on the product's several-points-per-lane path, among them), 33 clouds in one call, 512 samples of 200 points --, the
documented tie rule where it does not, rows of zeros where the reference wrote nothing.  Every call runs inside the guarded buffers
of tests/test_pc_group_gpu.py."""
import numpy as np
import pytest

from tests import pc_ref_cases as pc
from tests.test_pc_group_gpu import _same, hip_ball, hip_fps, hip_group_bwd, hip_group_fwd

pytestmark = pytest.mark.gpu

_PROMISED = [name for name in pc.fps_cases() if name not in pc.tie_cases()]


@pytest.mark.parametrize("name", _PROMISED)
def test_kernel_fps_is_the_reference_s(name):
    c = pc.load()[name]
    rc, gi, gn = hip_fps(c["xyz"], int(c["m"]))
    assert rc == 0 and _same(gi.numpy(), c["idx"]) and _same(gn.numpy(), c["new_xyz"])
    assert gi.intact() and gn.intact()


@pytest.mark.parametrize("name", pc.tie_cases())
def test_kernel_fps_parts_from_the_reference_only_by_the_documented_tie_rule(name):
    c = pc.load()[name]
    rc, gi, gn = hip_fps(c["xyz"], int(c["m"]))
    assert rc == 0 and gi.intact() and gn.intact()
    pc.check_tie_deviation(name, c["xyz"], gi.numpy(), gn.numpy(), c["idx"], c["new_xyz"])


@pytest.mark.parametrize("name", [f"ball_{n}_{ns}" for n, ns in pc.BALL] + [f"boundary_{k}" for k in pc.BOUNDARY_K])
def test_kernel_ball_query_is_the_reference_s_and_writes_zeros_where_it_wrote_nothing(name):
    c = pc.load()[name]
    rc, gi, gc = hip_ball(float(c["radius"]), int(c["nsample"]), c["xyz"], c["new_xyz"])
    assert rc == 0 and gi.intact() and gc.intact()
    pc.check_ball(gi.numpy(), gc.numpy(), c)


@pytest.mark.parametrize("C", pc.GROUP_C)
def test_kernel_group_forward_is_the_reference_s_gather_minus_the_centre(C):
    xyz, feats, new_xyz, idx, want = pc.group_expected(C)
    rc, out = hip_group_fwd(xyz, feats, new_xyz, idx)
    assert rc == 0 and _same(out.numpy(), want) and out.intact()


@pytest.mark.parametrize("name", list(pc.BWD))
def test_kernel_group_backward_is_the_reference_s_on_dyadic_cotangents(name):
    c = pc.load()[name]
    n, got = int(c["n"]), []
    for centre_idx in (None, c["centre_idx"]):
        rc, gx, gf, gn = hip_group_bwd(n, c["idx"], c["g_out"], centre_idx)
        assert rc == 0 and gx.intact() and gf.intact() and gn.intact()
        got.append((gx.numpy(), gf.numpy(), gn.numpy()))
    pc.check_group_bwd(c, *got)


def test_kernel_model_index_chain_is_the_reference_s():
    """512 of 200, ball 0.02 / 32, 128 of those 512, ball 0.02 / 64: each stage fed with the kernel's own output of the stage before."""
    c = pc.load()["chain"]
    rc, c1, x1 = hip_fps(c["xyz"], 512)
    assert rc == 0 and _same(c1.numpy(), c["idx"]) and _same(x1.numpy(), c["new_xyz"])
    rc, i1, n1 = hip_ball(0.02, 32, c["xyz"], x1.numpy())
    assert rc == 0 and _same(i1.numpy(), c["i1"]) and _same(n1.numpy(), c["cnt1"])
    rc, c2, x2 = hip_fps(x1.numpy(), 128)
    assert rc == 0 and _same(c2.numpy(), c["c2"]) and _same(x2.numpy(), c["x2"])
    rc, i2, n2 = hip_ball(0.02, 64, x1.numpy(), x2.numpy())
    assert rc == 0 and _same(i2.numpy(), c["i2"]) and _same(n2.numpy(), c["cnt2"])
