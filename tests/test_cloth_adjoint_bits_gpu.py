"""GPU: the one-workgroup cloth adjoint (cloth_rollout_bwd_fast_kernel, csrc/cloth_fast_bwd.hip) gives the recorded bits.

tests/golden/cloth_adjoint_bits.npz holds every adjoint output (cab.KEYS) of the cases of tests/cloth_adjoint_bits_cases.py as
the raw f32 the kernel wrote before its roundings were written out in the source (tools/record_cloth_adjoint_bits.py, run
once against a build of that commit on an MI355X).  The kernel's multiply-adds are explicit (`__builtin_fmaf` under
`fp contract(off)`), so these bits depend neither on the vectoriser nor on any other choice the compiler makes per build:
`make -C unidom_amd/csrc -B build/cloth_fast_bwd.o BWDFLAGS=` builds the file with the SLP vectoriser on, and this test passes on
that library unchanged (UNIDOM_HIP_SO=...; run once, docs/HISTORY.md section 12)."""
import os

import numpy as np
import pytest

import cloth_adjoint_bar as cab
import cloth_adjoint_bits_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", cc.GOLDEN))


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: cc.case_id(*c))
def test_adjoint_outputs_are_the_recorded_bits(golden, case):
    h = cc.run(*case)
    bad = []
    for q in cab.KEYS:
        got, want = h[q].view(np.uint32), golden[f"{cc.case_id(*case)}/{q}"].view(np.uint32)
        assert got.shape == want.shape, (q, got.shape, want.shape)
        n = int((got != want).sum())
        if n:
            d = np.abs(h[q].astype(np.float64) - want.view(np.float32).astype(np.float64)).max()
            print(f"BITS {cc.case_id(*case)}/{q}: {n} of {got.size} words differ, max |diff| {d:.3e}")
            bad.append(q)
    for q in cab.KEYS:
        np.testing.assert_array_equal(h[q].view(np.uint32), golden[f"{cc.case_id(*case)}/{q}"].view(np.uint32), err_msg=f"{q} (differing tensors: {bad})")
