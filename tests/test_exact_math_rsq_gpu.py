"""exact_math.h's select-free 1 / sqrt (rcp_sqrt_rn_rsq2x4 and its scalar form rcp_sqrt_rn_rsq), walked over EVERY f32 bit pattern of
the ranges it is used on, on the device (tests/devfn/exact_math_rsq.hip in tests/devfn/libdevfn.so; a missing library FAILS these tests):

  * [1e-12f, FLT_MAX], about 1.4e9 arguments -- the clipped link lengths of force_v2: the pair form and the scalar form against
    rcp_sqrt_rn_inrange2x4, the function they replace, which tests/test_devfn_gpu.py holds to NumPy's correctly rounded sqrt and /;
  * [2^-96, 1e-12f), +inf and NaNs -- what isV can see besides: the scalar form against 1.0f / sqrtf(x) compiled in the same object.

The bar is 0 mismatching bit patterns (any NaN equals any NaN).  The kernel counts on the device and returns the counts and the lowest
offending pattern.  The guard that admits a launch's constants to the isV use is a host function and is tested without a GPU."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devfn", "libdevfn.so")


@functools.lru_cache(maxsize=None)
def _lib():
    assert os.path.exists(SO), f"{SO} is missing: __graft_entry__.build() (make -C unidom_amd/csrc devfn) builds it"
    import torch  # noqa: F401  -- torch first, so that the library's HIP calls resolve to the runtime torch brought in (unidom_amd/_lib.py)
    return C.CDLL(SO)


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _sweep(ranges, against_compiler):
    """-> (mismatches of the pair form, mismatches of the scalar form, lowest offending pattern or None) over the inclusive pattern ranges"""
    import torch
    res = torch.tensor([0, 0, -1], dtype=torch.int64, device="cuda")   # -1 = ~0 as uint64
    fn = _lib().devfn_rcp_sqrt_rsq_sweep
    fn.restype = C.c_int
    for lo, hi in ranges:
        rc = fn(C.c_uint(lo), C.c_uint(hi), C.c_int(int(against_compiler)), C.c_void_p(res.data_ptr()))
        assert rc == 0, f"devfn_rcp_sqrt_rsq_sweep: hipError {rc}"
    torch.cuda.synchronize()
    bad2, bad1, first = (int(v) for v in res.cpu().numpy().view(np.uint64))
    return bad2, bad1, (None if first == 2 ** 64 - 1 else first)


@pytest.mark.gpu
def test_every_link_length_argument_gives_the_shipped_bits():
    lo, hi = _bits(1e-12), _bits(np.finfo(np.float32).max)
    assert hi - lo + 1 > 1_400_000_000
    bad2, bad1, first = _sweep([(lo, hi)], against_compiler=False)
    print(f"{hi - lo + 1} patterns: pair form {bad2} mismatches, scalar form {bad1}, first {first if first is None else hex(first)}")
    assert (bad2, bad1, first) == (0, 0, None)


@pytest.mark.gpu
def test_scalar_form_is_the_compilers_rcp_sqrt_below_the_clip_and_at_inf_and_nan():
    ranges = [(_bits(2.0 ** -96), _bits(1e-12) - 1),        # below force_v2's clip, down to the guard's floor for small_num
              (0x7F800000, 0x7F800000),                      # +inf -> 0
              (0x7F800001, 0x7F800040), (0x7FBFFFC0, 0x7FC00040), (0x7FFFFFC0, 0x7FFFFFFF)]   # NaNs, signalling and quiet
    _, bad1, first = _sweep(ranges, against_compiler=True)
    print(f"{sum(h - l + 1 for l, h in ranges)} patterns: scalar form {bad1} mismatches, first {first if first is None else hex(first)}")
    assert (bad1, first) == (0, None)


def test_isv_guard_admits_only_constants_that_keep_the_argument_in_range():
    """cloth_isv_consts_ok: small_num finite and >= 2^-96, max_v not NaN and 2 max_v^2 + small_num <= FLT_MAX.  Host code: no GPU."""
    ok = _lib().devfn_cloth_isv_consts_ok
    ok.restype = C.c_int
    f = lambda eps, max_v: ok(C.c_float(eps), C.c_float(max_v))
    fmax = float(np.finfo(np.float32).max)
    assert f(1e-8, 10.0) == 1                                  # the shipped environments' constants
    assert f(2.0 ** -96, 0.0) == 1 and f(float(np.nextafter(np.float32(2.0 ** -96), np.float32(0))), 10.0) == 0
    assert f(0.0, 10.0) == 0 and f(-1e-8, 10.0) == 0
    assert f(float("inf"), 10.0) == 0 and f(float("nan"), 10.0) == 0
    assert f(1e-8, float("nan")) == 0 and f(1e-8, float("inf")) == 0
    assert f(1e-8, 1.3e19) == 1 and f(1e-8, 1.31e19) == 0      # sqrt(FLT_MAX / 2) = 1.3043e19
    assert f(fmax, 0.0) == 1 and f(fmax, 1e19) == 0
    assert f(1e-8, -10.0) == 1                                 # clipf(v, 10, -10) still bounds |v| by 10
