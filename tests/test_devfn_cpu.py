"""The product's hand-written device math, function by function, in its HOST builds -- the product's own source through a host compiler:
  * svd3 (unidom_amd/csrc/mpm_device.h) and ud_expf (mpm_collide.h) of the UD_HOST_BUILD compilation, the deterministic mode's
    arithmetic (oracle/csrc/mpm_det_host.cpp: oc_dev_svd3_f32, oc_dev_expf);
  * dsvd3 (plb_svd.h) with IEEE stand-ins for its three hardware seeds (oracle/csrc/plb_svd_host.cpp: oc_dev_dsvd3_f64).
Inputs, assertions and where the 16 eps bar comes from: tests/devfn_cases.py.  The same cases run on the GPU in tests/test_devfn_gpu.py.

These tests are what stands between the SVDs' early exit and the suite: with the exit taken after a sweep whose normalised column
products were below 1e-4 (f32) / 3e-9 (f64) -- the thresholds before this file existed -- they fail, e.g.
    svd3/host / nearrot eps=0.0003: max|UtU - I| = 589.2 eps > 16.0      dsvd3/host / nearrot eps=1e-07: max|UtU - I| = 2132.3 eps > 16.0
(the first family that misses; the families are run in the order of devfn_cases.families)
and pass with the exit at round-off level (1e-13 / 1e-30 on the squared products; svd3 also rotates on that threshold only).  Recorded worst residuals of that source, in eps:
    DEVFN svd3/host: uu 3.2  vv 8.3  rec 5.9  s 3.8  polar 3.3  (worst, in eps)
    DEVFN dsvd3/host: uu 5.1  vv 6.1  rec 5.1  (worst, in eps)
(uu = max|UtU - I|, vv = max|Vh Vht - I|, rec = max|U S Vh - A| / S0, s = max|S - S_lapack| / S0, polar = max|U Vh - polar(A)|)
"""
import numpy as np

import devfn_cases as dc


def test_svd3_host_build_factors_hold_16_eps_on_every_family(capsys):
    from oracle.pyoracle import dev_svd3_f32
    worst = dc.check_all_families("svd3/host", dev_svd3_f32, np.float32)
    with capsys.disabled():
        print("\n" + dc.devfn_line("svd3/host", worst))


def test_dsvd3_host_build_factors_hold_16_eps_on_every_family(capsys):
    from oracle.pyoracle import dev_dsvd3_f64
    worst = dc.check_all_families("dsvd3/host", dev_dsvd3_f64, np.float64)
    with capsys.disabled():
        print("\n" + dc.devfn_line("dsvd3/host", worst))


def test_expf_host_build_is_within_2_ulp_on_the_range_that_reaches_it():
    """mpm_collide.h: "within 2 ulp of expf on the range that reaches it" -- the argument is -dist * softness <= 0.  Against f64 exp rounded
    to f32, on [-87, 0]; outside: +inf from 88.7 up, 0 below -87, NaN stays NaN.  Measured: 1 ulp at the most
    (with the polynomial at degree 6, as it was before this test: 3 ulp, at x = -80.75)."""
    from oracle.pyoracle import dev_expf
    x = dc.expf_points()
    y = dev_expf(x)
    neg = (x >= np.float32(-87.0)) & (x <= 0)
    want = np.exp(x[neg].astype(np.float64)).astype(np.float32)
    ulps = np.abs(y[neg].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulps.max() <= 2, (ulps.max(), x[neg][ulps.argmax()])
    assert (want >= np.finfo(np.float32).tiny).all()          # nothing on this range is below the normal range
    assert np.isnan(y[np.isnan(x)]).all() and (y[x >= np.float32(88.7)] == np.inf).all() and (y[x < np.float32(-87.0)] == 0).all()
    pos = (x > 0) & (x < np.float32(88.7))
    rel = np.abs(y[pos].astype(np.float64) / np.exp(x[pos].astype(np.float64)) - 1)
    assert rel.max() < 4 * np.finfo(np.float32).eps, rel.max()
