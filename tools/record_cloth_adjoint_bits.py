"""Record the bits of the one-workgroup cloth adjoint: every adjoint output (cab.KEYS) of the cases of
tests/cloth_adjoint_bits_cases.py, run through ClothSimulator / _Rollout on the GPU, as raw f32, into
tests/golden/cloth_adjoint_bits.npz (tests/test_cloth_adjoint_bits_gpu.py compares the uint32 views word for word).

Run it against a build of the commit whose bits are the reference (UNIDOM_HIP_SO=/path/to/that/libunidom_hip.so), never to make a
failing test pass.
usage: python tools/record_cloth_adjoint_bits.py [--cases MODULE] [--out FILE]
  --cases: the module under tests/ that lists the cases (CASES, GOLDEN, case_id, run); default cloth_adjoint_bits_cases, or
           cloth_bwd_unroll_cases for tests/golden/cloth_bwd_unroll_bits.npz (tests/test_cloth_bwd_unroll_bits_gpu.py)"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cloth_adjoint_bar as cab                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="cloth_adjoint_bits_cases")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cc = importlib.import_module(args.cases)
    args.out = args.out or os.path.join(ROOT, "tests", "golden", cc.GOLDEN)
    from unidom_amd import _lib
    out = {}
    for case in cc.CASES:
        h = cc.run(*case)
        for q in cab.KEYS:
            assert np.isfinite(h[q]).all(), (case, q)
            out[f"{cc.case_id(*case)}/{q}"] = h[q]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"{len(cc.CASES)} cases, {len(out)} arrays, {os.path.getsize(args.out)} bytes -> {args.out} (library {_lib.SO_PATH})")


if __name__ == "__main__":
    main()
