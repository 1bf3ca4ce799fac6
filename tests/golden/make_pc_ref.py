#!/usr/bin/env python3
"""Write tests/golden/pc_ref_cases.npz: the inputs of tests/pc_ref_cases.py and what the reference's own point-cloud sampling /
grouping kernels write for them.

Test infrastructure only.  Needs oracle/_ref/libref_pc.so (`make -C oracle ref_pc`, which needs the reference tree; the build
calls it).  The file holds arrays only: seeded inputs made here and the numbers the reference's program wrote.  Nothing is written
when a case has lost what makes it discriminating (pc_ref_cases.check_discriminating) or when the file would pass 512 KB.

    python tests/golden/make_pc_ref.py
"""
import io
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from oracle import ref_pc  # noqa: E402
from tests import pc_ref_cases as pc  # noqa: E402

LIMIT = 512 * 1024


def main():
    cases = pc.build_inputs()
    ref = pc.run_reference(ref_pc.RefPc(), cases)
    pc.check_discriminating(cases, ref)
    buf = io.BytesIO()
    np.savez_compressed(buf, **pc.flatten(cases, ref))
    size = buf.getbuffer().nbytes
    assert size <= LIMIT, f"{size} bytes: over {LIMIT}"
    with open(pc.FIXTURE, "wb") as fh:
        fh.write(buf.getvalue())
    print(f"wrote {pc.FIXTURE}: {size} bytes, {len(cases)} cases")


if __name__ == "__main__":
    main()
