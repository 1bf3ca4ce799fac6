"""ctypes binding of libunidom_hip.so.  The structs, the prototypes and the symbol list are those _abi.py parses out of
include/unidom_hip.h; nothing of the header is re-stated here.

The HIP library IS the product path: there is no CPU or eager-PyTorch fallback. If the shared object is
missing or a call fails, an exception is raised (UnidomError) -- nothing silently routes elsewhere.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

from ._abi import DEFINES, PROTOTYPES, STRUCTS, UnidomError  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.environ.get("UNIDOM_HIP_SO", os.path.join(CSRC, "libunidom_hip.so"))   # override: diagnostic builds only

SYMBOLS = sorted(PROTOTYPES)                       # every function include/unidom_hip.h declares
RENDER_MAX_PRIM = DEFINES["UD_PLB_RENDER_MAX_PRIM"]
globals().update(STRUCTS)                          # ud_cloth_conf, ud_mpm_conf, ud_plb_conf, ud_*_render_conf, ud_plb_render_light


def build(force: bool = False) -> str:
    """Compile libunidom_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(os.path.dirname(_HERE), "include", "unidom_hip.h"))
    stale = (not os.path.exists(SO_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(SO_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-s", "-C", CSRC, "libunidom_hip.so"] + (["-B"] if force else []))
    return SO_PATH


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO_PATH):
            raise UnidomError(
                f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"(or `make -C {CSRC}`). There is no fallback path.")
        # torch first: its wheel carries its own libamdhip64 / libhsa-runtime64, the library links /opt/rocm's.  Loaded in this order the
        # library's HIP calls resolve to the runtime torch has already brought in (one runtime per process: device pointers and streams
        # are torch's); loaded the other way round the process holds two runtimes and the second one finds "no ROCm-capable device".
        import torch  # noqa: F401
        L = C.CDLL(SO_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            if not hasattr(L, name):
                raise UnidomError(f"{SO_PATH} does not export {name}")
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _LIB = L
    return _LIB


def check(rc: int, what: str):
    if rc != 0:
        raise UnidomError(f"{what} failed (status {rc}): {lib().ud_last_error().decode()}")


def ptr(t):
    """Device pointer of a contiguous float32/uint8 CUDA(HIP) tensor, or NULL."""
    if t is None:
        return C.c_void_p(0)
    assert t.is_cuda and t.is_contiguous(), "libunidom_hip takes contiguous device tensors"
    return C.c_void_p(t.data_ptr())


def stream(device):
    """The current stream of `device` as the void* the library's calls take."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
