"""ctypes binding of oracle/_ref/libref_pc.so: the reference's point-cloud sampling / grouping kernels run on the CPU by
oracle/ref_pc/driver.cpp (test infrastructure; built by `make -C oracle ref_pc` where the reference tree is present).

Every function takes and returns NumPy arrays in the reference's layouts.  Output buffers are pre-filled with a sentinel where the
reference does not write every element (ball query), and with zeros where it adds into them (the two gradients)."""
import ctypes
import os

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "_ref")
SENT_I = -77777                # what ball_query leaves in the rows the reference never writes

_f = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_i = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_c = ctypes.c_int


def path(fma=False):
    return os.path.join(_DIR, "libref_pc_fma.so" if fma else "libref_pc.so")


def available(fma=False):
    if fma:
        try:
            with open("/proc/cpuinfo") as fh:
                if " fma " not in fh.read():
                    return False
        except OSError:
            return False
    return os.path.exists(path(fma))


class RefPc:
    def __init__(self, fma=False):
        L = self.L = ctypes.CDLL(path(fma))
        for name, args in [("ref_pc_fps", [_c, _c, _c, _f, _f, _i]), ("ref_pc_gather", [_c, _c, _c, _f, _i, _f]),
                           ("ref_pc_scatter_add", [_c, _c, _c, _f, _i, _f]),
                           ("ref_pc_ball_query", [_c, _c, _c, ctypes.c_float, _c, _f, _f, _i, _i]),
                           ("ref_pc_group", [_c, _c, _c, _c, _c, _f, _i, _f]), ("ref_pc_group_grad", [_c, _c, _c, _c, _c, _f, _i, _f])]:
            getattr(L, name).argtypes, getattr(L, name).restype = args, None

    def fps(self, xyz, m):
        """xyz [B,n,3] -> idx [B,m] int32."""
        xyz = np.ascontiguousarray(xyz, np.float32)
        B, n, _ = xyz.shape
        idx, temp = np.full((B, m), SENT_I, np.int32), np.zeros(32 * n, np.float32)
        self.L.ref_pc_fps(B, n, m, xyz, temp, idx)
        return idx

    def gather(self, xyz, idx):
        """xyz [B,n,3], idx [B,m] -> [B,m,3]."""
        xyz, idx = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(idx, np.int32)
        B, n, _ = xyz.shape
        out = np.full((B, idx.shape[1], 3), np.float32(12345.678), np.float32)
        self.L.ref_pc_gather(B, n, idx.shape[1], xyz, idx, out)
        return out

    def scatter_add(self, n, idx, g):
        """g [B,m,3] added at idx [B,m] into zeros [B,n,3]."""
        g, idx = np.ascontiguousarray(g, np.float32), np.ascontiguousarray(idx, np.int32)
        B, m = idx.shape
        out = np.zeros((B, n, 3), np.float32)
        self.L.ref_pc_scatter_add(B, n, m, g, idx, out)
        return out

    def ball_query(self, radius, nsample, xyz, new_xyz):
        """-> (idx [B,m,nsample], cnt [B,m]); rows without a hit keep SENT_I."""
        xyz, new_xyz = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(new_xyz, np.float32)
        B, n, _ = xyz.shape
        m = new_xyz.shape[1]
        idx, cnt = np.full((B, m, nsample), SENT_I, np.int32), np.full((B, m), SENT_I, np.int32)
        self.L.ref_pc_ball_query(B, n, m, float(radius), nsample, xyz, new_xyz, idx, cnt)
        return idx, cnt

    def group(self, points, idx):
        """points [B,n,C], idx [B,m,nsample] -> [B,m,nsample,C]."""
        points, idx = np.ascontiguousarray(points, np.float32), np.ascontiguousarray(idx, np.int32)
        B, n, C = points.shape
        _, m, ns = idx.shape
        out = np.full((B, m, ns, C), np.float32(12345.678), np.float32)
        self.L.ref_pc_group(B, n, C, m, ns, points, idx, out)
        return out

    def group_grad(self, n, idx, g):
        """g [B,m,nsample,C] added at idx into zeros [B,n,C]."""
        g, idx = np.ascontiguousarray(g, np.float32), np.ascontiguousarray(idx, np.int32)
        B, m, ns, C = g.shape
        out = np.zeros((B, n, C), np.float32)
        self.L.ref_pc_group_grad(B, n, C, m, ns, g, idx, out)
        return out
