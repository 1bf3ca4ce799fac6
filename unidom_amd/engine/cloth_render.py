"""ClothRenderer -- MeshPyRenderer.render of the cloth envs on the device (daxbench/core/engine/pyrender/py_render.py:16-117): the cloth's
triangle mesh, the gripper and the ground seen by the reference's camera, many frames per call, in libunidom_hip.so
(csrc/cloth_render.hip; the contract is the ud_cloth_render_* block of include/unidom_hip.h, the specification tests/cloth_render_twin.py).

Camera, projection, coverage, depth and the returned orientation (mirrored left-right, BGR) are the reference's.  Not pinned by reference
data: the shading is this project's own (flat Lambert under the reference's three lights, not pyrender's PBR shader), the ground is one
flat colour (the wood texture is not shipped), the gripper is an analytic sphere (not an icosphere with random face colours) and a
triangle with a vertex nearer than znear is dropped whole (not clipped).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from .. import _lib


class ClothRenderConf:
    """BasicPyRenderer's scene (py_render.py:17-47); positions in the render frame (z up: sim (x, y, z) is render (x, z, y))."""
    width, height = 640, 480              # :17 screen_size
    yfov = math.pi / 3.0                  # :37
    znear = 0.05                          # pyrender's PerspectiveCamera default; no far plane
    camera_pos = (0.9, 0.5, 1.0)          # :39 (also the pose of the directional and the spot light)
    camera_target = (0.6, 0.5, 0.0)
    camera_up = (0.0, 0.0, 1.0)           # :50
    ground_min = (-0.02, -0.04)           # :24-28: wood.obj scaled to 1 x 1, moved to (0.48, 0.46, -0.02)
    ground_max = (0.98, 0.96)
    ground_z = -0.02
    cloth_color = (0.12, 0.2, 0.35)       # base colours (RGB), this project's own
    ground_color = (0.3, 0.2, 0.12)
    sphere_color = (0.35, 0.05, 0.05)

    def __init__(self, **overrides):
        for k, v in overrides.items():
            if not hasattr(type(self), k):
                raise AttributeError(f"ClothRenderConf has no field {k!r}")
            setattr(self, k, v)


class ClothRenderer:
    """frames(x_grid, primitive0) -> (color u8 [..., H, W, 3], depth f32 [..., H, W][, tri i32 [..., H, W]]) on the device, for any leading
    shape; more than max_frames frames are rendered in chunks of max_frames.  `sim`: a ClothSimulator (its N and indices)."""

    def __init__(self, sim, conf=None, max_frames=64, n_spheres=1):
        rc = ClothRenderConf() if conf is None else conf
        self.conf, self.device, self.max_frames, self.n_spheres = rc, sim.device, int(max_frames), int(n_spheres)
        self.n_vertices = int(sim.N) * int(sim.N)
        faces = np.ascontiguousarray(np.asarray(sim.indices).reshape(-1, 3).astype(np.int32))   # the reference keeps them as f32
        self.n_faces = int(faces.shape[0])
        d3, d2, f3 = (lambda v: (C.c_double * 3)(*map(float, v))), (lambda v: (C.c_double * 2)(*map(float, v))), (lambda v: (C.c_float * 3)(*map(float, v)))
        cc = _lib.ud_cloth_render_conf(
            width=int(rc.width), height=int(rc.height), yfov=float(rc.yfov), znear=float(rc.znear), camera_pos=d3(rc.camera_pos),
            camera_target=d3(rc.camera_target), camera_up=d3(rc.camera_up), ground_min=d2(rc.ground_min), ground_max=d2(rc.ground_max),
            ground_z=float(rc.ground_z), cloth_color=f3(rc.cloth_color), ground_color=f3(rc.ground_color), sphere_color=f3(rc.sphere_color),
            n_vertices=self.n_vertices, n_faces=self.n_faces, n_spheres=self.n_spheres, max_frames=self.max_frames)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ud_cloth_render_create(C.byref(cc), faces.ctypes.data_as(C.c_void_p), C.byref(self._h)), "ud_cloth_render_create")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.lib().ud_cloth_render_destroy(self._h)
        except Exception:
            pass

    def frames(self, x_grid, primitive0, want_tri=False):
        """x_grid [..., N, N, 3] or [..., N*N, 3] (sim order, get_x_grid's), primitive0 [..., 4] (centre in sim order, radius)."""
        V, S, H, W = self.n_vertices, self.n_spheres, int(self.conf.height), int(self.conf.width)
        x = x_grid.detach().to(torch.float32)
        lead = tuple(x.shape[:-3]) if x.shape[-2] != V else tuple(x.shape[:-2])
        x = x.reshape(-1, V, 3).contiguous()
        M = x.shape[0]
        sp = None
        if S > 0:
            sp = primitive0.detach().to(torch.float32).reshape(M, S, 4).contiguous()
        color = torch.empty((M, H, W, 3), dtype=torch.uint8, device=self.device)
        depth = torch.empty((M, H, W), dtype=torch.float32, device=self.device)
        tri = torch.empty((M, H, W), dtype=torch.int32, device=self.device) if want_tri else None
        stream = _lib.stream(self.device)
        L = _lib.lib()
        for m0 in range(0, M, self.max_frames):
            m1 = min(M, m0 + self.max_frames)
            _lib.check(L.ud_cloth_render_frames(self._h, m1 - m0, _lib.ptr(x[m0:m1]), _lib.ptr(sp[m0:m1] if S > 0 else None),
                                                _lib.ptr(color[m0:m1]), _lib.ptr(depth[m0:m1]), _lib.ptr(tri[m0:m1] if want_tri else None),
                                                stream), "ud_cloth_render_frames")
        out = (color.reshape(lead + (H, W, 3)), depth.reshape(lead + (H, W)))
        return out + (tri.reshape(lead + (H, W)),) if want_tri else out
