"""MpmRenderer -- what the MLS-MPM envs show, on the device (ParticlePyRenderer and WaterPyRenderer of
daxbench/core/engine/pyrender/py_render.py:120-174, the primitives of envs/basic/mpm_env.py:200-236): one sphere or one point per
particle, the primitives the particles collide with and the ground, seen by the reference's camera, many frames per call, in
libunidom_hip.so (csrc/mpm_render.hip; the contract is the ud_mpm_render_* block of include/unidom_hip.h, the specification
tests/mpm_render_twin.py).

Camera, projection, the sphere radius, the particle grey, the water colour and the returned orientation (RGB, not mirrored) are the
reference's.  Deviations, none pinned by reference data (nothing of pyrender's was ever rendered for comparison): a particle is an
analytic sphere, not a uv_sphere mesh; only the nearest point of a pixel blends; a primitive is drawn where the simulator collides with
it (the inverse transform of inv_trans_batch), not through the reference's Euler-angle detour; the cut hollow sphere is sphere-traced on
its SDF, not drawn from a marching-cubes mesh; a particle nearer than the near plane is dropped whole; the shading and the primitive and
ground colours are this project's own (flat Lambert under the reference's three lights); the ground is one flat colour.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from .cloth_render import ClothRenderConf

SPHERES, POINTS = 0, 1
BOX, CONTAINER = 0, 1


class MpmRenderConf(ClothRenderConf):
    """BasicPyRenderer's scene (the cloth renderer's: cam_pose is None in every MPM env) and how the particles are drawn."""
    particle_color = (0.5, 0.5, 0.5, 1.0)         # py_render.py:130 vertex colour; WATER_COLOR is :157's (100, 100, 249, 125) / 255
    prim_color = (0.35, 0.3, 0.05)                # this project's own
    mode = SPHERES                                # :128 uv_sphere per particle; POINTS: :157 Mesh.from_points
    radius = 0.008                                # :128
    point_size = 1                                # pyrender's default point size, pixels

    WATER_COLOR = (100 / 255, 100 / 255, 249 / 255, 125 / 255)

    def __init__(self, **overrides):
        for k, v in overrides.items():
            if not hasattr(type(self), k):
                raise AttributeError(f"MpmRenderConf has no field {k!r}")
            setattr(self, k, v)


class MpmRenderer:
    """frames(x, prim_pos, prim_rot) -> (color u8 [..., H, W, 3] RGB, depth f32 [..., H, W][, id i32 [..., H, W]]) on the device, for any
    leading shape; more than max_frames frames are rendered in chunks of max_frames.  prim_sizes [n_prims, 3]: half sizes (box) or
    (r, h, t) (cut hollow sphere), fixed for the handle."""

    def __init__(self, n_particles, prim_sizes, prim_kind, conf=None, max_frames=64, device="cuda"):
        rc = MpmRenderConf() if conf is None else conf
        self.conf, self.device, self.max_frames = rc, torch.device(device), int(max_frames)
        self.n_particles, self.prim_kind = int(n_particles), int(prim_kind)
        sizes = np.ascontiguousarray(np.asarray(prim_sizes, np.float32).reshape(-1, 3))
        self.prim_sizes, self.n_prims = sizes, int(sizes.shape[0])
        d3, d2 = (lambda v: (C.c_double * 3)(*map(float, v))), (lambda v: (C.c_double * 2)(*map(float, v)))
        f3, f4 = (lambda v: (C.c_float * 3)(*map(float, v))), (lambda v: (C.c_float * 4)(*map(float, v)))
        cc = _lib.ud_mpm_render_conf(
            width=int(rc.width), height=int(rc.height), yfov=float(rc.yfov), znear=float(rc.znear), camera_pos=d3(rc.camera_pos),
            camera_target=d3(rc.camera_target), camera_up=d3(rc.camera_up), ground_min=d2(rc.ground_min), ground_max=d2(rc.ground_max),
            ground_z=float(rc.ground_z), particle_color=f4(rc.particle_color), prim_color=f3(rc.prim_color), ground_color=f3(rc.ground_color),
            mode=int(rc.mode), radius=float(rc.radius), point_size=int(rc.point_size), n_particles=self.n_particles, n_prims=self.n_prims,
            prim_kind=self.prim_kind, max_frames=self.max_frames)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ud_mpm_render_create(C.byref(cc), sizes.ctypes.data_as(C.c_void_p) if self.n_prims else C.c_void_p(0),
                                                       C.byref(self._h)), "ud_mpm_render_create")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.lib().ud_mpm_render_destroy(self._h)
        except Exception:
            pass

    def frames(self, x, prim_pos=None, prim_rot=None, want_id=False):
        """x [..., N, 3] (sim order), prim_pos [..., n_prims, 3], prim_rot [..., n_prims, 4] (w, x, y, z); None when n_prims = 0."""
        N, NP, H, W = self.n_particles, self.n_prims, int(self.conf.height), int(self.conf.width)
        x = x.detach().to(device=self.device, dtype=torch.float32)
        if x.shape[-2:] != (N, 3):
            raise ValueError(f"MpmRenderer.frames: x {tuple(x.shape)} does not end in ({N}, 3)")
        lead = tuple(x.shape[:-2])
        x = x.reshape(-1, N, 3).contiguous()
        M = x.shape[0]
        pp = pr = None
        if NP > 0:
            pp = prim_pos.detach().to(device=self.device, dtype=torch.float32).reshape(M, NP, 3).contiguous()
            pr = prim_rot.detach().to(device=self.device, dtype=torch.float32).reshape(M, NP, 4).contiguous()
        color = torch.empty((M, H, W, 3), dtype=torch.uint8, device=self.device)
        depth = torch.empty((M, H, W), dtype=torch.float32, device=self.device)
        ids = torch.empty((M, H, W), dtype=torch.int32, device=self.device) if want_id else None
        stream = _lib.stream(self.device)
        L = _lib.lib()
        with torch.cuda.device(self.device):
            for m0 in range(0, M, self.max_frames):
                m1 = min(M, m0 + self.max_frames)
                _lib.check(L.ud_mpm_render_frames(self._h, m1 - m0, _lib.ptr(x[m0:m1]), _lib.ptr(pp[m0:m1] if NP else None),
                                                  _lib.ptr(pr[m0:m1] if NP else None), _lib.ptr(color[m0:m1]), _lib.ptr(depth[m0:m1]),
                                                  _lib.ptr(ids[m0:m1] if want_id else None), stream), "ud_mpm_render_frames")
        out = (color.reshape(lead + (H, W, 3)), depth.reshape(lead + (H, W)))
        return out + (ids.reshape(lead + (H, W)),) if want_id else out
