"""PlbRenderer -- TaichiEnv.render() of the PLB path on the device (GenORM/policy/pbm/plb/engine/renderer/renderer.py): the particle SDF bake,
the first-hit G-buffer and the path-traced image for B envs per call, in libunidom_hip.so (csrc/plb_render.hip; the contract is the
ud_plb_render_* block of include/unidom_hip.h, the specification tests/plb_render_twin.py).

The directional light (on in envs/torus.yml, off in the defaults and in the other task files) and Russian roulette (off everywhere) are state of the
handle: PlbRenderer sets them from the RenderConf after create (set_light; the specification is tests/plb_render_light_twin.py).  Not covered: the
`target` overlay (commented out in the reference).  The random draws are this project's own hash (ti.random cannot be pinned).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib


class RenderConf:
    """cfg.RENDERER of plb/config/default_config.py:41-59."""
    spp = 50                              # :42
    max_ray_depth = 2                     # :43, :50
    image_res = (512, 512)                # :44
    voxel_res = (168, 168, 168)           # :45
    dx = 1.0 / 150                        # :48
    sdf_threshold = 0.65 * 0.56           # :49
    bake_size = 6                         # :51
    use_roulette = False                  # :52, :58
    light_direction = (2.0, 1.0, 0.7)     # :54 (read by the directional light only)
    camera_pos = (0.5, 1.2, 4.0)          # :55
    camera_rot = (0.2, 0.0)               # :56
    use_directional_light = False         # :57

    def __init__(self, **overrides):
        for k, v in overrides.items():
            if not hasattr(type(self), k):
                raise AttributeError(f"RenderConf has no field {k!r}")
            setattr(self, k, v)


def render_conf_of(sim_conf, **overrides):
    """RenderConf() under the env file's RENDERER block (sim_conf.render_overrides), then `overrides`."""
    kw = dict(getattr(sim_conf, "render_overrides", {}) or {})
    kw.update(overrides)
    return RenderConf(**kw)


class PlbRenderer:
    """bake(state, color) -> (bbox [B,2,3], status [B]); gbuffer(state) -> dict; render(state) -> image.  `state`: a PlbState, or anything with
    x [B,N,3], prim_pos [B,P,3] and optionally prim_rot [B,P,4] / prim_gap [B,P].  A state without prim_rot (no rot_state) is drawn with the
    conf's constant orientation, sim_conf.prim_rot."""

    def __init__(self, sim_conf, render_conf=None, batch_size=1, device="cuda"):
        rc = render_conf_of(sim_conf) if render_conf is None else render_conf
        self.sim_conf, self.conf, self.batch_size, self.device = sim_conf, rc, int(batch_size), torch.device(device)
        self.n_particles = int(sim_conf.n_particles)
        self.n_primitive = P = len(sim_conf.prim_radius)
        if P > _lib.RENDER_MAX_PRIM:
            raise ValueError(f"the renderer takes at most {_lib.RENDER_MAX_PRIM} primitives")
        M = _lib.RENDER_MAX_PRIM
        pad = lambda seq, fill: (list(seq)[:P] + [fill] * M)[:M]
        # primitive cfg colour: every task file of the reference sets (0.7, 0.7, 0.7) or leaves the default (0.3, 0.3, 0.3) (primive_base.py)
        colors = pad(getattr(sim_conf, "prim_color", ()), (0.3, 0.3, 0.3))
        # particle colour, one i32 0xRRGGBB for the whole body: Shapes.add_box's `color`, else COLORS[0] of shape_maker.py:4-9
        self.color = torch.full((self.n_particles,), int(getattr(sim_conf, "particle_color", (127 << 16) + 127)) & 0xFFFFFF, dtype=torch.int32,
                                device=self.device)
        cc = _lib.ud_plb_render_conf(
            dx=float(rc.dx), voxel_res=(C.c_int * 3)(*rc.voxel_res), bake_size=int(rc.bake_size), sdf_threshold=float(rc.sdf_threshold),
            image_res=(C.c_int * 2)(*rc.image_res), spp=int(rc.spp), max_ray_depth=int(rc.max_ray_depth),
            camera_pos=(C.c_double * 3)(*rc.camera_pos), camera_rot=(C.c_double * 2)(*rc.camera_rot),
            use_directional_light=0, use_roulette=0, n_primitives=P,      # lighting is handle state: set_light below
            prim_kind=(C.c_int * M)(*pad(getattr(sim_conf, "prim_kind", ()), 0)), prim_radius=(C.c_double * M)(*pad(sim_conf.prim_radius, 0.0)),
            prim_h=(C.c_double * M)(*pad(getattr(sim_conf, "prim_h", ()), 0.0)),
            prim_shape=(C.c_double * 3 * M)(*[(C.c_double * 3)(*(list(s) + [0.0] * 3)[:3]) for s in pad(getattr(sim_conf, "prim_shape", ()), (0.0, 0.0, 0.0))]),
            prim_color=(C.c_float * 3 * M)(*[(C.c_float * 3)(*c) for c in colors]),
            n_particles=self.n_particles, max_envs=self.batch_size)
        # the constant orientation of a handle without rot_state (PlbConf.prim_rot; identity where the conf gives none)
        rots = (list(getattr(sim_conf, "prim_rot", ())) + [(1.0, 0.0, 0.0, 0.0)] * P)[:P]
        self._conf_rot = torch.tensor([tuple(map(float, q)) for q in rots], dtype=torch.float64, device=self.device).reshape(P, 4)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().ud_plb_render_create(C.byref(cc), C.byref(self._h)), "ud_plb_render_create")
        self.set_light(rc.use_directional_light, rc.use_roulette, rc.light_direction)

    def set_light(self, use_directional_light, use_roulette=False, light_direction=None):
        """ud_plb_render_set_light: which instance of the image kernel the next image() runs (host only).  light_direction None = the conf's."""
        d = self.conf.light_direction if light_direction is None else light_direction
        ll = _lib.ud_plb_render_light(use_directional_light=int(bool(use_directional_light)), use_roulette=int(bool(use_roulette)),
                                      light_direction=(C.c_double * 3)(*map(float, d)))
        _lib.check(_lib.lib().ud_plb_render_set_light(self._h, C.byref(ll)), "ud_plb_render_set_light")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.lib().ud_plb_render_destroy(self._h)
        except Exception:
            pass

    def bake(self, state, color=None):
        """set_particles: bake the envs' particle SDF volumes into the handle.  color: [N] int32 0xRRGGBB (None = the conf's).  Returns
        (bbox [B,2,3] f32, status [B] i32) without synchronising; status 1 = the cloud does not fit voxel_res (render() raises)."""
        x = state.x.detach().to(torch.float64).contiguous()
        B = x.shape[0]
        assert tuple(x.shape[1:]) == (self.n_particles, 3), tuple(x.shape)
        col = self.color
        if color is not None:                  # 24 bits: anything above them would reach the distance bits of the packed minimum
            col = torch.bitwise_and(torch.as_tensor(color, device=self.device).to(torch.int64), 0xFFFFFF).to(torch.int32).contiguous()
        assert col.numel() == self.n_particles
        bbox = torch.empty((B, 2, 3), dtype=torch.float32, device=self.device)
        status = torch.empty((B,), dtype=torch.int32, device=self.device)
        _lib.check(_lib.lib().ud_plb_render_bake(self._h, B, *[_lib.ptr(t) for t in (x, col, bbox, status)], _lib.stream(self.device)),
                   "ud_plb_render_bake")
        return bbox, status

    def volume(self, B):
        """The packed volume [B,rx,ry,rz] (int64) and the smoothed sdf (float32) of the last bake."""
        r = tuple(self.conf.voxel_res)
        vol = torch.empty((B,) + r, dtype=torch.int64, device=self.device)
        sdf = torch.empty((B,) + r, dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().ud_plb_render_read_volume(self._h, B, _lib.ptr(vol), _lib.ptr(sdf), _lib.stream(self.device)), "ud_plb_render_read_volume")
        return vol, sdf

    def _prims(self, state):
        if self.n_primitive == 0:
            return None, None, None
        f = lambda t: None if t is None else t.detach().to(torch.float64).contiguous()
        rot = getattr(state, "prim_rot", None)
        if rot is None:                        # no rot_state: the orientation is the conf's constant, the one the simulator handle was made with
            rot = self._conf_rot[None].expand(state.prim_pos.shape[0], -1, -1)
        return f(state.prim_pos), f(rot), f(getattr(state, "prim_gap", None))

    def gbuffer(self, state):
        """The deterministic first hit of the last bake, one ray per pixel centre: dict(kind [B,W,H] i32, t, normal [..,3], albedo [..,3]),
        indexed (env, u, v) as the reference's color_buffer."""
        B = state.x.shape[0]
        W, H = self.conf.image_res
        pp, pr, pg = self._prims(state)
        kind = torch.empty((B, W, H), dtype=torch.int32, device=self.device)
        t = torch.empty((B, W, H), dtype=torch.float32, device=self.device)
        normal = torch.empty((B, W, H, 3), dtype=torch.float32, device=self.device)
        albedo = torch.empty((B, W, H, 3), dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().ud_plb_render_gbuffer(self._h, B, *[_lib.ptr(a) for a in (pp, pr, pg, kind, t, normal, albedo)],
                                                    _lib.stream(self.device)), "ud_plb_render_gbuffer")
        return dict(kind=kind, t=t, normal=normal, albedo=albedo)

    def image(self, state, spp=None, seed=0):
        """The f32 image [B,H,W,3] of the last bake (no bake, no status check)."""
        B = state.x.shape[0]
        W, H = self.conf.image_res
        pp, pr, pg = self._prims(state)
        img = torch.empty((B, H, W, 3), dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().ud_plb_render_image(self._h, B, _lib.ptr(pp), _lib.ptr(pr), _lib.ptr(pg), int(self.conf.spp if spp is None else spp),
                                                  int(seed) & 0xFFFFFFFF, _lib.ptr(img), _lib.stream(self.device)), "ud_plb_render_image")
        return img

    def render(self, state, spp=None, seed=0, mode="rgb_array", color=None, strict=True):
        """TaichiEnv.render (taichi_env.py:88-94): bake + image.  mode "rgb_array": uint8 [B,H,W,3] = uint8(img.clip(0, 1) * 255); "float": the
        f32 image.  strict: raise where a cloud does not fit the volume (the reference's assert); otherwise such an env's image is zeros."""
        if mode not in ("rgb_array", "float"):
            raise ValueError(f"mode {mode!r}: 'rgb_array' or 'float'")
        bbox, status = self.bake(state, color)
        img = self.image(state, spp, seed)
        if strict and bool(status.any()):
            bad = status.nonzero().reshape(-1).tolist()
            raise _lib.UnidomError(f"render: the particles of env(s) {bad} do not fit voxel_res {tuple(self.conf.voxel_res)} at dx {self.conf.dx} "
                                   f"(bbox {bbox[bad[0]].tolist()})")
        if mode == "float":
            return img
        return (img.clamp(0.0, 1.0) * 255.0).to(torch.uint8)
