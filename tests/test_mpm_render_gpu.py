"""GPU: the MPM renderer (csrc/mpm_render.hip behind ud_mpm_render_*, engine/mpm_render.py, MPMEnv.render / render_batch /
step_with_render) against its specification tests/mpm_render_twin.py: id, depth bits and colour equal in every pixel -- the arithmetic
has no unpinned function, so no pixel is exempt, and the twin has no bounding window, so equality also shows that the kernel's culling
window is conservative.  What the twin itself is held to: tests/test_mpm_render_cpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mpm_render_twin as twin
from mpm_render_cases import KERNEL_SIZES, kernel_scene, single_particle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Handle:
    """a bare ud_mpm_render handle (the kernel-level tests go below MpmRenderer)"""

    def __init__(self, conf, n_particles, sizes, max_frames, null_sizes=False):
        from unidom_amd import _lib
        self.lib, self.conf = _lib, conf
        d3, d2 = (lambda v: (C.c_double * 3)(*v)), (lambda v: (C.c_double * 2)(*v))
        f3, f4 = (lambda v: (C.c_float * 3)(*v)), (lambda v: (C.c_float * 4)(*v))
        self.sizes = np.ascontiguousarray(np.asarray(sizes, np.float32).reshape(-1, 3))
        self.cc = _lib.ud_mpm_render_conf(
            width=conf.width, height=conf.height, yfov=conf.yfov, znear=conf.znear, camera_pos=d3(conf.camera_pos),
            camera_target=d3(conf.camera_target), camera_up=d3(conf.camera_up), ground_min=d2(conf.ground_min), ground_max=d2(conf.ground_max),
            ground_z=conf.ground_z, particle_color=f4(conf.particle_color), prim_color=f3(conf.prim_color), ground_color=f3(conf.ground_color),
            mode=conf.mode, radius=conf.radius, point_size=conf.point_size, n_particles=n_particles, n_prims=len(self.sizes),
            prim_kind=conf.prim_kind, max_frames=max_frames)
        self.h = C.c_void_p()
        sp = C.c_void_p(0) if (null_sizes or not len(self.sizes)) else self.sizes.ctypes.data_as(C.c_void_p)
        self.rc = _lib.lib().ud_mpm_render_create(C.byref(self.cc), sp, C.byref(self.h))

    def __del__(self):
        if self.h:
            self.lib.lib().ud_mpm_render_destroy(self.h)

    def outputs(self, M, fill=None):
        H, W = self.conf.height, self.conf.width
        mk = (lambda s, dt: torch.empty(s, dtype=dt, device=DEV)) if fill is None else (lambda s, dt: torch.full(s, fill, dtype=dt, device=DEV))
        return mk((M, H, W, 3), torch.uint8), mk((M, H, W), torch.float32), mk((M, H, W), torch.int32)

    def call(self, M, x, pos, rot, color, depth, ids, handle=True):
        p = lambda t: C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())
        rc = self.lib.lib().ud_mpm_render_frames(self.h if handle else C.c_void_p(0), M, p(x), p(pos), p(rot), p(color), p(depth), p(ids),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc


@functools.lru_cache(maxsize=None)
def _scene(size, kind, mode, point_size):
    conf, x, pp, pr, sz = kernel_scene(size[0], size[1], kind, mode, point_size)
    want = [twin.render(conf, x[m], pp[m], pr[m], sz) for m in range(3)]
    return conf, x, pp, pr, sz, want


def _dev(a):
    return torch.tensor(a, device=DEV).contiguous()


def _same(color, depth, ids, want):
    if ids is not None:
        np.testing.assert_array_equal(ids.cpu().numpy(), want[2])
    np.testing.assert_array_equal(depth.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    np.testing.assert_array_equal(color.cpu().numpy(), want[0])


@pytest.mark.parametrize("size", KERNEL_SIZES)
@pytest.mark.parametrize("kind", [0, 1], ids=["boxes", "containers"])
# point sizes 4 and 5: either side of the threshold between the tile kernel's lane-per-particle and lane-per-pixel paths
@pytest.mark.parametrize("mode,point_size", [(0, 1), (1, 1), (1, 3), (1, 4), (1, 5)], ids=["spheres", "points1", "points3", "points4", "points5"])
def test_kernels_equal_the_twin_in_every_pixel(size, kind, mode, point_size):
    conf, x, pp, pr, sz, want = _scene(size, kind, mode, point_size)
    h = _Handle(conf, x.shape[1], sz, 3)
    assert h.rc == 0
    xd, pd, rd = _dev(x), _dev(pp), _dev(pr)
    color, depth, ids = h.outputs(3)
    assert h.call(3, xd, pd, rd, color, depth, ids) == 0
    for m in range(3):
        _same(color[m], depth[m], ids[m], want[m])
    # a second call: identical bits; id may be NULL
    c2, d2, i2 = h.outputs(3)
    assert h.call(3, xd, pd, rd, c2, d2, i2) == 0
    assert torch.equal(c2, color) and torch.equal(d2.view(torch.int32), depth.view(torch.int32)) and torch.equal(i2, ids)
    c3, d3, _ = h.outputs(3)
    assert h.call(3, xd, pd, rd, c3, d3, None) == 0
    assert torch.equal(c3, color) and torch.equal(d3.view(torch.int32), depth.view(torch.int32))
    # M = 1 is frame 0 of M = 3
    c1, d1, i1 = h.outputs(1)
    assert h.call(1, xd[:1].contiguous(), pd[:1].contiguous(), rd[:1].contiguous(), c1, d1, i1) == 0
    assert torch.equal(c1[0], color[0]) and torch.equal(d1[0].view(torch.int32), depth[0].view(torch.int32)) and torch.equal(i1[0], ids[0])


@pytest.mark.parametrize("mode", [0, 1])
def test_one_particle_and_no_primitive(mode):
    conf, x = single_particle(37, 29, mode)
    want = twin.render(conf, x[0])
    assert set(np.unique(want[2]).tolist()) == {-3, -1, 0}
    h = _Handle(conf, 1, np.zeros((0, 3), np.float32), 2)
    assert h.rc == 0
    color, depth, ids = h.outputs(1)
    assert h.call(1, _dev(x), None, None, color, depth, ids) == 0
    _same(color[0], depth[0], ids[0], want)


def test_invalid_arguments_touch_nothing():
    from unidom_amd import _lib
    conf, x, pp, pr, sz, _ = _scene((37, 29), 0, 0, 1)
    N = x.shape[1]
    h = _Handle(conf, N, sz, 3)
    assert h.rc == 0
    xd, pd, rd = _dev(x), _dev(pp), _dev(pr)
    bx, bp, br = _dev(np.concatenate([x, x[:1]])), _dev(np.concatenate([pp, pp[:1]])), _dev(np.concatenate([pr, pr[:1]]))
    color, depth, ids = h.outputs(4, fill=7)

    def untouched():
        return bool((color == 7).all()) and bool((depth == 7).all()) and bool((ids == 7).all())

    for rc in (h.call(0, xd, pd, rd, color, depth, ids), h.call(4, bx, bp, br, color, depth, ids), h.call(3, None, pd, rd, color, depth, ids),
               h.call(3, xd, None, rd, color, depth, ids), h.call(3, xd, pd, None, color, depth, ids), h.call(3, xd, pd, rd, None, depth, ids),
               h.call(3, xd, pd, rd, color, None, ids), h.call(3, xd, pd, rd, color, depth, ids, handle=False)):
        assert rc == -1                                         # UD_ERR_INVALID
        assert untouched()
    assert b"ud_mpm_render_frames" in _lib.lib().ud_last_error()
    # create: UD_ERR_INVALID
    C_ = twin.Conf
    assert _lib.lib().ud_mpm_render_create(C.c_void_p(0), h.sizes.ctypes.data_as(C.c_void_p), C.byref(C.c_void_p())) == -1
    assert _Handle(conf, N, sz, 3, null_sizes=True).rc == -1
    for bad in (C_(width=0, height=29), C_(width=37, height=0), C_(width=37, height=29, yfov=0.0), C_(width=37, height=29, yfov=3.2),
                C_(width=37, height=29, znear=0.0), C_(width=37, height=29, camera_target=C_.camera_pos),
                C_(width=37, height=29, camera_pos=(0.6, 0.5, 1.0)), C_(width=37, height=29, mode=2), C_(width=37, height=29, mode=-1),
                C_(width=37, height=29, prim_kind=2), C_(width=37, height=29, radius=0.0), C_(width=37, height=29, mode=1, point_size=0)):
        assert _Handle(bad, N, sz, 3).rc == -1, vars(bad)
    assert _Handle(conf, 0, sz, 3).rc == -1 and _Handle(conf, N, sz, 0).rc == -1
    assert _Handle(C_(width=37, height=29, mode=1, radius=0.0), N, sz, 3).rc == 0          # the radius is not used in point mode
    # create: UD_ERR_UNSUPPORTED
    assert _Handle(C_(width=5000, height=29), N, sz, 3).rc == -2
    assert _Handle(C_(width=37, height=4097), N, sz, 3).rc == -2
    assert _Handle(conf, (1 << 20) + 1, sz, 1).rc == -2
    assert _Handle(conf, N, np.zeros((17, 3), np.float32), 3).rc == -2
    assert _Handle(conf, 1 << 20, sz, 2048).rc == -2                                       # the arena would reach 2^31 elements


def test_supported_edge_sizes_create():
    """16 primitives, a 1024 x 1024 image, 2^17 particles in 4 frames: inside the supported range (create only)"""
    assert _Handle(twin.Conf(width=1024, height=1024), 1 << 17, np.full((16, 3), 0.01, np.float32), 4).rc == 0
    assert _Handle(twin.Conf(width=4096, height=1), 1, np.zeros((0, 3), np.float32), 1).rc == 0


# ---- env level ------------------------------------------------------------------------------------------------------------------------
SMALL = dict(width=160, height=120)


def _conf_with_render(conf_cls, **kw):
    conf = conf_cls()
    conf.render_conf = dict(SMALL, **kw)
    return conf


def _twin_of(env, state, b=None, t=None):
    """the twin's frame of env b of a state (or of entry t, env b of a state list)"""
    pick = (lambda a: a[b]) if t is None else (lambda a: a[t, b])
    x = pick(state.x).cpu().numpy()
    pos = np.stack([pick(p.position)[0].cpu().numpy() for p in state.primitives])
    rot = np.stack([pick(p.rotation)[0].cpu().numpy() for p in state.primitives])
    sizes = np.stack([p.size.reshape(-1, 3)[0].cpu().numpy() for p in state.primitives])
    rc = env._render_conf()
    tc = twin.Conf(width=rc.width, height=rc.height, mode=rc.mode, radius=rc.radius, point_size=rc.point_size, particle_color=rc.particle_color,
                   prim_color=rc.prim_color, ground_color=rc.ground_color, prim_kind=1 if env.simulator.sdf_kind == "container" else 0)
    return twin.render(tc, x, pos, rot, sizes)


def test_whip_rope_render_and_render_batch():
    from unidom_amd.envs.whip_rope_env import DefaultConf, WhipRopeEnv
    env = WhipRopeEnv(batch_size=2, seed=1, conf=_conf_with_render(DefaultConf))
    _, state = env.reset(np.array([0, 7], np.uint32))
    assert getattr(env, "_mpm_renderer", None) is None               # nothing is allocated before the first render call
    color, depth = env.render(state)
    assert isinstance(color, np.ndarray) and color.shape == (120, 160, 3) and color.dtype == np.uint8
    assert isinstance(depth, np.ndarray) and depth.shape == (120, 160) and depth.dtype == np.float32
    r = env._mpm_renderer
    assert r.conf.mode == 0 and r.conf.radius == 0.008 and r.prim_kind == 0 and r.n_prims == len(state.primitives)
    want = _twin_of(env, state, 0)
    assert (want[2] >= 0).sum() > 20 and (want[2] <= -4).sum() > 5 and (want[2] == -3).sum() > 1000 and (want[2] == -1).sum() > 100
    np.testing.assert_array_equal(depth.view(np.uint32), want[1].view(np.uint32))
    np.testing.assert_array_equal(color, want[0])
    # a moved batch: each env equals its own twin
    shift = torch.tensor([[0.0, 0.0, 0.0], [0.06, 0.03, -0.04]], device=state.x.device)
    moved = state._replace(x=state.x + shift[:, None, :])
    cb, db, ib = env.render_batch(moved, want_id=True)
    assert cb.shape == (2, 120, 160, 3) and cb.dtype == torch.uint8 and db.shape == (2, 120, 160) and db.dtype == torch.float32
    assert ib.shape == (2, 120, 160) and ib.dtype == torch.int32
    for b in range(2):
        _same(cb[b], db[b], ib[b], _twin_of(env, moved, b))
    assert not torch.equal(cb[0], cb[1])
    assert env._mpm_renderer is r                                    # the same handle
    with pytest.raises(NotImplementedError):
        env.get_obs(state, obs_type="RGB")
    with pytest.raises(NotImplementedError):
        env.get_obs(state, obs_type="DEPTH")


def test_shape_rope_step_with_render_is_step_diff_plus_frames():
    from unidom_amd.envs.shape_rope_env import DefaultConf, ShapeRopeEnv
    env = ShapeRopeEnv(batch_size=2, seed=1, conf=_conf_with_render(DefaultConf))
    _, state = env.reset(np.array([0, 7], np.uint32))
    actions = torch.tensor([[0.45, 0.0, 0.45, 0.55, 0.0, 0.5], [0.5, 0.0, 0.55, 0.45, 0.0, 0.45]], device=state.x.device)   # push start -> end
    # the MPM forward accumulates with LDS float atomics, so two runs of step_diff differ in their last bits: what step_with_render
    # returns is compared with what ITS OWN step_diff call returned, recorded on the way out
    calls, inner = [], env.step_diff

    def recording(a, s):
        calls.append(inner(a, s))
        return calls[-1]

    env.step_diff = recording
    with torch.no_grad():
        obs, rew, done, info = env.step_with_render(actions, state)
    env.step_diff = inner
    assert len(calls) == 1 and calls[0][0] is obs and calls[0][1] is rew and calls[0][2] is done and calls[0][3] is info
    assert calls[0][3]["state"] is info["state"] and obs.shape == (2, env.observation_size) and rew.shape == (2,)
    sl, imgs = info["state_list"], info["img_list"]
    T = sl.x.shape[0]
    assert len(imgs) == T >= 1 and all(i.shape == (120, 160, 3) and i.dtype == np.uint8 for i in imgs)
    for t in range(T):
        np.testing.assert_array_equal(imgs[t], _twin_of(env, sl, 0, t)[0])


def test_pour_water_render_is_points_over_two_bowls():
    from unidom_amd.envs.pour_water_env import DefaultConf, PourWaterEnv
    env = PourWaterEnv(batch_size=1, seed=1, conf=_conf_with_render(DefaultConf))
    _, state = env.reset(np.array([0, 7], np.uint32))
    color, depth = env.render(state)
    r = env._mpm_renderer
    assert r.conf.mode == 1 and r.conf.point_size == 1 and r.prim_kind == 1 and r.n_prims == 2
    assert tuple(np.float32(r.conf.particle_color)) == tuple(np.float32([100 / 255, 100 / 255, 249 / 255, 125 / 255]))
    want = _twin_of(env, state, 0)
    assert (want[2] >= 0).sum() > 20 and (want[2] == -4).sum() > 20 and (want[2] == -5).sum() > 20
    np.testing.assert_array_equal(depth.view(np.uint32), want[1].view(np.uint32))
    np.testing.assert_array_equal(color, want[0])
    _, _, ids = env.render_batch(state, want_id=True)
    np.testing.assert_array_equal(ids[0].cpu().numpy(), want[2])


@pytest.mark.parametrize("which", ["whip_rope", "shape_rope", "shape_rope_hard", "pour_water", "pour_soup"])
def test_default_size_frame(which):
    from unidom_amd.envs.registration import env_functions
    env = env_functions[which](batch_size=1, seed=1)
    _, state = env.reset(np.array([0, 7], np.uint32))
    color, depth = env.render(state)
    assert color.shape == (480, 640, 3) and color.dtype == np.uint8 and depth.shape == (480, 640) and depth.dtype == np.float32
    assert color.min() < 255 and depth.max() > 0
