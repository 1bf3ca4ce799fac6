"""GPU: the cloth renderer (csrc/cloth_render.hip behind ud_cloth_render_*, engine/cloth_render.py, ClothEnv.render / render_batch /
step_with_render) against its specification tests/cloth_render_twin.py: triangle id, depth bits and colour equal in every pixel --
the arithmetic has no unpinned function, so no pixel is exempt.  What the twin itself is held to: tests/test_cloth_render_cpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cloth_render_twin as twin
from cloth_render_cases import kernel_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Handle:
    """a bare ud_cloth_render handle over explicit faces (the kernel-level tests go below ClothRenderer, which takes a simulator)"""

    def __init__(self, conf, faces, V, S, max_frames):
        from unidom_amd import _lib
        self.lib, self.conf, self.V, self.S = _lib, conf, V, S
        d3, d2, f3 = (lambda v: (C.c_double * 3)(*v)), (lambda v: (C.c_double * 2)(*v)), (lambda v: (C.c_float * 3)(*v))
        self.cc = _lib.ud_cloth_render_conf(
            width=conf.width, height=conf.height, yfov=conf.yfov, znear=conf.znear, camera_pos=d3(conf.camera_pos),
            camera_target=d3(conf.camera_target), camera_up=d3(conf.camera_up), ground_min=d2(conf.ground_min), ground_max=d2(conf.ground_max),
            ground_z=conf.ground_z, cloth_color=f3(conf.cloth_color), ground_color=f3(conf.ground_color), sphere_color=f3(conf.sphere_color),
            n_vertices=V, n_faces=len(faces), n_spheres=S, max_frames=max_frames)
        self.faces = np.ascontiguousarray(faces, np.int32)
        self.h = C.c_void_p()
        self.rc = _lib.lib().ud_cloth_render_create(C.byref(self.cc), self.faces.ctypes.data_as(C.c_void_p), C.byref(self.h))

    def __del__(self):
        if self.h:
            self.lib.lib().ud_cloth_render_destroy(self.h)

    def outputs(self, M, fill=None):
        H, W = self.conf.height, self.conf.width
        mk = (lambda s, dt: torch.empty(s, dtype=dt, device=DEV)) if fill is None else (lambda s, dt: torch.full(s, fill, dtype=dt, device=DEV))
        return mk((M, H, W, 3), torch.uint8), mk((M, H, W), torch.float32), mk((M, H, W), torch.int32)

    def call(self, M, verts, spheres, color, depth, tri, handle=True):
        p = lambda t: C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())
        rc = self.lib.lib().ud_cloth_render_frames(self.h if handle else C.c_void_p(0), M, p(verts), p(spheres), p(color), p(depth), p(tri),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc


@functools.lru_cache(maxsize=None)
def _scene(size):
    conf, faces, verts, spheres = kernel_scene(*size)
    want = [twin.render(conf, faces, verts[m], spheres[m]) for m in range(3)]
    return conf, faces, verts, spheres, want


def _dev(a):
    return torch.tensor(a, device=DEV).contiguous()


@pytest.mark.parametrize("size", [(50, 38), (37, 29)])
def test_kernels_equal_the_twin_in_every_pixel(size):
    conf, faces, verts, spheres, want = _scene(size)
    kinds = set(np.unique(want[0][2]).tolist())
    assert {-1, -2, -3} <= kinds and len([k for k in kinds if k >= 0]) >= 3      # the twin's own output holds every kind
    h = _Handle(conf, faces, verts.shape[1], 2, 3)
    assert h.rc == 0
    v, s = _dev(verts), _dev(spheres)
    color, depth, tri = h.outputs(3)
    assert h.call(3, v, s, color, depth, tri) == 0
    for m in range(3):
        np.testing.assert_array_equal(tri[m].cpu().numpy(), want[m][2])
        np.testing.assert_array_equal(depth[m].cpu().numpy().view(np.uint32), want[m][1].view(np.uint32))
        np.testing.assert_array_equal(color[m].cpu().numpy(), want[m][0])
    # a second call: identical bits; tri may be NULL
    c2, d2, t2 = h.outputs(3)
    assert h.call(3, v, s, c2, d2, t2) == 0
    assert torch.equal(c2, color) and torch.equal(d2.view(torch.int32), depth.view(torch.int32)) and torch.equal(t2, tri)
    c3, d3, _ = h.outputs(3)
    assert h.call(3, v, s, c3, d3, None) == 0
    assert torch.equal(c3, color) and torch.equal(d3.view(torch.int32), depth.view(torch.int32))
    # M = 1 is frame 0 of M = 3
    c1, d1, t1 = h.outputs(1)
    assert h.call(1, v[:1].contiguous(), s[:1].contiguous(), c1, d1, t1) == 0
    assert torch.equal(c1[0], color[0]) and torch.equal(d1[0].view(torch.int32), depth[0].view(torch.int32)) and torch.equal(t1[0], tri[0])


def test_invalid_arguments_touch_nothing():
    from unidom_amd import _lib
    conf, faces, verts, spheres, _ = _scene((37, 29))
    V = verts.shape[1]
    h = _Handle(conf, faces, V, 2, 3)
    v, s = _dev(verts), _dev(spheres)
    big_v, big_s = _dev(np.concatenate([verts, verts[:1]])), _dev(np.concatenate([spheres, spheres[:1]]))
    color, depth, tri = h.outputs(4, fill=7)

    def untouched():
        return bool((color == 7).all()) and bool((depth == 7).all()) and bool((tri == 7).all())

    for rc in (h.call(0, v, s, color, depth, tri), h.call(4, big_v, big_s, color, depth, tri), h.call(3, None, s, color, depth, tri),
               h.call(3, v, None, color, depth, tri), h.call(3, v, s, None, depth, tri), h.call(3, v, s, color, None, tri),
               h.call(3, v, s, color, depth, tri, handle=False)):
        assert rc == -1                                         # UD_ERR_INVALID
        assert untouched()
    assert b"ud_cloth_render_frames" in _lib.lib().ud_last_error()
    # create: a face index outside [0, V), a null conf; sizes past what the kernels cover
    bad = faces.copy()
    bad[3, 1] = V
    assert _Handle(conf, bad, V, 2, 3).rc == -1
    bad[3, 1] = -1
    assert _Handle(conf, bad, V, 2, 3).rc == -1
    assert _lib.lib().ud_cloth_render_create(C.c_void_p(0), h.faces.ctypes.data_as(C.c_void_p), C.byref(C.c_void_p())) == -1
    assert _Handle(twin.Conf(width=5000, height=29), faces, V, 2, 3).rc == -2          # UD_ERR_UNSUPPORTED
    assert _Handle(conf, faces, V, 17, 3).rc == -2


def test_supported_sizes_create():
    """V = 180^2, F = 2 * 179^2 and a 1024 x 1024 image are inside the supported range (create only: sizes, arena, index check)"""
    N = 180
    i, j = np.meshgrid(np.arange(N - 1), np.arange(N - 1), indexing="ij")
    a, b, c, d = i * N + j, (i + 1) * N + j, i * N + j + 1, (i + 1) * N + j + 1
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([d, c, b], -1).reshape(-1, 3)]).astype(np.int32)
    assert len(faces) == 2 * 179 * 179
    assert _Handle(twin.Conf(width=1024, height=1024), faces, N * N, 1, 2).rc == 0


# ---- env level ------------------------------------------------------------------------------------------------------------------------
def _twin_of(env, x_grid, prim0):
    return twin.render(twin.Conf(), np.asarray(env.simulator.indices), x_grid.cpu().numpy().reshape(-1, 3), prim0.cpu().numpy().reshape(1, 4))


def _same(color, depth, want):
    np.testing.assert_array_equal(depth.view(np.uint32), want[1].view(np.uint32))
    np.testing.assert_array_equal(color, want[0])


def test_fold_cloth1_render_and_render_batch():
    from unidom_amd.envs.fold_cloth1_env import FoldCloth1Env
    env = FoldCloth1Env(2)
    assert getattr(env, "_cloth_renderer", None) is None            # nothing is allocated before the first render call
    _, state = env.reset(np.array([0, 1], np.uint32))
    color, depth = env.render(state)
    assert isinstance(color, np.ndarray) and color.shape == (480, 640, 3) and color.dtype == np.uint8
    assert isinstance(depth, np.ndarray) and depth.shape == (480, 640) and depth.dtype == np.float32
    assert len(env.simulator.indices) == 840
    want = _twin_of(env, env.get_x_grid(state)[0], state.primitive0[0])
    _same(color, depth, want)
    kinds = want[2]
    assert (kinds >= 0).sum() > 5000 and (kinds == -3).sum() > 50000 and (kinds == -1).sum() > 1000 and (kinds == -2).sum() > 50
    cb, db, tb = env.render_batch(state, want_tri=True)
    assert cb.shape == (2, 480, 640, 3) and cb.dtype == torch.uint8 and db.shape == (2, 480, 640) and db.dtype == torch.float32
    _same(cb[0].cpu().numpy(), db[0].cpu().numpy(), want)
    np.testing.assert_array_equal(tb[0].cpu().numpy(), want[2])
    assert torch.equal(cb[0], cb[1]) and torch.equal(db[0], db[1])  # the two envs are equal at reset ...
    moved = state._replace(x=torch.stack([state.x[0], state.x[1] + torch.tensor([0.05, 0.02, 0.0], device=state.x.device)]))
    cm, dm = env.render_batch(moved)
    assert torch.equal(cm[0], cb[0]) and not torch.equal(cm[1], cb[1]) and not torch.equal(dm[1], db[1])   # ... and differ once one moves
    with pytest.raises(NotImplementedError):
        env.get_obs(state, obs_type="RGB")


def test_step_with_render_is_step_diff_plus_forty_frames():
    from unidom_amd.envs.fold_cloth1_env import FoldCloth1Env
    env = FoldCloth1Env(2)
    _, state = env.reset(np.array([0, 1], np.uint32))
    p = state.x[:, 100].detach()
    actions = torch.cat([p, p + torch.tensor([0.1, 0.0, 0.1], device=p.device)], -1)     # pick a cloth particle, place it elsewhere
    obs0, rew0, done0, info0 = env.step_diff(actions, state)
    obs, rew, done, info = env.step_with_render(actions, state)
    assert torch.equal(obs, obs0) and torch.equal(rew, rew0) and torch.equal(done, done0) and torch.equal(info["state"].x, info0["state"].x)
    imgs = info["img_list"]
    assert len(imgs) == 40 and all(i.shape == (480, 640, 3) and i.dtype == np.uint8 for i in imgs)
    sl = info["state_list"]
    for k in (0, 8, 39):                                             # first, one of the lift phase (macro steps 3..12), last
        want = _twin_of(env, env.simulator.get_x_grid(sl.x[k, :1])[0], sl.primitive0[k, 0])
        np.testing.assert_array_equal(imgs[k], want[0])
    assert not np.array_equal(imgs[0], imgs[39])


def test_fold_tshirt_frame_equals_the_twin():
    from unidom_amd.envs.fold_cloth_tshirt_env import FoldTshirtEnv
    env = FoldTshirtEnv(1)
    _, state = env.reset(np.array([0, 3], np.uint32))
    assert len(env.simulator.indices) == 6536
    color, depth = env.render(state)
    _same(color, depth, _twin_of(env, env.get_x_grid(state)[0], state.primitive0[0]))
