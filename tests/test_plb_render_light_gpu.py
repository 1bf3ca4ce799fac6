"""GPU: the lit / roulette instances of k_render_image (csrc/plb_render.hip) and ud_plb_render_set_light against their specification,
tests/plb_render_light_twin.py, on the small scene of tests/plb_render_cases.py.

Parity with the reference itself stays unpinned (Taichi cannot run here): the twin is what the kernels are held to."""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import plb_render_cases as cases
import plb_render_light_cases as lcases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = (2.0, 1.0, -0.7)


def _state(B=cases.B):
    s = cases.scene()
    t = lambda a: torch.tensor(a[:B], dtype=torch.float64, device="cuda")
    return SimpleNamespace(x=t(s["x"]), prim_pos=t(s["prim_pos"]), prim_rot=t(s["prim_rot"]), prim_gap=None)


@functools.lru_cache(maxsize=None)
def _renderer(depth=2):
    from unidom_amd.engine.plb_render import PlbRenderer
    return PlbRenderer(cases.SceneConf, cases.render_conf(max_ray_depth=depth), batch_size=cases.B)


def _color():
    return torch.tensor(cases.scene()["color"], device="cuda")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _render(r, light, roulette, direction=lcases.DEFAULT_LIGHT, seed=0, mode="float"):
    """One render with the light set, the handle left unlit afterwards (the renderers are shared)."""
    r.set_light(light, roulette, direction)
    try:
        return r.render(_state(), spp=cases.SPP, seed=seed, mode=mode, color=_color(), strict=False).cpu().numpy()
    finally:
        r.set_light(False, False)


def _allowed_share():
    """4 x the largest share of pixels a one-ulp nudge of cos / sin moved past 1e-4 in the lit twin itself (tests/test_plb_render_light_cpu.py
    measured it on this scene and ten seeds and wrote it to profiles/plb_render_light_tolerance.txt), or one pixel."""
    for line in open(os.path.join(ROOT, "profiles", "plb_render_light_tolerance.txt")):
        if line.startswith("largest_share"):
            return 4.0 * float(line.split()[1])
    raise AssertionError("profiles/plb_render_light_tolerance.txt holds no largest_share line")


def _hold_to_twin(img, u8, tw, what):
    W, H = cases.render_conf().image_res
    assert img.shape == (cases.B, H, W, 3) and u8.shape == img.shape and u8.dtype == np.uint8
    allowed = max(_allowed_share() * W * H, 1.0)
    for b in range(cases.B):
        err = np.abs(img[b] - tw[b]).max(-1)
        bad = ~(err <= 1e-4)
        print(f"{what} env {b}: {int(bad.sum())} of {W * H} pixels past 1e-4 (allowed {allowed:.1f}), max err on the rest {err[~bad].max():.3e}")
        assert bad.sum() <= allowed, (what, b, int(bad.sum()))
        d8 = np.abs(u8[b].astype(np.int32) - cases.twin().to_u8(tw[b]).astype(np.int32)).max(-1)
        assert d8[~bad].max() <= 1
    assert not img[2].any() and not u8[2].any()          # status 1: zeros


@pytest.mark.parametrize("seed", [0, 5])
@pytest.mark.parametrize("light,roulette,depth", [(True, False, 2), (False, True, 2), (True, True, 2), (True, True, 3)])
def test_image_against_the_light_twin(light, roulette, depth, seed):
    r = _renderer(depth)
    img = _render(r, light, roulette, seed=seed)
    u8 = _render(r, light, roulette, seed=seed, mode="rgb_array")
    tw = lcases.twin_image(light, roulette, seed, depth=depth)
    _hold_to_twin(img, u8, tw, f"light {int(light)} roulette {int(roulette)} depth {depth} seed {seed}")
    assert img[0].max() > 0.5
    unlit = cases.twin_image(seed) if depth == 2 else None
    if unlit is not None:                                 # and the branch shows: the unlit twin is another image
        assert (np.abs(img[0] - unlit[0]).max(-1) > 1e-2).mean() > 0.2


def test_negative_z_light_is_occluded_by_the_background_plane():
    """max_ray_depth 1: exact zeros (every first hit lies where the plane is within 100 along the light).  Depth 2: the twin's image, whose
    only light is a second bounce far behind the camera (include/unidom_hip.h)."""
    for roulette in (False, True):
        img = _render(_renderer(1), True, roulette, NEG)
        assert img.shape[0] == cases.B and not img.any()
    lit = _render(_renderer(1), True, False)              # the same handle under the default light is not black
    assert lit[0].max() > 0.5 and lit[1].max() > 0.5 and not lit[2].any()
    img = _render(_renderer(2), True, False, NEG)
    u8 = _render(_renderer(2), True, False, NEG, mode="rgb_array")
    _hold_to_twin(img, u8, lcases.twin_image(True, False, 0, direction=NEG), "negative z, depth 2")
    assert (img.max(-1) > 0).mean() < 0.01


def _raw_handle():
    from unidom_amd import _lib
    rc = cases.render_conf()
    cc = _lib.ud_plb_render_conf(dx=rc.dx, voxel_res=(C.c_int * 3)(*rc.voxel_res), bake_size=rc.bake_size, sdf_threshold=rc.sdf_threshold,
                                 image_res=(C.c_int * 2)(*rc.image_res), spp=2, max_ray_depth=2, camera_pos=(C.c_double * 3)(*rc.camera_pos),
                                 camera_rot=(C.c_double * 2)(*rc.camera_rot), n_primitives=0, n_particles=cases.N, max_envs=2)
    h = C.c_void_p()
    assert _lib.lib().ud_plb_render_create(C.byref(cc), C.byref(h)) == 0
    return h


def _raw_image(h, seed=1):
    from unidom_amd import _lib
    L = _lib.lib()
    p = lambda a: C.c_void_p(a.data_ptr())
    W, H = cases.render_conf().image_res
    x = torch.tensor(cases.scene()["x"][:2], dtype=torch.float64, device="cuda")
    col = _color()
    bbox, status = torch.empty((2, 2, 3), device="cuda"), torch.empty((2,), dtype=torch.int32, device="cuda")
    img = torch.full((2, H, W, 3), -7.0, device="cuda")
    assert L.ud_plb_render_bake(h, 2, p(x), p(col), p(bbox), p(status), None) == 0
    assert L.ud_plb_render_image(h, 2, None, None, None, 2, seed, p(img), None) == 0
    return img.cpu().numpy()


def _light(on, roulette, direction):
    from unidom_amd import _lib
    return _lib.ud_plb_render_light(use_directional_light=on, use_roulette=roulette, light_direction=(C.c_double * 3)(*direction))


def test_set_light_off_is_a_fresh_handle_and_lit_calls_repeat():
    from unidom_amd import _lib
    L = _lib.lib()
    h, fresh = _raw_handle(), _raw_handle()
    try:
        never_set = _raw_image(fresh)
        base = _raw_image(h)
        assert np.array_equal(_bits(base), _bits(never_set))
        seen = [base]
        for on, roulette in ((1, 0), (0, 1), (1, 1)):
            ll = _light(on, roulette, lcases.DEFAULT_LIGHT)
            assert L.ud_plb_render_set_light(h, C.byref(ll)) == 0
            a, b = _raw_image(h), _raw_image(h)
            assert np.array_equal(_bits(a), _bits(b)), "two calls of one instance differ"
            assert all(not np.array_equal(a, s) for s in seen), "two instances gave one image"
            seen.append(a)
        ll = _light(0, 0, (0.0, 0.0, 0.0))                # both off: the direction is not read, a zero one is no error
        assert L.ud_plb_render_set_light(h, C.byref(ll)) == 0
        assert np.array_equal(_bits(_raw_image(h)), _bits(never_set))
    finally:
        L.ud_plb_render_destroy(h); L.ud_plb_render_destroy(fresh)


def test_set_light_refusals_leave_the_handle_as_it_was():
    from unidom_amd import _lib
    L = _lib.lib()
    h = _raw_handle()
    try:
        ll = _light(1, 1, (2.0, 0.3, 0.7))
        assert L.ud_plb_render_set_light(h, C.byref(ll)) == 0
        before = _raw_image(h)
        refused = [(lambda: L.ud_plb_render_set_light(h, None), "null"),
                   (lambda: L.ud_plb_render_set_light(None, C.byref(ll)), "null"),
                   (lambda: L.ud_plb_render_set_light(h, C.byref(_light(1, 0, (2.0, float("nan"), 0.7)))), "finite"),
                   (lambda: L.ud_plb_render_set_light(h, C.byref(_light(0, 0, (float("inf"), 1.0, 0.7)))), "finite"),
                   (lambda: L.ud_plb_render_set_light(h, C.byref(_light(0, 0, (1e300, 1.0, 0.7)))), "finite"),     # inf once rounded to f32
                   (lambda: L.ud_plb_render_set_light(h, C.byref(_light(1, 0, (0.0, 0.0, 0.0)))), "zero"),
                   (lambda: L.ud_plb_render_set_light(h, C.byref(_light(1, 0, (1e-60, 0.0, 0.0)))), "zero")]       # zero once rounded to f32
        for call, word in refused:
            assert call() == -1
            assert word in L.ud_last_error().decode(), L.ud_last_error()
            assert np.array_equal(_bits(_raw_image(h)), _bits(before)), word
    finally:
        L.ud_plb_render_destroy(h)


def test_torus_conf_renders_under_its_directional_light():
    """A PlbRenderer made from TorusConf takes the light from the conf's RENDERER block; switching it off on the same handle gives the sky-lit
    image, another one."""
    from unidom_amd.engine.plb_render import PlbRenderer, render_conf_of
    from unidom_amd.engine.plb_simulator import PlbSimulator, TorusConf
    conf = TorusConf()
    rc = render_conf_of(conf, image_res=(64, 48), spp=1, voxel_res=(24, 96, 24))      # 64 wide: a pixel centre meets the 0.028 wide rod
    assert rc.use_directional_light and rc.camera_pos == (0.5, 0.27, 2.5)
    sim = PlbSimulator(conf, batch_size=2)
    st = sim.reset()
    r = PlbRenderer(conf, rc, batch_size=2)
    lit = r.render(st, seed=2, mode="float")
    assert bool(torch.isfinite(lit).all()) and float(lit.max()) > 0.3 and torch.equal(lit[0], lit[1])
    g = r.gbuffer(st)["kind"]
    assert int((g == 16).sum()) > 4 and int((g == 3).sum()) + int((g == 4).sum()) > 0      # the rod and a Sphere are in view
    r.set_light(False)
    sky = r.render(st, seed=2, mode="float")
    assert float((lit - sky).abs().amax(-1).gt(1e-2).float().mean()) > 0.5
    assert torch.equal(sim.render(st, seed=2, mode="float", render_conf=rc), lit)          # PlbSimulator.render draws the conf's light too
