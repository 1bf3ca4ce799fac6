"""GPU: csrc/plb_render.hip against its specification, tests/plb_render_twin.py, on the small scene of tests/plb_render_cases.py.

Parity with the reference itself is unpinned (neither Taichi nor cv2 can run here): the twin, a NumPy f32 restatement of the reference's text
in the order include/unidom_hip.h states, is what the kernels are held to -- bit for bit wherever no cos / sin is involved."""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import plb_render_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _state(B=cases.B):
    s = cases.scene()
    t = lambda a: torch.tensor(a[:B], dtype=torch.float64, device="cuda")
    return SimpleNamespace(x=t(s["x"]), prim_pos=t(s["prim_pos"]), prim_rot=t(s["prim_rot"]), prim_gap=None)


@functools.lru_cache(maxsize=None)
def _renderer():
    from unidom_amd.engine.plb_render import PlbRenderer
    return PlbRenderer(cases.SceneConf, cases.render_conf(), batch_size=cases.B)


def _color():
    return torch.tensor(cases.scene()["color"], device="cuda")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_bake_is_bit_equal_to_the_twin_and_repeatable():
    r, tw = _renderer(), cases.twin_bake()
    got = []
    for _ in range(2):
        bbox, status = r.bake(_state(), _color())
        vol, sdf = r.volume(cases.B)
        got.append([a.cpu().numpy() for a in (bbox, status, vol, sdf)])
    for a, b in zip(*got):
        assert np.array_equal(_bits(a) if a.dtype.kind == "f" else a, _bits(b) if b.dtype.kind == "f" else b), "two bakes differ"
    bbox, status, vol, sdf = got[0]
    assert status.tolist() == [e.status for e in tw] == [0, 0, 1]
    for b, e in enumerate(tw):
        assert np.array_equal(_bits(bbox[b]), _bits(e.bbox)), (b, bbox[b], e.bbox)
        assert np.array_equal(vol[b], e.vol), (b, int((vol[b] != e.vol).sum()))
        assert np.array_equal(_bits(sdf[b]), _bits(e.sdf)), (b, float(np.abs(sdf[b] - e.sdf).max()))
    assert len(np.unique(vol[0] & 0xFFFFFF)) >= 3        # both particle colours and the untouched cells are there


@functools.lru_cache(maxsize=None)
def _gbuffer():
    r = _renderer()
    r.bake(_state(), _color())
    return {k: v.cpu().numpy() for k, v in r.gbuffer(_state()).items()}


def test_gbuffer_body_ground_background_are_bit_equal():
    g, tw = _gbuffer(), cases.twin_gbuffer()
    seen = set()
    for b in range(cases.B):
        assert np.array_equal(g["kind"][b], tw[b]["kind"]), (b, int((g["kind"][b] != tw[b]["kind"]).sum()))
        m = np.isin(tw[b]["kind"], (0, 1, 2, 16))
        seen |= set(np.unique(tw[b]["kind"][m]).tolist())
        for k, tk in (("t", "t"), ("normal", "normal"), ("albedo", "albedo")):
            assert np.array_equal(_bits(g[k][b][m]), _bits(tw[b][tk][m])), (b, k, float(np.abs(g[k][b][m] - tw[b][tk][m]).max()))
    assert seen == {0, 1, 2, 16}, seen
    assert (tw[0]["kind"] == 16).mean() > 0.25


def test_gbuffer_primitives():
    g, tw = _gbuffer(), cases.twin_gbuffer()
    for b in range(2):
        k = tw[b]["kind"]
        skip = tw[b]["exhausted"]
        assert skip.mean() <= 0.02
        m = (k >= 3) & (k < 16) & ~skip
        assert {3, 4} <= set(np.unique(k[m]).tolist())
        assert np.array_equal(g["kind"][b][~skip], k[~skip])
        rel = np.abs(g["t"][b][m] - tw[b]["t"][m]) / np.abs(tw[b]["t"][m])
        assert rel.max() <= 1e-6, (b, float(rel.max()))
        assert np.abs(g["normal"][b][m] - tw[b]["normal"][m]).max() <= 1e-5
        assert np.array_equal(g["albedo"][b][m], tw[b]["albedo"][m])


def _allowed_share():
    """4 x the largest share of pixels a one-ulp nudge of cos / sin moved past 1e-4 in the twin itself (tests/test_plb_render_cpu.py measured it
    on this scene and ten seeds and wrote it to profiles/plb_render_tolerance.txt), or one pixel."""
    for line in open(os.path.join(ROOT, "profiles", "plb_render_tolerance.txt")):
        if line.startswith("largest_share"):
            return 4.0 * float(line.split()[1])
    raise AssertionError("profiles/plb_render_tolerance.txt holds no largest_share line")


@pytest.mark.parametrize("seed", [0, 5])
def test_image_against_the_twin(seed):
    r = _renderer()
    img = r.render(_state(), spp=cases.SPP, seed=seed, mode="float", color=_color(), strict=False).cpu().numpy()
    u8 = r.render(_state(), spp=cases.SPP, seed=seed, mode="rgb_array", color=_color(), strict=False).cpu().numpy()
    tw = cases.twin_image(seed)
    W, H = cases.render_conf().image_res
    assert img.shape == (cases.B, H, W, 3) and u8.shape == img.shape and u8.dtype == np.uint8
    allowed = max(_allowed_share() * W * H, 1.0)
    for b in range(cases.B):
        err = np.abs(img[b] - tw[b]).max(-1)
        bad = err > 1e-4
        print(f"env {b} seed {seed}: {int(bad.sum())} of {W * H} pixels past 1e-4 (allowed {allowed:.1f}), max err on the rest {err[~bad].max():.3e}")
        assert bad.sum() <= allowed, (b, int(bad.sum()))
        d8 = np.abs(u8[b].astype(np.int32) - cases.twin().to_u8(tw[b]).astype(np.int32)).max(-1)
        assert d8[~bad].max() <= 1
    assert not img[2].any() and not u8[2].any()          # status 1: zeros, the other envs unaffected (above)
    assert img[0].max() > 0.5


def test_render_raises_for_a_cloud_that_does_not_fit():
    from unidom_amd import _lib
    with pytest.raises(_lib.UnidomError, match="do not fit"):
        _renderer().render(_state(), spp=1, color=_color())


def test_orientation_seed_and_batch_rows():
    r = _renderer()
    a = r.render(_state(), spp=1, seed=3, mode="float", color=_color(), strict=False).cpu().numpy()
    # the twin's image() already returns img[:, ::-1].transpose(1, 0, 2) of its [u, v] buffer; a transposed or unflipped output cannot match it
    tw = cases.twin_image(3, spp=1)
    assert (np.abs(a[0] - tw[0]).max(-1) > 1e-4).sum() <= 1
    assert (np.abs(a[0] - tw[0][::-1]).max(-1) > 1e-4).mean() > 0.2, "the image matches its vertical mirror as well: the scene shows nothing"
    b = r.render(_state(), spp=1, seed=4, mode="float", color=_color(), strict=False).cpu().numpy()
    assert not np.array_equal(a[0], b[0])
    one = r.render(_state(1), spp=1, seed=3, mode="float", color=_color()).cpu().numpy()
    assert one.shape[0] == 1 and np.array_equal(_bits(one[0]), _bits(a[0]))


def _raw_conf(**kw):
    from unidom_amd import _lib
    rc = cases.render_conf()
    base = dict(dx=rc.dx, voxel_res=(C.c_int * 3)(*rc.voxel_res), bake_size=rc.bake_size, sdf_threshold=rc.sdf_threshold,
                image_res=(C.c_int * 2)(*rc.image_res), spp=2, max_ray_depth=2, camera_pos=(C.c_double * 3)(*rc.camera_pos),
                camera_rot=(C.c_double * 2)(*rc.camera_rot), n_primitives=0, n_particles=cases.N, max_envs=2)
    base.update(kw)
    return _lib.ud_plb_render_conf(**base)


def test_refusals_touch_nothing_and_name_the_reason():
    from unidom_amd import _lib
    L = _lib.lib()
    for kw, rc, word in ((dict(use_directional_light=1), -2, "use_directional_light"), (dict(use_roulette=1), -2, "use_roulette"),
                         (dict(voxel_res=(C.c_int * 3)(24, 11, 28)), -1, "bake_size")):
        h = C.c_void_p()
        cc = _raw_conf(**kw)
        assert L.ud_plb_render_create(C.byref(cc), C.byref(h)) == rc
        assert not h.value and word in L.ud_last_error().decode(), L.ud_last_error()
    h = C.c_void_p()
    cc = _raw_conf()
    assert L.ud_plb_render_create(C.byref(cc), C.byref(h)) == 0
    try:
        x = torch.tensor(cases.scene()["x"], dtype=torch.float64, device="cuda")
        col = _color()
        mark = lambda *shape, dt=torch.float32: torch.full(shape, -7, dtype=dt, device="cuda")
        bbox, status = mark(3, 2, 3), mark(3, dt=torch.int32)
        W, H = cases.render_conf().image_res
        kind, t, nrm, alb, img = mark(3, W, H, dt=torch.int32), mark(3, W, H), mark(3, W, H, 3), mark(3, W, H, 3), mark(3, H, W, 3)
        outs = (bbox, status, kind, t, nrm, alb, img)
        p = lambda a: C.c_void_p(a.data_ptr())
        null = C.c_void_p(0)
        calls = [
            (lambda: L.ud_plb_render_bake(h, 3, p(x), p(col), p(bbox), p(status), null), "max_envs"),
            (lambda: L.ud_plb_render_bake(h, 2, null, p(col), p(bbox), p(status), null), "null"),
            (lambda: L.ud_plb_render_bake(h, 2, p(x), p(col), p(bbox), null, null), "null"),
            (lambda: L.ud_plb_render_gbuffer(h, 3, null, null, null, p(kind), p(t), p(nrm), p(alb), null), "max_envs"),
            (lambda: L.ud_plb_render_gbuffer(h, 2, null, null, null, p(kind), null, p(nrm), p(alb), null), "null"),
            (lambda: L.ud_plb_render_image(h, 3, null, null, null, 1, 0, p(img), null), "max_envs"),
            (lambda: L.ud_plb_render_image(h, 2, null, null, null, 1, 0, null, null), "null"),
        ]
        for call, word in calls:
            assert call() == -1
            assert word in L.ud_last_error().decode(), L.ud_last_error()
        torch.cuda.synchronize()
        for o in outs:
            assert bool((o == -7).all()), "a refused call wrote to an output"
    finally:
        L.ud_plb_render_destroy(h)


def test_constant_orientation_of_the_conf_is_drawn_without_rot_state():
    """A handle without rot_state carries no prim_rot in its state: the primitive's orientation is the conf's constant (PlbConf.prim_rot), the
    one the simulator handle is made with.  The renderer must draw that pose, not the identity."""
    from unidom_amd.engine.plb_render import PlbRenderer
    s = cases.scene()

    class ConstConf(cases.SceneConf):
        prim_rot = tuple(tuple(q) for q in s["prim_rot"][0])
    r = PlbRenderer(ConstConf, cases.render_conf(), batch_size=cases.B)
    st = _state()
    st.prim_rot = None
    r.bake(st, _color())
    g = {k: v.cpu().numpy() for k, v in r.gbuffer(st).items()}
    want, tw = _gbuffer(), cases.twin_gbuffer()          # the same quaternions given as state: held to the twin above
    for k in ("kind", "t", "normal", "albedo"):
        assert np.array_equal(g[k], want[k]), k
    assert np.array_equal(g["kind"][0], tw[0]["kind"])
    # and the identity would have shown: the twin with the Capsule upright hits other pixels
    from plb_render_twin import prims_of
    upright = cases.twin().gbuffer(cases.twin_bake()[0], prims_of(cases.SceneConf, s["prim_pos"][0]))
    assert (upright["kind"] != tw[0]["kind"]).sum() >= 4


def test_simulator_render_draws_the_conf_orientation():
    """PlbSimulator.render on a non-rot_state Capsule handle (reset() leaves prim_rot None) equals the renderer given the conf's quaternion as
    state, and differs from the upright pose."""
    from unidom_amd.engine.plb_render import PlbRenderer, render_conf_of
    from unidom_amd.engine.plb_simulator import PlbSimulator, WriterConf
    th = 1.0

    class Tilted(WriterConf):
        n_particles = 200
        prim_rot = ((np.cos(th / 2), 0.0, 0.0, np.sin(th / 2)),)
    conf = Tilted()
    rc = render_conf_of(conf, image_res=(32, 24), spp=1, voxel_res=(64, 32, 64), camera_pos=(0.5, 0.3, 1.0), camera_rot=(0.25, 0.0))
    sim = PlbSimulator(conf, batch_size=2)
    st = sim.reset()
    assert st.prim_rot is None and sim.launch_plan() == 1
    img = sim.render(st, seed=2, mode="float", render_conf=rc)
    r = PlbRenderer(conf, rc, batch_size=2)
    rot = lambda q: torch.tensor([[q]] * 2, dtype=torch.float64, device="cuda")
    given = SimpleNamespace(x=st.x, prim_pos=st.prim_pos, prim_rot=rot(conf.prim_rot[0]), prim_gap=None)
    assert torch.equal(img, r.render(given, seed=2, mode="float"))
    g = r.gbuffer(given)["kind"]
    assert int((g == 3).sum()) > 20                      # the Capsule is in view
    upright = SimpleNamespace(x=st.x, prim_pos=st.prim_pos, prim_rot=rot((1.0, 0.0, 0.0, 0.0)), prim_gap=None)
    assert int((r.gbuffer(upright)["kind"] != g).sum()) >= 8
    assert not torch.equal(img, r.render(upright, seed=2, mode="float"))


def test_caller_colours_are_masked_to_24_bits():
    r = _renderer()
    col = _color()
    r.bake(_state(), col)
    a, _ = r.volume(2)
    r.bake(_state(), col.to(torch.int64) | (5 << 24))    # stray high bits must not reach the distance bits
    b, _ = r.volume(2)
    assert torch.equal(a, b)


def test_full_size_rope_handle_runs_the_multi_kernel_path():
    """A 1500-particle env has 47 parts of 32 particles, more than the 32 workgroups one XCD holds at the persistent kernels' occupancy: the
    library must not pick the persistent path for it (its parts would wait for siblings that cannot start), and says so when it is forced."""
    from unidom_amd import _lib
    from unidom_amd.engine.plb_simulator import PlbSimulator, RopeConf, TableConf

    class Forced(RopeConf):
        path = 2

    class Cut(RopeConf):
        n_particles = 1024
    with pytest.raises(_lib.UnidomError, match="does not fit"):
        PlbSimulator(Forced(), batch_size=2)
    assert PlbSimulator(Cut(), batch_size=2).launch_plan() == 2
    for conf in (RopeConf(), TableConf()):
        sim = PlbSimulator(conf, batch_size=2)
        assert sim.launch_plan() == 1
        with torch.no_grad():
            st = sim.step(sim.reset(), torch.tensor([[0.0, 0.5, 0.0]] * 2, dtype=torch.float64, device="cuda"))
        sim.check_status()
        assert bool(torch.isfinite(st.x).all()) and abs(float(st.prim_pos[0, 0, 1]) - (conf.prim_init_pos[0][1] + 0.0025)) < 1e-12


def test_unfold_small():
    """The Rope sweep cut down: 300 particles, window 2, steps 2, tail 2, a 32 x 32 image, spp 1 (and a volume just large enough for the sheet, so
    that the twin's twelve bakes stay quick).  The coverages are blue_coverage of the twin's render of the same final states."""
    from plb_render_twin import RenderTwin, prims_of
    from unidom_amd.algorithms.plb_unfold import blue_coverage, unfold
    from unidom_amd.engine.plb_render import render_conf_of
    from unidom_amd.engine.plb_simulator import RopeConf

    class SmallRope(RopeConf):
        n_particles = 300
    conf = SmallRope()
    rc = render_conf_of(conf, image_res=(32, 32), spp=1, voxel_res=(80, 24, 80))
    res = unfold(conf, window=2, steps=2, tail=2, render_conf=rc, seed=1)
    assert res["coverage"].shape == (12,) and res["image"].shape == (12, 32, 32, 3)
    tw = RenderTwin(rc)
    x, pp = res["state"].x.cpu().numpy(), res["state"].prim_pos.cpu().numpy()
    color = np.full(300, conf.particle_color, np.int32)
    imgs = []
    for b in range(12):
        e = tw.bake_one(x[b], color)
        assert e.status == 0
        imgs.append(tw.to_u8(tw.image(e, prims_of(conf, pp[b]), spp=1, seed=1)))
    want = blue_coverage(torch.tensor(np.stack(imgs))).numpy()
    assert want.max() > 0, "no blue pixel in the twin's images: the test shows nothing"
    assert np.array_equal(res["coverage"], want), (res["coverage"], want)
    assert res["index"] == int(np.argmax(want)) and res["max_acxel"] == (0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5, 0.55, 0.6, 0.65)[res["index"]]
