"""CPU: the specification of the lit / roulette image (tests/plb_render_light_twin.py) against definitions that do not share its code, TorusConf
against torus.yml, plb_release's action table and parameter draws against the reference's formulas, and the measurement the GPU test's
allowance comes from (profiles/plb_render_light_tolerance.txt)."""
import os

import numpy as np

import plb_render_cases as cases
import plb_render_light_cases as lcases
from plb_render_light_twin import LIGHT_K, LightTwin
from plb_render_twin import F, rand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCE_FILE = os.path.join(ROOT, "profiles", "plb_render_light_tolerance.txt")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _hash_by_hand(seed, pixel, sample, k):
    M = 0xFFFFFFFF
    x = seed ^ ((pixel * 0x9E3779B9 + sample * 0x85EBCA6B + k * 0xC2B2AE35) & M)
    x ^= x >> 16; x = (x * 0x7feb352d) & M; x ^= x >> 15; x = (x * 0x846ca68b) & M; x ^= x >> 16
    return x


def _draw_by_hand(seed, pixels, sample, k):
    return np.array([(_hash_by_hand(seed, int(p), sample, k) >> 8) * 2.0 ** -24 for p in pixels])


def _empty_env():
    """The bbox of env 2 (nothing baked) with an empty volume: next_hit sees the ground, the background plane and the sky only."""
    tw, e = cases.twin(), cases.twin_bake()[2]
    return type(e)(e.bbox, 0, np.full(tw.res, 2 ** 32 - 1, np.int64), np.ones(tw.res, np.float32))


def test_both_flags_off_is_the_unlit_twin_bit_for_bit():
    for seed in (0, 5):
        base, off = cases.twin_image(seed), lcases.twin_image(False, False, seed)
        for b in range(cases.B):
            assert np.array_equal(_bits(base[b]), _bits(off[b])), (seed, b)
    # the conf's own fields are what a LightTwin without arguments takes, and the default direction does not matter while the light is off
    tw = LightTwin(cases.render_conf())
    assert not tw.light and not tw.roulette and tw.light_direction.tolist() == [2.0, 1.0, F(0.7)]


def test_draw_indices_of_the_new_branches_cannot_meet_the_old_ones():
    # bounce b: 2 + 4b + 0..3 < 2^30 <= 2^30 + 4b + 0..3 < 2^32 for every b up to 2^28 - 2 (a depth no image is traced to)
    deepest = 2 ** 28 - 2
    assert LIGHT_K == 2 ** 30 and 2 + 4 * deepest + 3 < LIGHT_K and LIGHT_K + 4 * deepest + 3 < 2 ** 32
    px = np.arange(384, dtype=np.uint32)
    for s, k in ((0, LIGHT_K), (1, LIGHT_K + 3), (1, LIGHT_K + 4 + 2)):
        assert np.array_equal(rand(9, px, s, k), _draw_by_hand(9, px, s, k).astype(np.float32))


def test_lit_ground_against_an_independent_f64_evaluation():
    """Empty body, no primitives, max_ray_depth 1: a sample that meets the ground contributes colour * dot, dot = the y component of the
    noised, normalised light direction (nothing stands between the ground and a light with positive y and z).  Evaluated in f64 from the text
    of the reference, sharing only the draws; pixels with a sample on the background plane (whose offset origin can land behind the plane in
    f32) or within 1e-4 of a checker edge are left out."""
    rc = cases.render_conf(max_ray_depth=1)
    spp, seed, L = 2, 3, np.array(lcases.DEFAULT_LIGHT)
    img = LightTwin(rc, True, False, lcases.DEFAULT_LIGHT).image(_empty_env(), [], spp=spp, seed=seed)
    W, H = rc.image_res
    u, v = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    pixel = (u * H + v).astype(np.uint32)
    r0, r1 = rc.camera_rot
    mat = np.array([[np.cos(r1), 0, np.sin(r1)], [0, 1, 0], [-np.sin(r1), 0, np.cos(r1)]]) @ \
        np.array([[1, 0, 0], [0, np.cos(r0), np.sin(r0)], [0, -np.sin(r0), np.cos(r0)]])
    cam = np.array(rc.camera_pos)
    acc, robust = np.zeros((W * H, 3)), np.ones(W * H, bool)
    for s in range(spp):
        ju, jv = rand(seed, pixel, s, 0).astype(np.float64), rand(seed, pixel, s, 1).astype(np.float64)
        c = np.stack([2 * 0.23 * (u + ju) / H - 0.23 * (W / H) - 1e-5, 2 * 0.23 * (v + jv) / H - 0.23 - 1e-5, -np.ones(W * H)], axis=-1)
        d = (c / np.linalg.norm(c, axis=1, keepdims=True)) @ mat.T
        with np.errstate(all="ignore"):
            t_plane = -(cam[2] + 5.5) / d[:, 2]
            t_ground = (cam[1] + 0.002) / (-d[:, 1])
        on_ground = (d[:, 1] < 0) & (t_ground < 100) & ~((t_plane > 0) & (t_plane < t_ground))
        p = cam + d * np.where(on_ground, t_ground, 0.0)[:, None]
        inside = (p[:, 0] <= 1) & (p[:, 0] >= 0) & (p[:, 2] <= 1) & (p[:, 2] >= 0)
        f = np.where(inside, ((p[:, 0] / 0.25).astype(int) + (p[:, 2] / 0.25).astype(int)) % 2 * 0.2 + 0.35, 0.4)
        edge = np.minimum(np.abs(p[:, 0] / 0.25 - np.round(p[:, 0] / 0.25)), np.abs(p[:, 2] / 0.25 - np.round(p[:, 2] / 0.25))) * 0.25
        robust &= on_ground & (edge > 1e-4) & (np.abs(t_plane - t_ground) > 1e-4)
        noise = np.stack([(rand(seed, pixel, s, LIGHT_K + j).astype(np.float64) - 0.5) * 0.03 for j in range(3)], axis=-1)
        direct = L + noise
        dot = (direct / np.linalg.norm(direct, axis=1, keepdims=True))[:, 1]
        assert (dot > 0.3).all()
        acc += np.where(on_ground[:, None], np.array([0.3, 0.5, 0.7]) * f[:, None] * dot[:, None], 0.0)
    darken = 1 - 0.9 * np.sqrt((u / W - 0.5) ** 2 + (v / H - 0.5) ** 2)
    want = np.sqrt(acc * darken[:, None] * 1.5 / spp).reshape(W, H, 3)[:, ::-1].transpose(1, 0, 2)
    m = robust.reshape(W, H)[:, ::-1].T
    assert m.sum() > 150, int(m.sum())
    err = np.abs(img.astype(np.float64) - want)[m]
    assert err.max() < 1e-6, float(err.max())
    assert img[m].min() > 0.1 and np.ptp(want[m][:, 0]) > 0.05          # lit, and the checker shows


def test_negative_z_light():
    """The background plane takes part in the shadow ray: under (2, 1, -0.7) it lies -(z + 5.5) / direct_z away, within 100 for every point
    with z <= 24.4.  Every first hit of this camera is such a point, so a max_ray_depth 1 image is exactly zero; at depth 2 the only lit
    samples are second bounces that landed on the unbounded ground further behind the camera than that."""
    neg = (2.0, 1.0, -0.7)
    for seed in (0, 5):
        for img in lcases.twin_image(True, False, seed, direction=neg, depth=1):
            assert not img.any()
        for img in lcases.twin_image(True, True, seed, direction=neg, depth=1):
            assert not img.any()
    tw = lcases.light_twin(True, False, neg)
    seen = 0
    for seed in (0, 1):
        for b in range(2):
            rec = []
            tw.image(cases.twin_bake()[b], cases.twin_prims(b), seed=seed, records=rec)
            for rs in rec:
                assert rs[0]["facing"].sum() > 100 and rs[0]["occluded"][rs[0]["facing"]].all() and not rs[0]["lit"].any()
                seen += sum(int(r["lit"].sum()) for r in rs[1:])
    assert seen >= 1            # (seed 0, env 0) has one: the remark of the header is about something that happens


def test_shadow_condition_on_the_scene():
    """First-bounce shadow rays at the pixel centres: the body and the primitives shade some of the ground, most of it is lit."""
    for direction in (lcases.DEFAULT_LIGHT, (2.0, 0.3, 0.7)):
        tw = lcases.light_twin(True, False, direction)
        for b in range(2):
            rec = []
            img = tw.image(cases.twin_bake()[b], cases.twin_prims(b), spp=1, seed=0, records=rec, centre=True)
            r = rec[0][0]
            occluded, lit = int(r["occluded"].sum()), int(r["lit"].sum())
            print(f"light {direction} env {b}: facing {int(r['facing'].sum())} occluded {occluded} lit {lit}")
            assert occluded >= 10 and lit >= 100
            assert np.array_equal(r["facing"], r["occluded"] | r["lit"]) and not (r["occluded"] & r["lit"]).any()
            assert np.array_equal(r["facing"], r["hit"] & (r["dot"] > 0))
            # an occluded first bounce leaves nothing from that bounce: with one sample and one bounce the pixel is black
            one = LightTwin(cases.render_conf(max_ray_depth=1), True, False, direction)
            rec1 = []
            img1 = one.image(cases.twin_bake()[b], cases.twin_prims(b), spp=1, seed=0, records=rec1, centre=True)
            W, H = one.img
            flat = img1[::-1].transpose(1, 0, 2).reshape(W * H, 3)          # back to (u, v) order
            assert np.array_equal(rec1[0][0]["lit"], r["lit"])
            assert not flat[~r["lit"]].any() and (flat[r["lit"]].max(-1) > 0).all()
            assert img.shape == img1.shape


def test_roulette_by_hand():
    """Bounce 0 of every pixel: throughput = colour / max(colour) where the draw k = 2^30 + 3 is <= max(colour), else 0 and the path ends.
    Bounce 1: the lanes that met the sky roll too (draw k = 2^30 + 7 against the throughput they arrived with)."""
    seed, s = 4, 1
    tw = lcases.light_twin(False, True)
    e, prims = cases.twin_bake()[0], cases.twin_prims(0)
    rec = []
    tw.image(e, prims, spp=2, seed=seed, records=rec)
    r0, r1 = rec[s]
    u, v = tw.pixels()
    pixel = (u * tw.img[1] + v).astype(np.uint32)
    assert np.array_equal(r0["lanes"], np.arange(pixel.size))
    hit = tw.next_hit(e, prims, tw.cam, tw.camera_ray(u, v, rand(seed, pixel, s, 0), rand(seed, pixel, s, 1)))
    colour = np.where((hit["kind"] != 0)[:, None], hit["c"], F(1.0)).astype(np.float64)
    draw = _draw_by_hand(seed, pixel, s, 2 ** 30 + 3)
    keep = draw <= colour.max(1)
    assert np.array_equal(r0["survived"], keep) and 20 < keep.sum() < keep.size - 20
    want = np.where(keep[:, None], colour / colour.max(1, keepdims=True), 0.0)
    assert np.abs(r0["throughput"] - want).max() < 1e-7
    assert np.array_equal(r0["throughput"][keep].max(1), np.ones(keep.sum(), np.float32))
    # bounce 1 runs the survivors that hit something
    went_on = keep & r0["hit"]
    assert np.array_equal(r1["lanes"], np.nonzero(went_on)[0])
    sky = ~r1["hit"]
    assert sky.sum() > 10, "no second bounce of this sample meets the sky: the test shows nothing"
    before = r0["throughput"][r1["lanes"]].astype(np.float64)
    draw1 = _draw_by_hand(seed, pixel[r1["lanes"]], s, 2 ** 30 + 4 + 3)
    assert np.array_equal(r1["draw"], draw1.astype(np.float32))
    m1 = before.max(1)                                        # 1 after bounce 0's division: the sky lanes always survive, and are divided
    assert np.array_equal(r1["survived"][sky], draw1[sky] <= m1[sky]) and r1["survived"][sky].all()
    assert np.abs(r1["throughput"][sky] - before[sky] / m1[sky, None]).max() < 1e-7
    stopped = ~r1["survived"]
    assert stopped.sum() > 5 and not r1["throughput"][stopped].any()


def test_torus_conf_against_the_yml_file():
    from unidom_amd.engine.plb_render import RenderConf, render_conf_of
    from unidom_amd.engine.plb_simulator import PlbConf, TorusConf
    t = TorusConf()
    # torus.yml: SIMULATOR, SHAPES, PRIMITIVES
    assert (t.yield_stress, t.gravity, t.ground_friction) == (1762.2, (0.0, -0.4, 0.0), 0.5)
    assert (t.n_particles, t.box_width, t.box_init_pos, t.particle_color) == (1000, (0.028, 0.5, 0.028), (0.5, 0.3, 0.5), 100)
    assert (t.prim_kind, t.prim_radius, t.prim_init_pos) == ((0, 0), (0.025, 0.025), ((0.475, 0.05, 0.5), (0.5, 0.55, 0.5)))
    assert t.prim_color == ((0.7, 0.7, 0.7), (0.7, 0.7, 0.7)) and t.action_scale == (1.0, 1.0, 1.0)
    # RENDERER: use_directional_light: True, camera_pos: (0.5, 0.27, 2.5), camera_rot: (0., 0.)
    r = render_conf_of(t)
    assert (r.use_directional_light, r.camera_pos, r.camera_rot) == (True, (0.5, 0.27, 2.5), (0.0, 0.0))
    assert (r.light_direction, r.use_roulette, r.spp, r.max_ray_depth) == ((2.0, 1.0, 0.7), False, 50, 2)       # default_config.py
    # PlbConf keeps what it had: no RENDERER block, no colours
    p = render_conf_of(PlbConf())
    d = RenderConf()
    assert not hasattr(PlbConf, "render_overrides") and not hasattr(PlbConf, "prim_color") and not hasattr(PlbConf, "particle_color")
    assert (p.use_directional_light, p.camera_pos, p.camera_rot) == (False, (0.5, 1.2, 4.0), (0.2, 0.0)) == (d.use_directional_light, d.camera_pos, d.camera_rot)
    for name in ("n_particles", "E", "nu", "yield_stress", "box_width", "box_init_pos", "prim_radius", "prim_init_pos", "softness", "action_scale"):
        assert getattr(TorusConf, name) == getattr(PlbConf, name), name


def test_release_action_table_and_parameter_draws():
    from unidom_amd.algorithms.plb_release import START_POS, release_actions, release_parameters
    p0 = np.array([0.475, 0.05, 0.5])
    assert START_POS == (0.2, 0.3, 0.5)
    a = release_actions(p0)
    assert a.shape == (600, 3) and not a[200:].any()
    step = (np.array(START_POS) - p0) / 199                  # solver.py:301-303: 200 points, 199 equal differences, the first once more
    assert np.abs(a[:200] - step).max() < 1e-15 and np.array_equal(a[199], a[0])
    assert np.abs(p0 + a[:199].sum(0) - START_POS).max() < 1e-13 and a[0, 2] == 0.0
    small = release_actions(p0, approach=6, hold=3, tail=4)
    assert small.shape == (13, 3) and np.abs(small[:6] - (np.array(START_POS) - p0) / 5).max() < 1e-15 and not small[6:].any()
    # :127-144, run i of version 3
    st = np.random.get_state()
    E, nu, ys = release_parameters(3, 4)
    assert all(np.array_equal(x, y) for x, y in zip(np.random.get_state()[1:3], st[1:3])), "the global NumPy state moved"
    for i in range(4):
        rs = np.random.RandomState(3 * 1000 + i)
        assert E[i] == rs.uniform(500, 10500) and nu[i] == rs.uniform(0.2, 0.4)
    assert (ys == 200).all() and len(set(E.tolist())) == 4 and (E >= 500).all() and (E < 10500).all() and (nu >= 0.2).all() and (nu < 0.4).all()


def test_measurement_one_ulp_of_cos_sin_and_the_light_tolerance_file():
    """The lit and the lit + roulette twin against themselves with every cos / sin result moved by one ulp (up on even seeds, down on odd
    ones), on the GPU test's scene and ten seeds: the largest share of pixels that moves by more than 1e-4.  A nudge can flip a shadow ray, a
    roulette outcome cannot flip (its draw is compared with products of colours, no cos / sin enters).
    profiles/plb_render_light_tolerance.txt holds the share; the GPU test allows four times that (or one pixel)."""
    W, H = cases.render_conf().image_res
    worst, worst_err, lines = 0.0, 0.0, []
    for roulette in (False, True):
        for seed in range(10):
            nudge = 1 if seed % 2 == 0 else -1
            base, moved = lcases.twin_image(True, roulette, seed), lcases.twin_image(True, roulette, seed, nudge=nudge)
            for b in range(2):
                err = np.abs(moved[b] - base[b]).max(-1)
                share = float((err > 1e-4).mean())
                worst, worst_err = max(worst, share), max(worst_err, float(err[err <= 1e-4].max()))
                lines.append(f"light 1 roulette {int(roulette)} seed {seed} nudge {nudge:+d} env {b}: share {share:.6f} "
                             f"max_err_below_bar {float(err[err <= 1e-4].max()):.3e}")
    text = ("# tests/test_plb_render_light_cpu.py: lit twin against itself, cos / sin nudged by one ulp, scene of tests/plb_render_cases.py "
            f"({W} x {H}, spp {cases.SPP}), light (2, 1, 0.7), seeds 0..9\n" + f"largest_share {worst:.6f}\nlargest_err_on_passing_pixels {worst_err:.3e}\n"
            + "\n".join(lines) + "\n")
    print(text)
    try:
        if not os.path.exists(TOLERANCE_FILE) or open(TOLERANCE_FILE).read() != text:
            open(TOLERANCE_FILE, "w").write(text)
    except OSError:
        pass
    held = [ln for ln in open(TOLERANCE_FILE) if ln.startswith("largest_share")]
    assert held and float(held[0].split()[1]) == float(f"{worst:.6f}"), "profiles/plb_render_light_tolerance.txt does not hold the measured share"
