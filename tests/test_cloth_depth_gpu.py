"""GPU: the cloth DEPTH observation (csrc/env_depth.hip: ud_cloth_depth_fwd / _bwd, _fused.depth, ClothEnv.get_obs(DEPTH)).

The checker is depth_twin below, a NumPy restatement of the reference's state_to_depth (cloth_env.py:71-92) applied to every
image: a stable argsort on h, f32 true division, float clip, nan_to_num(nan=0), integer conversion, fancy assignment (the last
duplicate wins).  The kernels only select values and do one add, so images, owner and gradients are compared exactly; output
buffers are filled with NaN (owner with a marker) before every call, so anything left unwritten shows."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, cloth_reset_x

pytestmark = pytest.mark.gpu

PS, ZO = np.float32(0.003125), np.float32(0.01)
UD_ERR_INVALID, UD_ERR_UNSUPPORTED = -1, -2
MARK = -12345   # owner pre-fill


def depth_twin(x, H=320, W=320, pixel_size=PS, z_offset=ZO):
    """x [M,P,3] f32 -> (img [M,H,W] f32, owner [M,P] i32): owner[m,p] = py*W + px if p owns its pixel, else -1."""
    x = np.asarray(x, np.float32)
    M, P = x.shape[:2]
    pixel_size, z_offset = np.float32(pixel_size), np.float32(z_offset)
    img = np.zeros((M, H, W), np.float32)
    owner = np.full((M, P), -1, np.int32)
    with np.errstate(all="ignore"):
        for m in range(M):
            h = x[m, :, 1] + z_offset
            iz = np.argsort(h, kind="stable")                      # NaN last, ties in index order
            px = np.nan_to_num(np.clip(np.floor(x[m, :, 0] / pixel_size), 0, W - 1), nan=0).astype(np.int64)
            py = np.nan_to_num(np.clip(np.floor(x[m, :, 2] / pixel_size), 0, H - 1), nan=0).astype(np.int64)
            img[m][py[iz], px[iz]] = h[iz]                         # last duplicate wins
            last = {}
            for p in iz:
                last[int(py[p] * W + px[p])] = int(p)
            for pix, p in last.items():
                owner[m, p] = pix
    return img, owner


def twin_bwd(owner, g_img):
    M, P = owner.shape
    gx = np.zeros((M, P, 3), np.float32)
    flat = g_img.reshape(M, -1)
    for m in range(M):
        own = owner[m] >= 0
        gx[m, own, 1] = flat[m, owner[m, own]]
    return gx


# ---- ABI through ctypes ----------------------------------------------------------------------------
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def hip_fwd(x, H=320, W=320, pixel_size=PS, z_offset=ZO, bufs=None, want_owner=True):
    from unidom_amd import _lib
    M, P = x.shape[:2]
    xd = torch.tensor(x, device="cuda")
    if bufs is None:
        bufs = (torch.empty((M, H, W), dtype=torch.float32, device="cuda"), torch.empty((M, P), dtype=torch.int32, device="cuda"))
    img, owner = bufs
    img.fill_(float("nan"))
    owner.fill_(MARK)
    rc = _lib.lib().ud_cloth_depth_fwd(M, P, H, W, float(pixel_size), float(z_offset), _lib.ptr(xd), _lib.ptr(img),
                                       _lib.ptr(owner if want_owner else None), _stream())
    torch.cuda.synchronize()
    return rc, img.cpu().numpy(), owner.cpu().numpy()


def hip_bwd(owner, g_img, H=320, W=320):
    from unidom_amd import _lib
    M, P = owner.shape
    od, gd = torch.tensor(owner, device="cuda"), torch.tensor(g_img, device="cuda")
    gx = torch.full((M, P, 3), float("nan"), dtype=torch.float32, device="cuda")
    rc = _lib.lib().ud_cloth_depth_bwd(M, P, H, W, _lib.ptr(od), _lib.ptr(gd), _lib.ptr(gx), _stream())
    torch.cuda.synchronize()
    return rc, gx.cpu().numpy()


def _uniform_case(rng, M, P):
    x = rng.uniform(-0.05, 1.05, size=(M, P, 3)).astype(np.float32)       # both clips fire
    x[..., 1] = rng.uniform(-0.05, 0.2, size=(M, P)).astype(np.float32)   # negative heights too
    return x


def _contention_case():
    """fold_cloth1 rest lattice (16 x 32) mirrored onto itself about its mid-line, the upper layer 0.004 higher: every occupied
    pixel is contested by exactly two particles.  The four images differ in which half lies on top and in a lattice-aligned shift."""
    x0 = cloth_reset_x()                         # rows ii = 32..47, columns jj = 32..63, p = 32 * (ii - 32) + (jj - 32)
    ii, jj = np.divmod(np.arange(512), 32)
    partner = ii * 32 + (31 - jj)                # jj' = 95 - jj
    out = []
    for m in range(4):
        x = x0.copy()
        moved = jj >= 16 if m % 2 == 0 else jj < 16
        x[moved] = x0[partner[moved]]
        x[moved, 1] = np.float32(0.004)
        x[:, 0] += np.float32(0.0125 * m)
        out.append(x)
    return np.stack(out).astype(np.float32)


def _tshirt_case(rng):
    mask = np.load(os.path.join(ROOT, "unidom_amd", "envs", "others", "tshirt_mask.npy"))
    x0 = cloth_reset_x(180, mask)
    assert x0.shape == (3573, 3)
    return (x0[None] + rng.normal(size=(2, 3573, 3)) * 1e-3).astype(np.float32)


def _one_pixel_case(rng):
    """4096 particles in one pixel; the 2048 at random positions that share the top height tie: the highest index wins."""
    x = np.empty((1, 4096, 3), np.float32)
    x[..., 0] = np.float32(0.5005) + rng.uniform(0, 1e-3, size=4096).astype(np.float32)
    x[..., 2] = np.float32(0.3005) + rng.uniform(0, 1e-3, size=4096).astype(np.float32)
    h = rng.uniform(0.0, 0.04, size=4096).astype(np.float32)
    h[rng.permutation(4096)[:2048]] = np.float32(0.05)
    x[0, :, 1] = h
    return x


def _edges_case(rng):
    """The 321 pixel edges k * pixel_size and their f32 neighbours on either side, once along x and once along z."""
    k = np.arange(321, dtype=np.float32) * PS
    e = np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2))]).astype(np.float32)
    assert e.shape == (963,)
    other = ((np.arange(963) % 320 + np.float32(0.5)) * PS).astype(np.float32)
    h = rng.uniform(0, 0.1, size=963).astype(np.float32)
    a = np.stack([e, h, other], -1)
    b = np.stack([other, h, e], -1)
    return np.stack([a, b]).astype(np.float32)


def _nonfinite_case():
    """NaN, +inf and -inf in each coordinate, every such particle with one finite competitor in the pixel it lands in; and a NaN
    height among finite ones.  The second image holds the same particles in reverse order."""
    nan, inf = np.float32("nan"), np.float32("inf")
    rows = []
    for i, bad in enumerate((nan, inf, -inf)):
        z = np.float32(0.1 + 0.1 * i)
        px_land = np.float32(0.9999) if bad == inf else np.float32(0.0001)
        rows += [(bad, 0.05, z), (px_land, 0.02 + 0.02 * i, z)]           # bad x: column 0 or the last one
        xx = np.float32(0.5 + 0.1 * i)
        rows += [(xx, 0.05, bad), (xx, 0.08 - 0.02 * i, px_land)]         # bad z: row 0 or the last one
        rows += [(xx, bad, 0.5), (xx, 0.03, 0.5)]                         # bad height against a finite one
    rows += [(0.25, 0.01, 0.25), (0.25, nan, 0.25), (0.25, 0.07, 0.25), (0.25, inf, 0.25)]   # NaN above finite and +inf
    rows += [(nan, nan, nan), (0.0, 0.0, 0.0)]                            # all-NaN particle in pixel 0 against a finite one
    a = np.array(rows, np.float32)
    return np.stack([a, a[::-1]]).astype(np.float32)


def _nonsquare_case(rng):
    return _uniform_case(rng, 2, 100)


_DIMS = {"nonsquare": (8, 16, np.float32(1 / 16))}


@functools.lru_cache(maxsize=None)
def case(name):
    """(x, H, W, pixel_size, twin img, twin owner): built once and shared; nobody writes to the arrays."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("P"):
        P = int(name[1:])
        x = _uniform_case(rng, 1 if P == 1 else 3, P)
    else:
        x = {"contention": _contention_case, "tshirt": lambda: _tshirt_case(rng), "one_pixel": lambda: _one_pixel_case(rng),
             "edges": lambda: _edges_case(rng), "nonfinite": _nonfinite_case, "nonsquare": lambda: _nonsquare_case(rng)}[name]()
    H, W, ps = _DIMS.get(name, (320, 320, PS))
    img, owner = depth_twin(x, H, W, ps)
    for a in (x, img, owner):
        a.setflags(write=False)
    return x, H, W, ps, img, owner


SWEEP = ["P1", "P63", "P64", "P65", "P513", "P1024", "P1025"]
FWD_CASES = SWEEP + ["contention", "tshirt", "one_pixel", "edges", "nonfinite", "nonsquare"]
BWD_CASES = SWEEP + ["contention", "tshirt", "one_pixel", "nonfinite"]


@pytest.mark.parametrize("name", FWD_CASES)
def test_depth_forward_equals_the_twin(name):
    x, H, W, ps, img, owner = case(name)
    if name == "contention":   # every occupied pixel is contested, and the upper layer wins
        assert (owner >= 0).sum() == 4 * 256 and np.all(img[img != 0] == np.float32(0.004) + ZO)
    if name == "one_pixel":
        assert (owner >= 0).sum() == 1 and owner[0].argmax() == np.nonzero(x[0, :, 1] == np.float32(0.05))[0].max()
    rc, got_img, got_owner = hip_fwd(x, H, W, ps)
    assert rc == 0
    np.testing.assert_array_equal(got_img, img)
    np.testing.assert_array_equal(got_owner, owner)
    rc, got_img, got_owner = hip_fwd(x, H, W, ps, want_owner=False)   # owner may be NULL
    assert rc == 0
    np.testing.assert_array_equal(got_img, img)
    assert np.all(got_owner == MARK)


def test_true_division_differs_from_a_multiplication_at_the_edges():
    """The edge case tells x / pixel_size from x * 320: the twin itself must see the difference, or the case checks nothing."""
    x = case("edges")[0]
    with np.errstate(all="ignore"):
        assert np.any(np.floor(x[0, :, 0] / PS) != np.floor(x[0, :, 0] * np.float32(320)))


@pytest.mark.parametrize("name", BWD_CASES)
def test_depth_backward_equals_the_twin_and_owner_is_reproducible(name):
    x, H, W, ps, img, owner = case(name)
    rc1, _, o1 = hip_fwd(x, H, W, ps)
    rc2, _, o2 = hip_fwd(x, H, W, ps)
    assert rc1 == 0 and rc2 == 0
    np.testing.assert_array_equal(o1, o2)
    np.testing.assert_array_equal(o1, owner)
    g_img = np.random.default_rng(7).normal(size=img.shape).astype(np.float32)
    rc, gx = hip_bwd(o1, g_img, H, W)
    assert rc == 0
    np.testing.assert_array_equal(gx, twin_bwd(owner, g_img))
    assert np.all(gx[..., 0] == 0) and np.all(gx[..., 2] == 0)


def test_depth_buffers_can_be_reused():
    xa, xb = case("P513")[0], _uniform_case(np.random.default_rng(99), 3, 513)
    bufs = (torch.empty((3, 320, 320), dtype=torch.float32, device="cuda"), torch.empty((3, 513), dtype=torch.int32, device="cuda"))
    from unidom_amd import _lib
    for x in (xa, xb):   # the second call meets the first one's image and owners, not a NaN fill
        xd = torch.tensor(x, device="cuda")
        assert _lib.lib().ud_cloth_depth_fwd(3, 513, 320, 320, float(PS), float(ZO), _lib.ptr(xd), _lib.ptr(bufs[0]), _lib.ptr(bufs[1]),
                                             _stream()) == 0
    torch.cuda.synchronize()
    img, owner = depth_twin(xb)
    np.testing.assert_array_equal(bufs[0].cpu().numpy(), img)
    np.testing.assert_array_equal(bufs[1].cpu().numpy(), owner)


def test_depth_refuses_what_it_does_not_cover():
    from unidom_amd import _lib
    rng = np.random.default_rng(3)
    rc, img, owner = hip_fwd(_uniform_case(rng, 1, 4097))
    assert rc == UD_ERR_UNSUPPORTED and b"4097" in _lib.lib().ud_last_error()
    assert np.isnan(img).all() and np.all(owner == MARK)
    rc, img, owner = hip_fwd(_uniform_case(rng, 1, 8), H=1, W=131073)
    assert rc == UD_ERR_UNSUPPORTED and b"131073" in _lib.lib().ud_last_error()
    assert np.isnan(img).all() and np.all(owner == MARK)
    rc, gx = hip_bwd(np.zeros((1, 4097), np.int32), np.zeros((1, 320, 320), np.float32))
    assert rc == UD_ERR_UNSUPPORTED and np.isnan(gx).all()
    rc, gx = hip_bwd(np.zeros((1, 8), np.int32), np.zeros((1, 1, 131073), np.float32), H=1, W=131073)
    assert rc == UD_ERR_UNSUPPORTED and np.isnan(gx).all()
    # null pointers and sizes below 1
    L, t = _lib.lib(), torch.zeros(64, device="cuda")
    p, null = _lib.ptr(t), C.c_void_p(0)
    assert L.ud_cloth_depth_fwd(1, 1, 4, 4, float(PS), float(ZO), null, p, null, _stream()) == UD_ERR_INVALID
    assert L.ud_cloth_depth_fwd(1, 1, 4, 4, float(PS), float(ZO), p, null, null, _stream()) == UD_ERR_INVALID
    assert L.ud_cloth_depth_fwd(0, 1, 4, 4, float(PS), float(ZO), p, p, null, _stream()) == UD_ERR_INVALID
    assert L.ud_cloth_depth_fwd(1, 0, 4, 4, float(PS), float(ZO), p, p, null, _stream()) == UD_ERR_INVALID
    assert L.ud_cloth_depth_fwd(1, 1, 0, 4, float(PS), float(ZO), p, p, null, _stream()) == UD_ERR_INVALID
    assert L.ud_cloth_depth_bwd(1, 1, 4, 4, null, p, p, _stream()) == UD_ERR_INVALID
    assert L.ud_cloth_depth_bwd(1, 1, 4, 0, p, p, p, _stream()) == UD_ERR_INVALID
    torch.cuda.synchronize()
    assert np.all(t.cpu().numpy() == 0)


# ---- env level ---------------------------------------------------------------------------------------
def _check_env_depth(env, B, P):
    from unidom_amd.envs.basic.cloth_env import ClothEnv
    _, state = env.reset(np.array([0, 1], np.uint32))
    assert state.x.shape == (B, P, 3)
    obs = env.get_obs(state, obs_type=ClothEnv.DEPTH)
    assert obs.shape == (B, 320, 320, 1) and obs.dtype == torch.float32
    img, _ = depth_twin(state.x.cpu().numpy())
    np.testing.assert_array_equal(obs.cpu().numpy()[..., 0], img)
    assert (img != 0).any()
    d0 = env.state_to_depth(state)
    assert isinstance(d0, np.ndarray) and d0.shape == (320, 320, 1)
    np.testing.assert_array_equal(d0[..., 0], img[0])
    with pytest.raises(NotImplementedError):
        env.get_obs(state, obs_type="RGB")
    with pytest.raises(NotImplementedError):
        env.get_obs(state, obs_type="THERMAL")
    assert env.get_obs(state).shape == (B, env.observation_size)   # the default is still PARTICLE


def test_fold_cloth1_depth_observation():
    from unidom_amd.envs.fold_cloth1_env import FoldCloth1Env
    _check_env_depth(FoldCloth1Env(2), 2, 512)


def test_fold_tshirt_depth_observation():
    from unidom_amd.envs.fold_cloth_tshirt_env import FoldTshirtEnv
    _check_env_depth(FoldTshirtEnv(1), 1, 3573)


def test_step_diff_with_depth_observations_is_opt_in_and_differentiable():
    from unidom_amd.envs.basic.cloth_env import ClothEnv
    from unidom_amd.envs.fold_cloth1_env import DefaultConf, FoldCloth1Env

    class DepthConf(DefaultConf):
        obs_type = ClothEnv.DEPTH
        substeps = 2

    env = FoldCloth1Env(2, conf=DepthConf())
    _, state = env.reset(np.array([0, 1], np.uint32))
    x0 = state.x[:, 200].detach()
    # gripper 0 starts on particle 200, so the grasp fires within the shortened substeps and the heights depend on the actions
    state = state._replace(primitive0=torch.cat([x0 + torch.tensor([0.0, 0.002, 0.0], device=x0.device), state.primitive0[:, 3:]], -1))
    # the pick lies beside the particle, not on it: at distance 0 the contact distance's own derivative is the reference's 0/0
    pick, place = x0 + torch.tensor([0.001, 0.0, 0.0005], device=x0.device), x0 + torch.tensor([0.1, 0.0, 0.05], device=x0.device)
    actions = torch.cat([pick, place], -1).requires_grad_(True)
    obs, reward, done, info = env.step_diff(actions, state)
    assert obs.shape == (2, 320, 320, 1) and info["obs_list"].shape == (40, 2, 320, 320, 1)
    xs, xl = info["state"].x, info["state_list"].x
    img, owner = depth_twin(xs.detach().cpu().numpy())
    np.testing.assert_array_equal(obs.detach().cpu().numpy()[..., 0], img)
    img_l, _ = depth_twin(xl.detach().cpu().numpy().reshape(80, 512, 3))
    np.testing.assert_array_equal(info["obs_list"].detach().cpu().numpy().reshape(80, 320, 320), img_l)
    seen = []
    xs.register_hook(seen.append)
    w = torch.tensor(np.random.default_rng(5).normal(size=(2, 320, 320, 1)).astype(np.float32), device=obs.device)
    (obs * w).sum().backward()
    g = actions.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().sum() > 0
    assert len(seen) == 1
    np.testing.assert_array_equal(seen[0].cpu().numpy(), twin_bwd(owner, w.cpu().numpy()[..., 0]))
