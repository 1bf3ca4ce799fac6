"""The cases on which the ud_pc_* kernels and their NumPy specification (tests/pc_twin.py) are held to the reference's own sampling /
grouping kernels, run on the CPU by oracle/ref_pc (built where the reference tree is present).

build_inputs() makes the inputs (seeded), run_reference() feeds them to a oracle.ref_pc.RefPc and returns what the reference wrote,
check_discriminating() asserts what gives each case its point.  tests/golden/make_pc_ref.py stores inputs and outputs in
tests/golden/pc_ref_cases.npz under "<case>.<array>"; load() reads them back as {case: {array: value}}.  The tests read the
fixture only, so they run where the reference is absent.

What the reference does not write: a ball-query row without a hit (it keeps SENT_I here; the contract writes zeros)."""
import os

import numpy as np

from tests import pc_twin as tw

F = np.float32
SENT_I = -77777
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pc_ref_cases.npz")
WIDTH = 512                     # threads per block of the reference's sampling launch: its tie order above 512 points is (k mod 512, k)

FPS_N = [1, 63, 65, 200, 257, 513, 1025, 3100]
FPS_M = {1: 3, 63: 20}          # every other cloud: 64
LATTICES = [4, 7, 9]            # 64, 343, 729 points
BALL = [(200, 32), (1500, 65), (200, 1)]
BOUNDARY_K = [6, 8, 10]
GROUP_C = [0, 1, 3, 131]
BWD = {"bwd_m300": dict(n=60, m=300, ns=4, C=2), "bwd_c131": dict(n=50, m=20, ns=4, C=131)}


def fps_cases():
    """name -> (kind, n) of every FPS case."""
    out = {f"fps_{kind}_{n}": (kind, n) for n in FPS_N for kind in ("random", "dup")}
    out["fps_b33"] = ("random", 65)
    out.update({f"fps_lattice_{s}": ("lattice", s ** 3) for s in LATTICES})
    out["chain"] = ("random", 200)
    return out


def tie_cases():
    """The FPS cases on which the contract does NOT promise the reference's indices: exact ties above 512 points."""
    return [f"fps_dup_{n}" for n in FPS_N if n > WIDTH] + ["fps_lattice_9"]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def build_inputs():
    cases = {}
    for n in FPS_N:
        B = 3 if n <= 513 else 2                           # two clouds on the largest: the fixture's size
        for kind in ("random", "dup"):
            rng = np.random.default_rng(1000 * n + len(kind))
            xyz = tw.random_cloud(rng, B, n) if kind == "random" else tw.duplicate_cloud(rng, B, n)
            cases[f"fps_{kind}_{n}"] = dict(xyz=xyz.astype(F), m=np.int32(FPS_M.get(n, 64)))
    cases["fps_b33"] = dict(xyz=tw.random_cloud(np.random.default_rng(33), 33, 65), m=np.int32(8))
    for s in LATTICES:
        cases[f"fps_lattice_{s}"] = dict(xyz=tw.lattice(s)[None], m=np.int32(64))
    # the model's own chain on one cloud: 512 of 200, ball 0.02 / 32, then 128 of those 512, ball 0.02 / 64
    cases["chain"] = dict(xyz=tw.random_cloud(np.random.default_rng(7), 1, 200), m=np.int32(512))
    for n, ns in BALL:
        xyz, new_xyz, _, _ = tw.ball_case(1, 2, n, 40, ns)
        cases[f"ball_{n}_{ns}"] = dict(xyz=xyz, new_xyz=new_xyz, radius=F(0.02), nsample=np.int32(ns))
    for k in BOUNDARY_K:
        xyz, centre, radius = tw.boundary_case(k)
        cases[f"boundary_{k}"] = dict(xyz=xyz, new_xyz=centre, radius=F(radius), nsample=np.int32(4))
    # group: the indices are ball_200_32's (run_reference fills them in).  C = 131 is 335 k gathered floats: its features are drawn
    # from two full-mantissa values so that the fixture compresses (a gather copies bits; what can go wrong is which element, and
    # 131 such draws tell any two rows and any two channel offsets apart), the narrow ones are normal draws
    rng = np.random.default_rng(50)
    alphabet = rng.normal(size=2).astype(F)
    group = {}
    for C in GROUP_C:
        if C:
            group[f"feats_{C}"] = alphabet[rng.integers(0, 2, (2, 200, C))] if C > 8 else rng.normal(size=(2, 200, C)).astype(F)
    cases["group"] = group
    # backward: cotangents = small integers times 2^-10, so every sum is exact in f32 whatever its order
    for name, s in BWD.items():
        rng = np.random.default_rng(len(name) + s["m"])
        idx = rng.integers(0, s["n"], (2, s["m"], s["ns"])).astype(np.int32)
        centre_idx = rng.integers(0, s["n"], (2, s["m"])).astype(np.int32)
        centre_idx[:, 1] = centre_idx[:, 0]
        g = (rng.integers(-8, 9, (2, s["m"], s["ns"], 3 + s["C"])) * 2.0 ** -10).astype(F)
        cases[name] = dict(idx=idx, centre_idx=centre_idx, g_out=g, n=np.int32(s["n"]))
    return cases


# ---- the reference's outputs ----------------------------------------------------------------------------------------------------------
def neg_sum_k(g_xyz_part):
    """-(sum over the sample axis), float32, k ascending from +0: the cotangent of the centres."""
    s = np.zeros(g_xyz_part.shape[:2] + (3,), F)
    for k in range(g_xyz_part.shape[2]):
        s = (s + g_xyz_part[:, :, k]).astype(F)
    return -s


def run_reference(R, cases):
    """-> {case: {array: value}}: what the reference's kernels write for the inputs of `cases` (R: oracle.ref_pc.RefPc)."""
    out = {}
    for name in fps_cases():
        c = cases[name]
        idx = R.fps(c["xyz"], int(c["m"]))
        out[name] = dict(idx=idx, new_xyz=R.gather(c["xyz"], idx))
    c, o = cases["chain"], out["chain"]
    o["i1"], o["cnt1"] = R.ball_query(0.02, 32, c["xyz"], o["new_xyz"])
    o["c2"] = R.fps(o["new_xyz"], 128)
    o["x2"] = R.gather(o["new_xyz"], o["c2"])
    o["i2"], o["cnt2"] = R.ball_query(0.02, 64, o["new_xyz"], o["x2"])
    for name, c in cases.items():
        if name.startswith("ball_") or name.startswith("boundary_"):
            idx, cnt = R.ball_query(float(c["radius"]), int(c["nsample"]), c["xyz"], c["new_xyz"])
            out[name] = dict(idx=idx, cnt=cnt)
    b = cases["ball_200_32"]
    idx = np.where(out["ball_200_32"]["cnt"][:, :, None] > 0, out["ball_200_32"]["idx"], 0).astype(np.int32)
    o = out["group"] = dict(idx=idx, grouped_xyz=R.group(b["xyz"], idx))      # idx: rows the reference left unwritten -> the contract's zeros
    for key, feats in cases["group"].items():
        o["grouped_" + key] = R.group(feats, idx)
    for name in BWD:
        c = cases[name]
        n, g = int(c["n"]), c["g_out"]
        plain = R.group_grad(n, c["idx"], np.ascontiguousarray(g[..., :3]))
        centre = R.scatter_add(n, c["centre_idx"], neg_sum_k(g[..., :3]))
        out[name] = dict(g_xyz_plain=plain, g_xyz_centred=(plain + centre).astype(F),
                         g_feats=R.group_grad(n, c["idx"], np.ascontiguousarray(g[..., 3:])))
    return out


# ---- FPS: following an index sequence ---------------------------------------------------------------------------------------------------
def fps_maxima(xyz_b, seq):
    """For one cloud [n,3] and an index sequence: per sample j >= 1 the (mind, indices of its maxima) the contract's recurrence has
    when sample j is chosen, given that seq[:j] was chosen before."""
    mind = np.full(len(xyz_b), F(1e38), F)
    for j in range(1, len(seq)):
        mind = np.minimum(mind, tw._d2(xyz_b, xyz_b[seq[j - 1]]))
        yield j, mind, np.nonzero(mind == mind.max())[0]


def lowest(maxima):
    return int(maxima.min())


def reference_order(maxima):
    """The reference's pick among tied maxima: each of its 512 threads keeps the lowest index of its own points k = t, t + 512, ..,
    and the tree reduction keeps the lower thread: the minimum of (k mod 512, k)."""
    return int(min(maxima, key=lambda k: (k % WIDTH, k)))


def first_parting(a, b):
    d = np.nonzero(np.asarray(a) != np.asarray(b))[0]
    return int(d[0]) if len(d) else None


def check_tie_deviation(name, xyz, got_idx, got_new, ref_idx, ref_new):
    """The documented deviation on the tie cases (include/unidom_hip.h, ud_pc_fps), for `got` = the twin's or the kernel's result.
    Per cloud, at the first sample where got and the reference part ways: both candidates hold the same mind bits, got's is the
    lowest index among the maxima, the reference's the minimum of (k mod 512, k).  Duplicate clouds: the parted picks are the same
    point, so the rule is checked at EVERY sample and new_xyz is bit-equal throughout.  The 729-point lattice: the picks differ as
    points.  Returns the number of differing indices."""
    u32 = lambda a: np.ascontiguousarray(a, F).view(np.uint32)
    differing = int((got_idx != ref_idx).sum())
    assert differing > 0, name
    for b in range(len(xyz)):
        j0 = first_parting(got_idx[b], ref_idx[b])
        if j0 is None:
            continue
        for j, mind, maxima in fps_maxima(xyz[b], ref_idx[b]):
            if j < j0:
                continue
            g, r = int(got_idx[b, j]), int(ref_idx[b, j])
            assert u32(mind[g]) == u32(mind[r]) == u32(mind.max()), (name, b, j)
            assert g == lowest(maxima) and r == reference_order(maxima), (name, b, j, g, r)
            if "lattice" in name:
                break                                          # from here on the two follow different point sets
            assert np.array_equal(u32(xyz[b, g]), u32(xyz[b, r])), (name, b, j)
    if "lattice" in name:
        assert not np.array_equal(u32(got_new), u32(ref_new)), name
    else:
        assert np.array_equal(u32(got_new), u32(ref_new)), name
    return differing


# ---- what makes each case worth keeping ------------------------------------------------------------------------------------------------
def check_discriminating(cases, ref):
    for name, (kind, n) in fps_cases().items():
        xyz, idx = cases[name]["xyz"], ref[name]["idx"]
        assert xyz.shape[1] == n and idx.shape == (len(xyz), int(cases[name]["m"])), name
        if kind == "dup" and n > 2:
            assert all(len(np.unique(x, axis=0)) < n for x in xyz), name
            if n <= WIDTH:                                         # a tie is met while sampling and both rules agree on it
                assert any(len(mx) > 1 and mind.max() > 0 for x, s in zip(xyz, idx) for _, mind, mx in fps_maxima(x, s)), name
    assert len(cases["fps_b33"]["xyz"]) > 32                       # a block of the reference takes a second cloud
    assert cases["fps_random_3100"]["xyz"].shape[1] > 3072         # past the reference's shared-memory copy of the cloud
    assert int(cases["chain"]["m"]) > cases["chain"]["xyz"].shape[1]
    got = ref["chain"]["idx"][0]
    assert sorted(got[:200].tolist()) == list(range(200)) and (got[200:] == 0).all()
    for name in tie_cases():                                       # the reference parts from the lowest-index rule here
        ti, tn = tw.fps(cases[name]["xyz"], int(cases[name]["m"]))
        check_tie_deviation(name, cases[name]["xyz"], ti, tn, ref[name]["idx"], ref[name]["new_xyz"])
    for n, ns in BALL:
        c, r = cases[f"ball_{n}_{ns}"], ref[f"ball_{n}_{ns}"]
        hist = np.bincount(r["cnt"].reshape(-1), minlength=ns + 1)
        assert hist[0] > 0 and hist[ns] > 0 and (ns == 1 or hist[1:ns].sum() > 0), (n, ns, hist)
        assert (r["idx"][r["cnt"] == 0] == SENT_I).all()
        p, s = tw.sqrt_disagreement(0, 0.02)                       # the planted point: s < r r holds, sqrtf(s) < r does not
        far = max(1, 40 // 8)
        assert np.array_equal(c["xyz"][0, n // 2], p) and not c["new_xyz"][0, far].any() and s < F(0.02) * F(0.02)
        assert n // 2 not in r["idx"][0, far].tolist()
    for k in BOUNDARY_K:
        r = ref[f"boundary_{k}"]
        assert r["cnt"].tolist() == [[1]] and r["idx"][0, 0].tolist() == [3, 3, 3, 3]
    g = ref["group"]
    assert g["idx"].min() >= 0 and g["idx"].max() < 200 and any((row == row[0]).all() for row in g["idx"][0])
    for name, s in BWD.items():
        c = cases[name]
        assert all(len(np.unique(ci)) < len(ci) for ci in c["centre_idx"]) and (c["centre_idx"][:, 0] == c["centre_idx"][:, 1]).all()
        assert not np.array_equal(ref[name]["g_xyz_plain"], ref[name]["g_xyz_centred"])
        q = c["g_out"].astype(np.float64) * 1024
        assert np.array_equal(q, np.round(q)) and np.abs(q).sum() < 2 ** 24      # dyadic, and no partial sum can leave f32's integers
    assert BWD["bwd_m300"]["m"] > 256                              # more centres than the reference's threads per block


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
def flatten(cases, ref):
    flat = {}
    for src in (cases, ref):
        for name, arrays in src.items():
            for key, value in arrays.items():
                assert f"{name}.{key}" not in flat
                flat[f"{name}.{key}"] = np.asarray(value)
    return flat


_LOADED = None


def load():
    """{case: {array: value}} of the committed fixture, inputs and reference outputs together; read once, read-only."""
    global _LOADED
    if _LOADED is None:
        _LOADED = {}
        with np.load(FIXTURE) as z:
            for full in z.files:
                name, key = full.split(".")
                a = z[full]
                a.setflags(write=False)
                _LOADED.setdefault(name, {})[key] = a
    return _LOADED


# ---- checks shared by the CPU tests (the twin) and the GPU tests (the kernels) -----------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


def check_ball(idx, cnt, c):
    """cnt everywhere, idx on the rows with a hit, zeros where the reference wrote nothing (its buffer kept the sentinel)."""
    hit = c["cnt"] > 0
    assert same(cnt, c["cnt"])
    assert np.array_equal(idx[hit], c["idx"][hit])
    assert (idx[~hit] == 0).all() and (c["idx"][~hit] == SENT_I).all()


def group_expected(C):
    """(xyz, feats, new_xyz, idx, out): the reference's two gathers, the centre subtracted from the first (one float32 subtraction, as
    pnet2_layers does after the op), the features behind it."""
    fx = load()
    b, g = fx["ball_200_32"], fx["group"]
    out = (g["grouped_xyz"] - b["new_xyz"][:, :, None, :]).astype(F)
    if C:
        out = np.concatenate([out, g[f"grouped_feats_{C}"]], -1)
    return b["xyz"], (g[f"feats_{C}"] if C else None), b["new_xyz"], g["idx"], out


def check_group_bwd(c, plain, centred):
    """plain / centred: (g_xyz, g_feats, g_new_xyz) without / with centre_idx."""
    g_new = neg_sum_k(c["g_out"][..., :3])
    assert same(plain[0], c["g_xyz_plain"]) and same(centred[0], c["g_xyz_centred"])
    for got in (plain, centred):
        assert same(got[1], c["g_feats"]) and same(got[2], g_new)
