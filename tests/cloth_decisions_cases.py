"""Shared by tests/test_cloth_decisions_gpu.py and tests/test_cloth_decisions_cases.py (a plain module, no fixtures): the decision words
the cloth forward call leaves behind its checkpoint records for the one-workgroup fast adjoint (csrc/cloth_common.h: one 32-bit word per
env, substep and padded particle), restated in NumPy float32 -- operation by operation in the order of grip_own, clip_grad_01 and
cloth_decisions_kernel (csrc/cloth_fast_adj.h, csrc/cloth_fast_bwd.hip), no fused multiply-add -- and the inputs both tests run.

    bits  0-7, 8-15, 16-23   2 * clip_grad_01(x2[d]):  0 outside [0, 1], 1 on a bound, 2 inside
    bits 24-26               |v of the next record| < max_v
    bit  27, 28              held by gripper 0, gripper 1
    bits 29-30               lanes 0-7: 2 * clip_grad_01(primitive component + its move)   (lanes 3 and 7: the radii, which do not move)
    padding lanes (i >= P): 0 in every particle field

Bodies: 1, 63, 65 particles (tests/test_cloth_adjoint_f64_gpu.py), 257 and 449 (tests/cloth_bwd_ragged_cases.py), 512 (fold_cloth1's).
Every case has B = 2 envs and is built so that the words take every value they can (asserted on the CPU oracle alone by
tests/test_cloth_decisions_cases.py):
    env 0: gripper 0 sits on a particle that lies on the ground (every seventh does) and pushes it DOWN with partial suction, so the held
           particle's displaced position leaves [0, 1] (factor 0) while its neighbours on the ground sit exactly on the bound (0.5);
           gripper 1 sits on a particle of the first wave with a move of its own (held in some waves only, where there are several);
           one particle starts at five times max_v, so the velocity clip is active behind the first substep.
    env 1: gripper 1 stays at the corner (1, 1, 1) and is pushed outwards along x: its x component leaves the cube (code 0), y and z sit
           on the bound (1), the radii and all of env 0's components are inside (2).
    variant "r0big": gripper 0's input radius is 1.25 and it floats 1.1 above its particle: the first substep's threshold (the radius
           as given) holds what every later one (the radius clipped to 1, the position clipped into the cube) decides on its own."""
import zlib

import numpy as np

import cloth_adjoint_bar as cab

B = 2
S_GRID, T_GRID = (1, 2, 3), (1, 2)
DV, M0, M1, PRIM = 24, 27, 28, 29
_IN = {}
f32 = np.float32


def _bodies():
    from cloth_bwd_ragged_cases import BODIES as RAGGED
    from test_cloth_adjoint_f64_gpu import BODIES as SMALL
    out = {name: (SMALL[name][0], SMALL[name][2]) for name in ("one_particle", "rect7x9", "rect5x13", "patch16x32")}
    out.update({name: (RAGGED[name][0], RAGGED[name][1]) for name in ("p257", "p449")})
    return out


BODY_NAMES = ("one_particle", "rect7x9", "rect5x13", "p257", "p449", "patch16x32")     # 1, 63, 65, 257, 449, 512 particles


def inputs(body, S, T, variant=""):
    """-> (conf, mask, P, [x, v, prim, k, mu, actions]); the same arrays whenever it is asked again"""
    key = (body, S, T, variant)
    if key not in _IN:
        make, P = _bodies()[body]
        mask = make()
        assert int(mask.sum()) == P
        conf = cab.make_conf(substeps=S)
        rng = np.random.default_rng(zlib.crc32(f"decisions/{body}/S{S}/T{T}".encode()))
        x, v, prim, k, mu, actions = cab.make_case(rng, conf, mask, B, T)
        x[:, ::7, 1] = 0
        p0 = 7 * int(rng.integers(0, -(-P // 7)))          # a particle on the ground
        prim[0, 0, :3] = x[0, p0] + f32([0, 0.002, 0])
        actions[:, 0, 1] = -1.0                             # pushed down: the held particle's x2 leaves the cube
        actions[:, 0, 3] = 0.25
        p1 = (p0 + 5) % min(P, 64)                          # in the first wave, cells away from p0: gripper 0 does not carry it off
        prim[0, 1, :3] = x[0, p1] + f32([0, 0.002, 0])
        actions[:, 0, 4:7] = (rng.normal(size=(T, 3)) * 0.3).astype(f32)
        actions[:, 0, 7] = rng.uniform(0.2, 0.8, size=T).astype(f32)
        actions[:, 1, 4] = 1.0                              # env 1: gripper 1 leaves the cube through x = 1
        v[0, P // 2, 0] = f32(5) * f32(conf.max_v)
        if variant == "r0big":
            prim[:, 0, 1] += f32(1.1)
            prim[:, 0, 3] = f32(1.25)
        else:
            assert variant == ""
        _IN[key] = (conf, mask, P, [x, v, prim, k, mu, actions])
    return _IN[key]


# -- the restatement -------------------------------------------------------------------------------------------------------------
def grasp_thr(r):
    """the largest float32 whose correctly rounded square root is <= r (csrc/cloth_common.h); np.sqrt of a float32 is correctly rounded"""
    r = f32(r)
    if not r >= 0:
        return f32(-1)
    if np.isinf(r):
        return r
    t = np.uint32((r * r).view(np.uint32))
    bits = lambda u: np.uint32(u).view(f32)
    for _ in range(4):
        if np.sqrt(bits(t)) > r:
            t = np.uint32(t - 1)
    for _ in range(4):
        if np.sqrt(bits(t + 1)) <= r:
            t = np.uint32(t + 1)
    assert np.sqrt(bits(t)) <= r and not np.sqrt(bits(t + 1)) <= r
    return bits(t)


def _clipf(x, lo, hi):
    return np.minimum(f32(hi), np.maximum(f32(lo), x))


def _code01(x):
    """2 * clip_grad_01(x) from the sign of x (1 - x)"""
    p = x * (f32(1) - x)
    return np.where(p > 0, 2, np.where(p == 0, 1, 0)).astype(np.uint32)


def decision_words(x, v_next, prim, actions, S, Pp, max_v):
    """x, v_next [B, T S, P, 3] (positions of every substep's input record, velocities of the record AFTER it), prim [B, T S, 2, 4]
    (primitives of every substep's input record), actions [T, B, 8]  ->  uint32 [B, T S, Pp]"""
    x, v_next, prim, actions = (np.asarray(a, f32) for a in (x, v_next, prim, actions))
    nB, n, P = x.shape[:3]
    T = actions.shape[0]
    assert n == T * S and P <= Pp
    fifty = f32(1) / f32(50)
    a8 = np.repeat(np.moveaxis(actions, 0, 1), S, axis=1)                    # [B, T S, 8]: the macro action of every substep
    act = a8.copy()
    for g in (0, 4):
        act[..., g:g + 3] = _clipf(a8[..., g:g + 3], -2, 2) * fifty
    thr = np.empty((nB, n, 2), f32)                                          # per gripper: record 0's radius as given, then clipped
    for b in range(nB):
        for g in range(2):
            r0 = prim[b, 0, g, 3]
            thr[b, :, g] = grasp_thr(_clipf(r0 + f32(0), 0, 1))
            thr[b, 0, g] = grasp_thr(r0)
    with np.errstate(all="ignore"):
        cur, held = x, []
        for g in range(2):
            d = cur - prim[:, :, None, g, :3]
            s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            m = s <= thr[:, :, None, g]
            move = act[..., 4 * g:4 * g + 3] * (f32(1) - act[..., 4 * g + 3])[..., None]
            cur = np.where(m[..., None], cur + move[:, :, None, :], cur)
            held.append(m)
        assert cur.dtype == f32 and s.dtype == f32
        w = np.zeros((nB, n, Pp), np.uint32)
        for d in range(3):
            w[..., :P] |= _code01(cur[..., d]) << np.uint32(8 * d)
            w[..., :P] |= (np.abs(v_next[..., d]) < f32(max_v)).astype(np.uint32) << np.uint32(DV + d)
        w[..., :P] |= held[0].astype(np.uint32) << np.uint32(M0)
        w[..., :P] |= held[1].astype(np.uint32) << np.uint32(M1)
        comp = prim.reshape(nB, n, 8)
        moves = np.array([q & 3 < 3 for q in range(8)])
        addl = np.where(moves, _clipf(a8, -2, 2) * fifty, f32(0))
        w[..., :8] |= _code01(comp + addl) << np.uint32(PRIM)
    return w


def fields(w):
    """-> dict of the word's fields"""
    w = np.asarray(w, np.uint32)
    return dict(dx=np.stack([(w >> np.uint32(8 * d)) & np.uint32(0xFF) for d in range(3)], -1),
                dv=np.stack([(w >> np.uint32(DV + d)) & np.uint32(1) for d in range(3)], -1),
                m0=(w >> np.uint32(M0)) & np.uint32(1), m1=(w >> np.uint32(M1)) & np.uint32(1), prim=(w >> np.uint32(PRIM)) & np.uint32(3))


def oracle_words(body, S, T, variant=""):
    """the words of the case from the order-2 CPU oracle's forward alone -> (words [B, T S, Pp], grasp sets [T S, B, 2, P])"""
    conf, mask, P, case = inputs(body, S, T, variant)
    fwd = cab.make_oracle(conf, mask, 2).rollout_fwd(*case, want_lists=True, want_grasp=True, want_ckpt=True, nthreads=cab.NTHREADS)
    ck = fwd["ckpt"].reshape(B, T * S, 6 * P + 8)
    x = ck[..., :3 * P].reshape(B, T * S, P, 3)
    v = ck[..., 3 * P:6 * P].reshape(B, T * S, P, 3)
    v_next = np.concatenate([v[:, 1:], fwd["v"][:, None]], 1)
    w = decision_words(x, v_next, ck[..., 6 * P:].reshape(B, T * S, 2, 4), case[5], S, -(-P // 64) * 64, conf.max_v)
    return w, np.asarray(fwd["grasp"]).reshape(T * S, B, 2, P) != 0
