"""The Rope ("unfold cloth") branch of the reference's expert generator (GenORM/policy/pbm/plb/optimizer/solver.py:150-236, solve_action):
lift the sheet by `height` in window * steps actions, release it along one of twelve acceleration profiles, let it settle for `tail`
actions, render the final state from rope.yml's top-down camera and keep the acceleration whose image has the largest blue area.

The reference runs the twelve profiles one after the other in one env and renders twelve times; here they are the twelve envs of one
batch: one rollout, one PlbSimulator.render call, one blue_coverage call.

blue_coverage restates cv2.cvtColor(img, COLOR_RGB2HSV) + cv2.inRange(hsv, (120, 150, 150), (140, 255, 255)) + mask.sum() in torch on the
device.  cv2 is not available beside this package, so the rounding of its 8-bit HSV (a fixed-point table in OpenCV) is an UNPINNED reading: H and
S are formed in float32 by the documented formulas (V = max; S = 255 (V - min) / V; H = 60 (..) / (V - min) / 2, + 180 below zero) and rounded to
nearest.

Left out: tell_rope_break (:97-113, connected components of the pink mask).

    python -m unidom_amd.algorithms.plb_unfold --env rope [--window 30 --steps 16 --tail 100 --image_res 512 --spp 50]
"""
from __future__ import annotations

import argparse

import numpy as np
import torch

from ..engine.plb_render import render_conf_of
from ..engine.plb_simulator import PlbSimulator, RopeConf

ACXEL_LIST = (0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5, 0.55, 0.6, 0.65)    # solver.py:162
BLUE_LO, BLUE_HI = (120, 150, 150), (140, 255, 255)                                # :196-197
EXPERT_MASK_SUM = 9000000                                                          # :205


def release_actions(height=0.32, window=30, steps=16, tail=100, scale=0.005, acxel_list=ACXEL_LIST):
    """[T, len(acxel_list), 3] float64, T = 2 * window * steps + tail: solver.py:153-178 for every acceleration.  `steps` (the reference's 16)
    must be even: the rates are 1 -+ acxel * (0.5, 1, ..., steps / 4), without the middle."""
    assert steps % 2 == 0 and steps >= 2, steps
    unit_action = height / window / steps
    up = np.array([[0, unit_action / scale, 0]] * window * steps)
    half = steps // 2
    mult = [-(half - i) * 0.5 for i in range(half)] + [(i + 1) * 0.5 for i in range(half)]
    out = []
    for acxel in acxel_list:
        action_list = np.array([1 + acxel * m for m in mult]) * unit_action
        action_list = np.clip(action_list, 0, 1000000)
        action_list = np.repeat(action_list, window)
        action_list = action_list / scale
        down = np.array([[0, -i, 0] for i in action_list[::-1]])
        out.append(np.concatenate([up, down, np.array([[0, 0, 0]] * tail).reshape(tail, 3)]))
    return np.stack(out, axis=1)


def blue_coverage(img):
    """img: uint8 [..., H, W, 3] RGB (a torch tensor, any device) -> int64 [...]: the reference's mask.sum(), 255 per pixel inside the blue range."""
    rgb = img.to(torch.float32)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    v = rgb.amax(-1)
    diff = v - rgb.amin(-1)
    safe = torch.where(diff > 0, diff, torch.ones_like(diff))
    s = torch.where(v > 0, torch.round(255.0 * diff / torch.where(v > 0, v, torch.ones_like(v))), torch.zeros_like(v))
    h = torch.where(v == r, 60.0 * (g - b) / safe, torch.where(v == g, 120.0 + 60.0 * (b - r) / safe, 240.0 + 60.0 * (r - g) / safe))
    h = torch.where(diff > 0, h, torch.zeros_like(h))
    h = torch.where(h < 0, h + 360.0, h)
    h = torch.round(h / 2.0)
    h = torch.where(h >= 180.0, h - 180.0, h)
    inside = (h >= BLUE_LO[0]) & (h <= BLUE_HI[0]) & (s >= BLUE_LO[1]) & (s <= BLUE_HI[1]) & (v >= BLUE_LO[2]) & (v <= BLUE_HI[2])
    return inside.sum((-1, -2)).to(torch.int64) * 255


def unfold(conf=None, window=30, steps=16, tail=100, height=0.32, render_conf=None, spp=None, seed=0, E=None, nu=None, yield_stress=None,
           out=None, device="cuda", env_name="Rope-v1"):
    """Returns dict(coverage [12] int64, index, max_acxel, final PlbState, bf_state, image uint8 [12,H,W,3]); writes the reference's bc_data
    fields to `out` (.npz) when given."""
    conf = RopeConf() if conf is None else conf
    scale = float(conf.action_scale[1])
    acts = release_actions(height, window, steps, tail, scale)
    B = acts.shape[1]
    sim = PlbSimulator(conf, batch_size=B, device=device)
    state = sim.reset()
    if E is not None:                          # taichi_env.set_parameter
        state = state._replace(E=torch.full_like(state.E, float(E)))
    if nu is not None:
        state = state._replace(nu=torch.full_like(state.nu, float(nu)))
    if yield_stress is not None:
        state = state._replace(yield_stress=torch.full_like(state.yield_stress, float(yield_stress)))
    a = torch.tensor(acts, dtype=torch.float64, device=sim.device)
    bf_state = None
    with torch.no_grad():
        for i in range(a.shape[0]):
            state = sim.step(state, a[i])
            if i == window * steps - 1:
                bf_state = state.x.clone()
        sim.check_status()
        img = sim.render(state, spp=spp, seed=seed, mode="rgb_array", render_conf=render_conf)
        cov = blue_coverage(img)
    index = int(torch.argmax(cov))
    res = dict(coverage=cov.cpu().numpy(), index=index, max_acxel=ACXEL_LIST[index], state=state, bf_state=bf_state, image=img)
    if out is not None:
        np.savez(out, max_acxel=ACXEL_LIST[index], bf_state=bf_state[index].cpu().numpy(), E=float(state.E[0]), Poisson=float(state.nu[0]),
                 yield_stress=float(state.yield_stress[0]), env_name=env_name, height=height, window=window, steps=steps, scale=scale,
                 acxel_list=np.array(ACXEL_LIST), mask_sum_list=res["coverage"], is_expert=res["coverage"] > EXPERT_MASK_SUM)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--env", default="rope", choices=["rope"])
    ap.add_argument("--window", type=int, default=30)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--tail", type=int, default=100)
    ap.add_argument("--image_res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--E", type=float, default=None)
    ap.add_argument("--nu", type=float, default=None)
    ap.add_argument("--yield_stress", type=float, default=None)
    ap.add_argument("--out", default=None, help="write the reference's bc_data fields to this .npz")
    args = ap.parse_args(argv)
    conf = RopeConf()
    rc = render_conf_of(conf, image_res=(args.image_res, args.image_res), spp=args.spp)
    res = unfold(conf, args.window, args.steps, args.tail, render_conf=rc, seed=args.seed, E=args.E, nu=args.nu, yield_stress=args.yield_stress,
                 out=args.out)
    for acxel, c in zip(ACXEL_LIST, res["coverage"]):
        print(f"acxel {acxel:.2f}  mask_sum {int(c)}" + ("  expert" if c > EXPERT_MASK_SUM else ""))
    print(f"max_acxel {res['max_acxel']:.2f} (index {res['index']})")
    return res


if __name__ == "__main__":
    main()
