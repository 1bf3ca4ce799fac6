"""The Torus ("release") branch of the reference's expert generator (GenORM/policy/pbm/plb/optimizer/solver.py:290-350, solve_action): carry
the hanging rod's lower end to `start_pos` with the sticky Sphere in `approach` actions, hold, let go (set_softness1(0)) after action index
approach + hold - 1 (the reference's 300), and follow the rod's lowest particle for the rest: `release_point` is the Sphere's position at the
release, `max_x` the largest x that particle reaches.  These pairs are what GenORM/policy/src/Torus/*_train_para.py learn from.

The reference draws one (E, nu) per run of its loop over `i` and rolls the runs out one after the other; here run i is env i of one batch:
np.random.seed(version * 1000 + i), E ~ U(500, 10500), nu ~ U(0.2, 0.4), yield stress U(200, 200) (:127-144).  max_x is kept on the device
(a running maximum per env), and a rendered step is one render call for all envs, under torus.yml's directional light (TorusConf).

Left out: the GIF and its text overlay (the frames are returned instead), the Pinch branch (the reference ships no pinch.yml).

    python -m unidom_amd.algorithms.plb_release --env torus [--num_envs 8 --approach 200 --hold 101 --tail 299 --frames_every 0 --out x.npz]
"""
from __future__ import annotations

import argparse

import numpy as np
import torch

from ..engine.plb_render import render_conf_of
from ..engine.plb_simulator import PlbSimulator, TorusConf

START_POS = (0.2, 0.3, 0.5)                     # solver.py:299
E_RANGE, NU_RANGE, YIELD_RANGE = (500, 10500), (0.2, 0.4), (200, 200)       # :127-129
REPEAT_TIME = 1000                              # :117


def release_actions(prim0_pos, start_pos=START_POS, approach=200, hold=101, tail=299):
    """[approach + hold + tail, 3] float64: solver.py:301-304 -- the differences of `approach` evenly spaced points from the Sphere to
    start_pos, the first difference once more, then zeros (the reference's 400 = hold + tail)."""
    assert approach >= 2, approach
    init_actions = np.linspace(np.asarray(prim0_pos, np.float64), np.asarray(start_pos, np.float64), approach)
    init_actions = np.diff(init_actions, n=1, axis=0)
    init_actions = np.vstack([init_actions, init_actions[0][None, :]])
    return np.concatenate([init_actions, np.zeros((hold + tail, 3))])


def release_parameters(version, num_envs):
    """(E, nu, yield_stress), [num_envs] float64 each: env i is run i of the reference's loop (:139-142).  NumPy's global state is put back."""
    st = np.random.get_state()
    out = np.empty((3, num_envs))
    for i in range(num_envs):
        np.random.seed(int(version) * REPEAT_TIME + i)
        out[0, i] = np.random.uniform(*E_RANGE)
        out[1, i] = np.random.uniform(*NU_RANGE)
        out[2, i] = np.random.uniform(*YIELD_RANGE)
    np.random.set_state(st)
    return out[0], out[1], out[2]


def release(conf=None, num_envs=8, version=1, approach=200, hold=101, tail=299, frames_every=0, render_conf=None, spp=None, seed=0, out=None,
            device="cuda", env_name=None):
    """Returns dict(release_point [B,3], max_x [B], action [T,3], E, Poisson, yield_stress [B] (NumPy), state (the final PlbState), frames
    (uint8 [F,B,H,W,3] on the host, frame_steps the action indices they follow): frames_every N > 0 renders after every action whose index
    is a multiple of N (the reference's 5), 0 the final state only.  Writes the reference's bc_data fields per env to `out` (.npz) when
    given."""
    conf = TorusConf() if conf is None else conf
    B = int(num_envs)
    env_name = f"Torus-v{version}" if env_name is None else env_name
    sim = PlbSimulator(conf, batch_size=B, device=device)
    state = sim.reset()
    E, nu, ys = release_parameters(version, B)                       # taichi_env.set_parameter
    f64 = lambda a: torch.tensor(a, dtype=torch.float64, device=sim.device)
    state = state._replace(E=f64(E), nu=f64(nu), yield_stress=f64(ys))
    acts = release_actions(conf.prim_init_pos[0], START_POS, approach, hold, tail)
    a = f64(acts)
    bottom = state.x[:, :, 1].argmin(1, keepdim=True)                # rope_bottom_index (:306-307), per env
    max_x = torch.zeros((B,), dtype=torch.float64, device=sim.device)   # best_max_x = 0
    release_at = approach + hold - 1
    release_point, frames, frame_steps = None, [], []
    with torch.no_grad():
        for i in range(a.shape[0]):
            state = sim.step(state, a[i][None].expand(B, 3))
            if i == release_at:
                release_point = state.prim_pos[:, 0].clone()
                state = sim.set_softness1(state, 0.0)
            if frames_every > 0 and i % frames_every == 0:
                frames.append(sim.render(state, spp=spp, seed=seed, mode="rgb_array", render_conf=render_conf).cpu())
                frame_steps.append(i)
            max_x = torch.maximum(max_x, state.x.gather(1, bottom[:, :, None].expand(B, 1, 3))[:, 0, 0])
        sim.check_status()
        if frames_every <= 0:
            frames.append(sim.render(state, spp=spp, seed=seed, mode="rgb_array", render_conf=render_conf).cpu())
            frame_steps.append(a.shape[0] - 1)
    assert release_point is not None
    res = dict(release_point=release_point.cpu().numpy(), max_x=max_x.cpu().numpy(), action=acts, E=E, Poisson=nu, yield_stress=ys,
               env_name=env_name, state=state, frames=torch.stack(frames).numpy(), frame_steps=np.array(frame_steps))
    if out is not None:
        np.savez(out, **{k: res[k] for k in ("release_point", "max_x", "action", "E", "Poisson", "yield_stress", "env_name", "frame_steps")},
                 start_pos=np.array(START_POS), final_frame=res["frames"][-1])
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--env", default="torus", choices=["torus"])
    ap.add_argument("--num_envs", type=int, default=8)
    ap.add_argument("--version", type=int, default=1, help="the N of Torus-vN: seeds the parameter draws")
    ap.add_argument("--approach", type=int, default=200)
    ap.add_argument("--hold", type=int, default=101)
    ap.add_argument("--tail", type=int, default=299)
    ap.add_argument("--frames_every", type=int, default=0, help="render after every N-th action (the reference: 5); 0 = the final state only")
    ap.add_argument("--image_res", type=int, nargs="+", default=[512])
    ap.add_argument("--spp", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="write the reference's bc_data fields per env to this .npz")
    args = ap.parse_args(argv)
    conf = TorusConf()
    res2 = tuple(args.image_res) if len(args.image_res) == 2 else (args.image_res[0], args.image_res[0])
    rc = render_conf_of(conf, image_res=res2, spp=args.spp)
    res = release(conf, args.num_envs, args.version, args.approach, args.hold, args.tail, args.frames_every, render_conf=rc, seed=args.seed,
                  out=args.out)
    for i in range(args.num_envs):
        print(f"env {i}  E {res['E'][i]:.2f}  Poisson {res['Poisson'][i]:.4f}  yield_stress {res['yield_stress'][i]:.1f}  "
              f"release_point {np.round(res['release_point'][i], 4).tolist()}  max_x {res['max_x'][i]:.4f}")
    return res


if __name__ == "__main__":
    main()
