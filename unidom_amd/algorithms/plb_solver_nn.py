"""Closed-loop policy optimisation for the f64 PLB path: the reference's `SolverNN.solve` (optimizer/solver_nn.py:3-59), the second of
solve.py's differentiable algorithms (DIFF_ALGOS = ['action', 'nn']), on top of plb_solver's `Adam` / `Momentum`.

Where `Solver` optimises an action sequence, `SolverNN` optimises the parameters of a PlbPolicy that produces the action of every step
from the state (policy.act -> sim.step -> loss.compute_loss), so the gradient also runs through the observations.  The reference
trains one net in one env; here B envs run side by side: B independent policies (PlbPolicy(shared=False), parameters [B, n_params], each
env's best parameters tracked by its own summed loss) or one shared policy (parameters [1, n_params], tracked by the loss summed over
the envs).

    python -m unidom_amd.algorithms.plb_solver_nn --env torus --iters 10
"""
from __future__ import annotations

import argparse
import math

import torch

from .plb_solver import OPTIMS, make_goal


class SolverNN:
    """SolverNN.solve of the reference: n_iters times (set the parameters -> start state with the solver's softness -> loss.reset ->
    horizon x (policy.act -> sim.step -> compute_loss, summed) -> backward -> optimiser step).  lr is the given one x 0.001 and the
    parameters are unbounded (solver_nn.py:6-7).  Returns the best parameters seen (:45-59), not the last ones as `Solver` does."""

    def __init__(self, sim, loss, policy, horizon=50, n_iters=100, softness=666.0, optim="Adam", lr=0.1, **optim_kwargs):
        if getattr(sim, "chopsticks", False):       # the reference's MLP refuses a Chopsticks (engine/nn/mlp.py:26-27), and so does PlbPolicy
            raise ValueError("SolverNN: a Chopsticks simulator (prim_kind[0] = 6) has no policy; optimise its actions with plb_solver.Solver")
        self.sim, self.loss, self.policy = sim, loss, policy
        self.horizon, self.n_iters, self.softness = int(horizon), int(n_iters), float(softness)
        self.optim_cls = OPTIMS[optim] if isinstance(optim, str) else optim
        self.optim_kwargs = dict(optim_kwargs, lr=float(lr) * 0.001, bounds=(-math.inf, math.inf))
        self.total_steps = 0

    def start_state(self):
        st = self.sim.reset()
        return st._replace(softness=torch.full_like(st.softness, self.softness))       # env.set_state(sim_state, softness, False)

    def forward(self, state0, params):
        """(every env's loss summed over the steps [B], the gradient in the parameters [n_rows, n_params], the per-step info dicts)."""
        policy = self.policy
        policy.set_params(params)
        policy.zero_grad()
        self.loss.reset(state0)
        state, per_env, infos = state0, None, []
        for _ in range(self.horizon):
            state = self.sim.step(state, policy.act(state))
            self.total_steps += 1
            info = self.loss.compute_loss(state)
            infos.append(info)
            per_env = info["loss"] if per_env is None else per_env + info["loss"]
        per_env.sum().backward()
        return per_env.detach(), policy.grad.clone(), infos

    def solve(self, callbacks=()):
        policy = self.policy
        params = policy.get_params()
        optim = self.optim_cls(params, **self.optim_kwargs)
        state0 = self.start_state()
        self.total_steps = 0
        self.last_infos = None
        best = params.clone()
        self.best_loss = torch.full((params.shape[0],), 1e10, dtype=torch.float64, device=params.device)
        for _ in range(self.n_iters):
            self.params = params
            loss, grad, self.last_infos = self.forward(state0, params)
            row_loss = loss.sum(0, keepdim=True) if policy.shared else loss          # the loss each parameter row answers for
            better = row_loss < self.best_loss
            self.best_loss = torch.where(better, row_loss, self.best_loss)
            best = torch.where(better[:, None], params, best)
            params = optim.step(grad)
            for callback in callbacks:
                callback(self, optim, loss, grad)
        return best


def main(argv=None):
    from ..engine.plb_losses import PlbLoss
    from ..engine.plb_policy import PlbPolicy
    from ..engine.plb_simulator import BimanualConf, MoveConf, PlbConf, PlbSimulator
    ap = argparse.ArgumentParser(description="PLB closed-loop policy optimisation towards a goal density (the reference's solve.py --algo nn)")
    ap.add_argument("--env", choices=["torus", "move", "bimanual"], default="torus")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--horizon", type=int, default=5)
    ap.add_argument("--num_envs", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0, help="env b's policy is initialised with seed + b")
    ap.add_argument("--optim", choices=sorted(OPTIMS), default="Adam")
    ap.add_argument("--lr", type=float, default=0.01, help="solve.py's default; multiplied by 0.001, as the reference does")
    ap.add_argument("--softness", type=float, default=666.0)
    ap.add_argument("--goal_steps", type=int, default=5, help="the goal is the grid mass after this many steps of a fixed action")
    ap.add_argument("--hidden", type=int, nargs="*", default=[256, 256])
    ap.add_argument("--activation", choices=["relu", "tanh"], default="relu")
    ap.add_argument("--init_scale", type=float, default=0.01,
                    help="the last layer's initial W and b are multiplied by this (1 = the reference's initialisation as it is: on torus, whose "
                         "action scale is 1, that policy drives the sphere so hard that the state is no longer finite after three steps)")
    args = ap.parse_args(argv)
    cfg = {"move": MoveConf, "bimanual": BimanualConf}.get(args.env, PlbConf)()
    sim = PlbSimulator(cfg, batch_size=args.num_envs)
    # the sphere pushes the rod's end in / drags the torus sideways / the two spheres push the rod's ends towards each other
    push = {"move": [-0.6, 0.0, 0.0], "bimanual": [-0.6, 0.0, 0.0, 0.6, 0.0, 0.0]}.get(args.env, [0.6, 0.0, 0.0])
    goal_actions = torch.tensor([push] * args.goal_steps, dtype=torch.float64, device=sim.device)
    loss = PlbLoss(sim, weights=(1.0, 1.0, 1.0), soft_contact=True).load_target_density(make_goal(sim, goal_actions, args.softness))
    policy = PlbPolicy(sim, hidden_dims=tuple(args.hidden), activation=args.activation).init_params(args.seed)
    p = policy.get_params()
    p[:, -(policy.dims[-1] * policy.dims[-2] + policy.dims[-1]):] *= args.init_scale
    policy.set_params(p)
    solver = SolverNN(sim, loss, policy, horizon=args.horizon, n_iters=args.iters, softness=args.softness, optim=args.optim, lr=args.lr)
    it = [0]

    def report(s, optim, loss_env, grad):
        inc = s.last_infos[-1]["incremental_iou"]
        print("iter %3d  loss %.9g  |grad|_1 %.3g  incremental_iou %s" % (it[0], float(loss_env.sum()), float(grad.abs().sum()),
                                                                       [round(v, 6) for v in inc.tolist()]), flush=True)
        it[0] += 1

    solver.solve(callbacks=(report,))
    sim.check_status()


if __name__ == "__main__":
    main()
