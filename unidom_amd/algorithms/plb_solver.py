"""Trajectory optimisation for the f64 PLB path: the reference's `Solver.solve` (optimizer/solver.py:31-71) with its `Adam` and `Momentum`
(optimizer/optim.py), the PLB counterpart of the apg* command lines.

The reference optimises one env's action sequence [horizon, action_dim] with ti.Tape; here B envs are optimised side by side (actions
[horizon, B, action_dim]; the envs are independent, so the gradient of the loss summed over envs is every env's own gradient) and
`loss.backward()` through PlbSimulator.step / PlbLoss.compute_loss plays the tape.  The optimisers work on float64 device tensors.

    python -m unidom_amd.algorithms.plb_solver --env torus --iters 10
    python -m unidom_amd.algorithms.plb_solver --env bimanual --iters 10     (two actuated Spheres: actions [horizon, B, 6])
"""
from __future__ import annotations

import argparse

import torch


class Optimizer:
    """optim.py:5-30.  `parameters` is updated in place; step(grads) returns a copy, clipped to `bounds`."""

    def __init__(self, parameters, lr=0.1, bounds=(-1.0, 1.0)):
        self.lr, self.bounds = float(lr), (float(bounds[0]), float(bounds[1]))
        self.parameters = parameters.detach().to(torch.float64).clone()
        self.initialize()

    def initialize(self):
        raise NotImplementedError

    def _step(self, grads):
        raise NotImplementedError

    def step(self, grads):
        assert grads.shape == self.parameters.shape
        self.parameters.copy_(self._step(grads.to(torch.float64)).clamp(*self.bounds))
        return self.parameters.clone()


class Momentum(Optimizer):
    def __init__(self, parameters, lr=0.1, bounds=(-1.0, 1.0), momentum=0.9):
        self.momentum = float(momentum)
        super().__init__(parameters, lr, bounds)

    def initialize(self):
        self.momentum_buffer = torch.zeros_like(self.parameters)

    def _step(self, grads):
        grads = self.momentum_buffer * self.momentum + grads * (1 - self.momentum)
        self.momentum_buffer.copy_(grads)
        return self.parameters - self.lr * grads


class Adam(Optimizer):
    def __init__(self, parameters, lr=0.1, bounds=(-1.0, 1.0), beta_1=0.9, beta_2=0.999, epsilon=1e-8):
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
        super().__init__(parameters, lr, bounds)

    def initialize(self):
        self.momentum_buffer = torch.zeros_like(self.parameters)
        self.v_buffer = torch.zeros_like(self.parameters)
        self.iter = 0

    def _step(self, grads):
        m_t = self.beta_1 * self.momentum_buffer + (1 - self.beta_1) * grads
        v_t = self.beta_2 * self.v_buffer + (1 - self.beta_2) * (grads * grads)
        self.momentum_buffer.copy_(m_t)
        self.v_buffer.copy_(v_t)
        m_cap = m_t / (1 - self.beta_1 ** (self.iter + 1))
        v_cap = v_t / (1 - self.beta_2 ** (self.iter + 1))
        self.iter += 1
        return self.parameters - (self.lr * m_cap) / (torch.sqrt(v_cap) + self.epsilon)


OPTIMS = {"Adam": Adam, "Momentum": Momentum}


class Solver:
    """Solver.solve of the reference: n_iters times (reset state -> loss.reset -> horizon steps, summing compute_loss()['loss'] ->
    backward -> optimiser step).  optim: a name of OPTIMS or a class; optim_kwargs go to its constructor (lr, bounds, ...)."""

    def __init__(self, sim, loss, horizon=50, n_iters=100, softness=666.0, optim="Adam", init_range=0.0, **optim_kwargs):
        self.sim, self.loss = sim, loss
        self.horizon, self.n_iters, self.softness, self.init_range = int(horizon), int(n_iters), float(softness), float(init_range)
        self.optim_cls = OPTIMS[optim] if isinstance(optim, str) else optim
        self.optim_kwargs = optim_kwargs
        self.total_steps = 0

    def init_actions(self):
        shape = (self.horizon, self.sim.batch_size, self.sim.action_dim)
        return (torch.rand(shape, dtype=torch.float64, device=self.sim.device) * 2 - 1) * self.init_range      # init_sampler 'uniform'

    def start_state(self):
        st = self.sim.reset()
        return st._replace(softness=torch.full_like(st.softness, self.softness))       # env.set_state(sim_state, softness, False)

    def forward(self, state0, actions):
        """(total loss over steps and envs, its gradient in the actions, the per-step info dicts)."""
        a = actions.detach().clone().requires_grad_(True)
        self.loss.reset(state0)
        state, total, infos = state0, None, []
        for i in range(a.shape[0]):
            state = self.sim.step(state, a[i])
            self.total_steps += 1
            info = self.loss.compute_loss(state)
            infos.append(info)
            total = info["loss"].sum() if total is None else total + info["loss"].sum()
        total.backward()
        return total.detach(), a.grad, infos

    def solve(self, init_actions=None, callbacks=()):
        actions = self.init_actions() if init_actions is None else torch.as_tensor(init_actions, dtype=torch.float64, device=self.sim.device)
        assert actions.shape == (self.horizon, self.sim.batch_size, self.sim.action_dim), tuple(actions.shape)
        optim = self.optim_cls(actions, **self.optim_kwargs)
        actions = optim.parameters.clone()
        state0 = self.start_state()
        self.total_steps = 0
        self.last_infos = None
        for _ in range(self.n_iters):
            self.params = actions.clone()
            loss, grad, self.last_infos = self.forward(state0, actions)
            actions = optim.step(grad)
            for callback in callbacks:
                callback(self, optim, loss, grad)
        return actions          # the last actions, as the reference returns them (not the best)


def make_goal(sim, actions, softness=666.0):
    """A goal density: the grid mass [n,n,n] of env 0 after stepping `actions` [K, action_dim] from the reset state."""
    with torch.no_grad():
        st = sim.reset()
        st = st._replace(softness=torch.full_like(st.softness, float(softness)))
        for a in actions:
            st = sim.step(st, a[None].expand(sim.batch_size, -1))
        return sim.get_grid_mass(st)[0].clone()


def main(argv=None):
    from ..engine.plb_losses import PlbLoss
    from ..engine.plb_simulator import BimanualConf, PlbConf, PlbSimulator, WriterConf
    ap = argparse.ArgumentParser(description="PLB trajectory optimisation towards a goal density (the reference's solve.py)")
    ap.add_argument("--env", choices=["torus", "writer", "bimanual"], default="torus")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--horizon", type=int, default=5)
    ap.add_argument("--num_envs", type=int, default=1)
    ap.add_argument("--optim", choices=sorted(OPTIMS), default="Adam")
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--softness", type=float, default=666.0)
    ap.add_argument("--goal_steps", type=int, default=5, help="the goal is the grid mass after this many steps of a fixed action")
    args = ap.parse_args(argv)
    cfg = {"writer": WriterConf, "bimanual": BimanualConf}.get(args.env, PlbConf)()
    sim = PlbSimulator(cfg, batch_size=args.num_envs)
    # the Capsule presses down / the sphere drags the torus sideways / the two spheres push the rod's ends towards each other
    push = {"writer": [0.0, -0.6, 0.0], "bimanual": [-0.6, 0.0, 0.0, 0.6, 0.0, 0.0]}.get(args.env, [0.6, 0.0, 0.0])
    goal_actions = torch.tensor([push] * args.goal_steps, dtype=torch.float64, device=sim.device)
    loss = PlbLoss(sim, weights=(1.0, 1.0, 1.0), soft_contact=True).load_target_density(make_goal(sim, goal_actions, args.softness))
    solver = Solver(sim, loss, horizon=args.horizon, n_iters=args.iters, softness=args.softness, optim=args.optim, init_range=0.0001, lr=args.lr)
    it = [0]

    def report(s, optim, total, grad):
        inc = s.last_infos[-1]["incremental_iou"]
        print("iter %3d  loss %.9g  incremental_iou %s" % (it[0], float(total), [round(v, 6) for v in inc.tolist()]), flush=True)
        it[0] += 1

    solver.solve(callbacks=(report,))
    sim.check_status()


if __name__ == "__main__":
    main()
