"""System identification for the f64 PLB path: the loop of PlasticineLab's sim2sim / real2sim trees (plb/optimizer/solver.py with the Adam of
plb/optimizer/optim.py:52-72).  A fixed action sequence is rolled out from guessed material parameters (E, nu, yield_stress), the grid
mass of the scored frames is held against a recorded trajectory of target densities (PlbTrajectoryLoss: sum over frames of
sum_I |grid_mass(x_f)_I - target[f]_I|), the loss is back-propagated to the three numbers (g_E, g_nu, g_yield_stress of
ud_plb_step_bwd) and Adam steps them.

The reference identifies one env per process; here the B envs of the simulator are B independent candidates (or recordings) side by
side: the loss summed over envs has every env's own gradient.

    python -m unidom_amd.algorithms.plb_identify --env move --horizon 5 --iters 3 --num_envs 2
"""
from __future__ import annotations

import argparse

import numpy as np
import torch

YIELD_STRESS = 200.0                                            # solver.py:22
SIM2SIM_BOUNDS = ((None, None), (0.2, 0.4), (None, None))       # sim2sim/plb/optimizer/solver.py:73
REAL2SIM_BOUNDS = ((500.0, 10700.0), (0.2, 0.4), (None, None))  # real2sim/plb/optimizer/solver.py:72-73
FLOOR = 0.01                                                    # np.clip(parameters, 0.01, 9999999999999999)


class ParameterAdam:
    """optim.py:52-72 on [B,3] parameters (E, nu, yield_stress): learning rates (lr, lr / 50000, lr), and no clipping to bounds inside the
    optimiser (optim.py:22-23).  `parameters` is the optimiser's own copy: what the solver clips afterwards never comes back in here, as
    in the reference, whose optimiser keeps stepping its unclipped array."""

    def __init__(self, parameters, lr=100.0, beta_1=0.9, beta_2=0.999, epsilon=1e-8):
        self.parameters = parameters.detach().to(torch.float64).clone()
        self.lr = torch.tensor([lr, lr / 50000, lr], dtype=torch.float64, device=self.parameters.device)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
        self.momentum_buffer = torch.zeros_like(self.parameters)
        self.v_buffer = torch.zeros_like(self.parameters)
        self.iter = 0

    def step(self, grads):
        assert grads.shape == self.parameters.shape
        gd = grads.to(torch.float64)
        m_t = self.beta_1 * self.momentum_buffer + (1 - self.beta_1) * gd
        v_t = self.beta_2 * self.v_buffer + (1 - self.beta_2) * (gd * gd)
        self.momentum_buffer.copy_(m_t)
        self.v_buffer.copy_(v_t)
        m_cap = m_t / (1 - self.beta_1 ** (self.iter + 1))
        v_cap = v_t / (1 - self.beta_2 ** (self.iter + 1))
        self.iter += 1
        self.parameters.copy_(self.parameters - (self.lr * m_cap) / (torch.sqrt(v_cap) + self.epsilon))
        return self.parameters.clone()


def constrain(parameters, pin, bounds):
    """What the solver does to the optimiser's output (solver.py:72-74): pin, clip to the bounds, floor.  parameters [B,3], a new tensor."""
    p = parameters.clone()
    for k, value in enumerate(pin):
        if value is not None:
            p[:, k] = float(value)
    for k, (lo, hi) in enumerate(bounds):
        if lo is not None or hi is not None:
            p[:, k] = p[:, k].clamp(min=lo, max=hi)
    return p.clamp(min=FLOOR)


class Identifier:
    """actions [H,3] (shared) or [H,B,3].  Frame i scores the state before step i; i = H is the state after the last step.  frames =
    range(H) is real2sim's loop, frames = (H - 1,) sim2sim's.  Steps behind the last scored frame cannot reach the loss and are not run.
    pin: per parameter a constant the solver puts back after every step (None = free)."""

    def __init__(self, sim, loss, actions, frames=None, softness=666.0, lr=100.0, pin=(None, None, YIELD_STRESS), bounds=SIM2SIM_BOUNDS):
        self.sim, self.loss = sim, loss
        B = sim.batch_size
        a = torch.as_tensor(actions, dtype=torch.float64, device=sim.device)
        if a.dim() == 2:
            a = a[:, None, :].expand(-1, B, -1)
        assert a.dim() == 3 and a.shape[1] == B, tuple(a.shape)
        self.actions = a.contiguous()
        self.horizon = H = a.shape[0]
        self.frames = tuple(range(H)) if frames is None else tuple(int(f) for f in frames)
        assert self.frames and all(0 <= f <= H for f in self.frames), (self.frames, H)
        self.softness, self.lr, self.pin, self.bounds = float(softness), float(lr), tuple(pin), tuple(bounds)
        self.total_steps = 0

    def start_state(self):
        st = self.sim.reset()
        return st._replace(softness=torch.full_like(st.softness, self.softness))

    def rollout(self, state0, parameters, n_steps=None):
        """The states before step 0 .. n_steps - 1 and after the last one (n_steps + 1 of them), E / nu / yield_stress taken from parameters [B,3]."""
        n_steps = self.horizon if n_steps is None else n_steps
        state = state0._replace(E=parameters[:, 0], nu=parameters[:, 1], yield_stress=parameters[:, 2])
        states = [state]
        for i in range(n_steps):
            state = self.sim.step(state, self.actions[i])
            self.total_steps += 1
            states.append(state)
        return states

    def forward(self, state0, parameters):
        """(loss per frame and env [len(frames),B], its gradient in the parameters [B,3])."""
        E, nu, ys = (parameters[:, k].detach().clone().requires_grad_(True) for k in range(3))
        states = self.rollout(state0, torch.stack([E, nu, ys], 1), max(self.frames))
        per_frame = self.loss.loss_of([states[f] for f in self.frames], self.frames)
        per_frame.sum().backward()
        zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
        return per_frame.detach(), torch.stack([zero(E), zero(nu), zero(ys)], 1)

    def solve(self, init_parameters, n_iters, callbacks=()):
        """Returns (best parameters [B,3]: per env those of the lowest loss, taken before the update; parameter history [n_iters,B,3]: the
        parameters after each update; loss history [n_iters,B])."""
        dev = self.sim.device
        parameters = torch.as_tensor(init_parameters, dtype=torch.float64, device=dev).reshape(self.sim.batch_size, 3).clone()
        optim = ParameterAdam(parameters, lr=self.lr)
        state0 = self.start_state()
        best = parameters.clone()
        best_loss = torch.full((self.sim.batch_size,), float("inf"), dtype=torch.float64, device=dev)
        history, losses = [], []
        self.total_steps = 0
        for _ in range(int(n_iters)):
            per_frame, grad = self.forward(state0, parameters)
            loss = per_frame.sum(0)
            better = loss < best_loss
            best = torch.where(better[:, None], parameters, best)
            best_loss = torch.where(better, loss, best_loss)
            parameters = constrain(optim.step(grad), self.pin, self.bounds)
            history.append(parameters.clone())
            losses.append(loss)
            for callback in callbacks:
                callback(self, optim, loss, grad, parameters)
        return best, torch.stack(history), torch.stack(losses)


def build_parser():
    ap = argparse.ArgumentParser(description="PLB system identification against a recorded grid-mass trajectory (sim2sim / real2sim solve)")
    ap.add_argument("--env", choices=["move", "writer"], default="move")
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--num_envs", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lr", type=float, default=100.0)
    ap.add_argument("--softness", type=float, default=666.0)
    ap.add_argument("--targets", default=None, help="a .npy of recorded grid masses [K,n,n,n], K >= horizon: real2sim (every frame is scored, "
                    "E is kept in [500, 10700]); without it a sim2sim run against a truth drawn from --seed")
    return ap


def draw_truth(seed):
    """solve_action (sim2sim/plb/optimizer/solver.py:126-129): np.random.seed(seed), E ~ U(500, 10500), then nu ~ U(0.2, 0.4)."""
    st = np.random.get_state()
    np.random.seed(seed)
    E, nu = np.random.uniform(500, 10500), np.random.uniform(0.2, 0.4)
    np.random.set_state(st)
    return E, nu


def draw_candidates(seed, B):
    """:155-158, one draw per env from seed + 10000000 + b: E ~ U(2000, 8000), nu ~ U(0.2, 0.4), yield stress 200.  [B,3]."""
    st = np.random.get_state()
    out = []
    for b in range(B):
        np.random.seed(seed + 10000000 + b)
        out.append([np.random.uniform(2000, 8000), np.random.uniform(0.2, 0.4), YIELD_STRESS])
    np.random.set_state(st)
    return np.array(out, np.float64)


def main(argv=None):
    from ..engine.plb_losses import PlbTrajectoryLoss
    from ..engine.plb_simulator import MoveConf, PlbSimulator, WriterConf
    args = build_parser().parse_args(argv)
    B, H = args.num_envs, args.horizon
    sim = PlbSimulator(WriterConf() if args.env == "writer" else MoveConf(), batch_size=B)
    actions = torch.tensor([[0.0, 0.6, 0.0]] * H, dtype=torch.float64, device=sim.device)
    loss = PlbTrajectoryLoss(sim)
    truth_last = None
    if args.targets is None:
        E, nu = draw_truth(args.seed)
        print("seed %d  truth E %.6g  Poisson %.6g  yield_stress %.6g" % (args.seed, E, nu, YIELD_STRESS), flush=True)
        ident = Identifier(sim, loss, actions, frames=(H - 1,), softness=args.softness, lr=args.lr, bounds=SIM2SIM_BOUNDS)
        truth = torch.tensor([[E, nu, YIELD_STRESS]] * B, dtype=torch.float64, device=sim.device)
        with torch.no_grad():
            states = ident.rollout(ident.start_state(), truth)
            loss.update_target_density(torch.stack([sim.get_grid_mass(s)[0] for s in states[:H]]))   # get_grid_mass before each step
        truth_last = states[-1].x[:1]
    else:
        loss.update_target_density(args.targets)
        assert loss.n_frames >= H, "--targets holds %d frames, --horizon is %d" % (loss.n_frames, H)
        ident = Identifier(sim, loss, actions, frames=range(H), softness=args.softness, lr=args.lr, bounds=REAL2SIM_BOUNDS)
    it = [0]

    def report(s, optim, l, grad, parameters):
        for b in range(B):
            print("iter %3d env %d  loss %.9g  E %.6f  Poisson %.6f  yield_stress %.6f" % ((it[0], b, float(l[b])) + tuple(parameters[b].tolist())),
                  flush=True)
        it[0] += 1

    best, history, losses = ident.solve(draw_candidates(args.seed, B), args.iters, callbacks=(report,))
    for b in range(B):
        print("env %d  best E %.6f  Poisson %.6f  yield_stress %.6f  (loss %.9g)" % ((b,) + tuple(best[b].tolist()) + (float(losses[:, b].min()),)))
    if truth_last is not None:
        with torch.no_grad():
            last = ident.rollout(ident.start_state(), history[-1])[-1].x
        print("chamfer distance of the last states (truth, estimate):", [float(v) for v in sim.chamfer(last, truth_last)])
    sim.check_status()


if __name__ == "__main__":
    main()
