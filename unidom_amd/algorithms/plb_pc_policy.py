"""The point-cloud policy of GenORM/policy on the f64 PLB path: the PointNet++ single-scale-grouping models (models/cls_ssg_model.py),
their behaviour-cloning trainer on the trajectory optimiser's rollouts (pbm/plb/optimizer/solver.py:376-414 collects them,
src/pinch/train_para.py trains and evaluates) and the closed loop on the simulator.

    optimise B trajectories side by side (plb_solver.Solver)  ->  collect()  ->  BehaviourCloner.fit()  ->  evaluate()

The sampling and grouping run in libunidom_hip.so (engine/pointnet.py over csrc/pc_group.hip); the conv stacks and the head are torch.
The simulator is float64, the policy float32 as in the reference (its TensorFlow model is f32, the Taichi simulator f64).

    python -m unidom_amd.algorithms.plb_pc_policy --env move --num_envs 2 --expert_iters 2 --epochs 3
"""
from __future__ import annotations

import argparse
import math
from typing import NamedTuple

import torch

from ..engine.pointnet import PointnetSA
from .plb_solver import Solver

BN_EPSILON = 1e-3          # keras BatchNormalization default
VOXEL_SIZE = 0.005         # util/preprocess.py:42


class _InferenceBN(torch.nn.Module):
    """keras BatchNormalization called without `training`: y = gamma (x - moving_mean) / sqrt(moving_var + eps) + beta with the moving
    statistics at their initial (0, 1); gamma and beta are trainable."""

    def __init__(self, features):
        super().__init__()
        self.gamma = torch.nn.Parameter(torch.ones(features))
        self.beta = torch.nn.Parameter(torch.zeros(features))
        self.scale = 1.0 / math.sqrt(1.0 + BN_EPSILON)

    def forward(self, x):
        return x * (self.gamma * self.scale) + self.beta


def _dense(fan_in, fan_out, generator=None):
    """keras Dense defaults: glorot_uniform kernel, zero bias."""
    lin = torch.nn.Linear(fan_in, fan_out)
    limit = math.sqrt(6.0 / (fan_in + fan_out))
    with torch.no_grad():
        lin.weight.copy_((torch.rand(lin.weight.shape, generator=generator) * 2 - 1) * limit)
        lin.bias.zero_()
    return lin


class ClsSsgModel(torch.nn.Module):
    """CLS_SSG_Model (cls_ssg_model.py:296-400), layer for layer:

        layer1  PointnetSA(512 centres, radius 0.02, 32 samples, mlp 64-64-128)   on (point, vector): 6 input channels
        layer2  PointnetSA(128 centres, radius 0.02, 64 samples, mlp 128-128-256) : 131 input channels
        layer3  PointnetSA(group_all, mlp 256-512-1024)                            : 259 input channels
        dense1 1024 -> 256, batchnorm1, dropout1, last_dense1 256 -> 128, last_dense2 128 -> action_size

    forward(point [B,n,3], vector [B,n,3]) -> action [B, action_size], float32.  The reference's quirks, kept:
      * activation=None is the default and what every training script passes: the conv stacks and the Dense layers are then linear.
      * last_dense2 carries the activation like every other Dense (the output is not a plain linear layer when one is given).
      * forward_pass hands no `training` flag to batchnorm1 and dropout1, so keras runs both in inference form, also inside
        train_step: the BN is the affine map gamma x / sqrt(1 + 1e-3) + beta (moving statistics never leave (0, 1), gamma / beta are
        trained), the dropout is the identity.  This is a reading of the keras source, not pinned by a run (TensorFlow is not here).
      * bn=True is refused (no reference script uses it).
    The conv kernels are glorot-normal, the Dense kernels keras' default glorot-uniform with zero bias."""

    head_in = 256

    def __init__(self, action_size=3, bn=False, activation=None, generator=None):
        super().__init__()
        if bn:
            raise NotImplementedError("bn=True: the reference's scripts all build the model with bn=False; only that is implemented")
        self.action_size, self.activation = int(action_size), activation
        self.layer1 = PointnetSA(512, 0.02, 32, [64, 64, 128], in_channels=3, activation=activation, generator=generator)
        self.layer2 = PointnetSA(128, 0.02, 64, [128, 128, 256], in_channels=128, activation=activation, generator=generator)
        self.layer3 = PointnetSA(None, None, None, [256, 512, 1024], in_channels=256, group_all=True, activation=activation, generator=generator)
        self.dense1 = _dense(1024, 256, generator)
        self.batchnorm1 = _InferenceBN(256)
        self.last_dense1 = _dense(self.head_in, 128, generator)
        self.last_dense2 = _dense(128, self.action_size, generator)

    def _act(self, x):
        return x if self.activation is None else self.activation(x)

    def features(self, point, vector):
        xyz, feats = self.layer1(point, vector)
        xyz, feats = self.layer2(xyz, feats)
        _, feats = self.layer3(xyz, feats)
        net = self._act(self.dense1(feats.reshape(feats.shape[0], -1)))
        return self.batchnorm1(net)                                # dropout1: the identity (see the class docstring)

    def head(self, net):
        return self._act(self.last_dense2(self._act(self.last_dense1(net))))

    def forward(self, point, vector):
        return self.head(self.features(point, vector))


class ClsSsgModelPara(ClsSsgModel):
    """CLS_SSG_Model_PARA (cls_ssg_model.py:181-293): ClsSsgModel whose head also reads the normalised material parameters [B,3].
    forward(point, vector, parameters).  One more quirk, kept: `parameters_process1 = Dense(256)` is overwritten on the next line by
    `parameters_process1 = BatchNormalization()`, and forward_pass calls it twice, so the parameters pass through that one BN (inference
    form, 3 features) twice and through no Dense; last_dense1 reads 256 + 3 values."""

    head_in = 259

    def __init__(self, action_size=3, bn=False, activation=None, generator=None):
        super().__init__(action_size, bn, activation, generator)
        self.parameters_process1 = _InferenceBN(3)

    def forward(self, point, vector, parameters):
        par = self.parameters_process1(self.parameters_process1(parameters.to(torch.float32)))
        return self.head(torch.cat([self.features(point, vector), par], dim=1))


def sample_pc(x, n_points, generator=None):
    """util/preprocess.py:38-44 on the device with torch ops: the means of the points in every occupied voxel of 0.005 (open3d
    voxel_down_sample: voxel index floor((p - (min - 0.0025)) / 0.005)), then n_points of them drawn with replacement.  x [N,3] ->
    [n_points,3]; x [B,N,3] -> [B,n_points,3] (cloud by cloud: the voxel counts differ).  Float32 out.  The voxels are listed in
    ascending (i, j, k) order; open3d's hash-map order is not pinned, so the draw differs from the reference's for the same seed."""
    if x.dim() == 3:
        return torch.stack([sample_pc(c, n_points, generator) for c in x])
    p = x.detach().to(torch.float64)
    cell = torch.floor((p - (p.min(0).values - 0.5 * VOXEL_SIZE)) / VOXEL_SIZE).to(torch.int64)
    extent = cell.max(0).values + 1
    key = (cell[:, 0] * extent[1] + cell[:, 1]) * extent[2] + cell[:, 2]
    _, inverse = torch.unique(key, sorted=True, return_inverse=True)
    n_vox = int(inverse.max()) + 1
    sums = torch.zeros((n_vox, 3), dtype=torch.float64, device=p.device).index_add_(0, inverse, p)
    counts = torch.zeros((n_vox,), dtype=torch.float64, device=p.device).index_add_(0, inverse, torch.ones_like(p[:, 0]))
    means = sums / counts[:, None]
    gdev = p.device if generator is None else generator.device
    pick = torch.randint(n_vox, (int(n_points),), generator=generator, device=gdev).to(p.device)
    return means[pick].to(torch.float32)


class Dataset(NamedTuple):
    points: torch.Tensor        # [R,n,3] float32
    vector: torch.Tensor        # [R,n,3] points - primitive 0's position
    parameters: torch.Tensor    # [R,3]  normalised
    action: torch.Tensor        # [R,action_dim]
    mean: torch.Tensor          # [3] what the parameters were normalised with
    std: torch.Tensor           # [3]


def normalise_parameters(parameters, mean=None, std=None):
    """(p - mean) / std per column over the rows, as train_para.py:219-222 does with the data set's lists (np.std: population);
    a column that does not vary is divided by 1.  Returns (normalised, mean, std)."""
    p = torch.as_tensor(parameters, dtype=torch.float64)
    mean = p.mean(0) if mean is None else torch.as_tensor(mean, dtype=torch.float64, device=p.device)
    if std is None:
        std = p.std(0, unbiased=False)
        std = torch.where(std > 0, std, torch.ones_like(std))
    std = torch.as_tensor(std, dtype=torch.float64, device=p.device)
    return ((p - mean) / std).to(torch.float32), mean, std


def collect(solver, parameters, actions=None, state0=None, n_points=200, generator=None):
    """The data set of one solved batch (solver.py:376-414 + create_dataset): the expert actions [H,B,A] (None: solver.solve() is run)
    are replayed from the start state and before every step the plasticine is sampled (sample_pc), giving H B rows of
    (points, vector = points - primitive 0's position, normalised parameters, action).  parameters [B,3]: each env's material
    parameters (any triple the caller identifies envs by), normalised over the batch."""
    sim = solver.sim
    if actions is None:
        actions = solver.solve()
    norm, mean, std = normalise_parameters(parameters)
    norm = norm.to(sim.device)
    rows = []
    with torch.no_grad():
        state = solver.start_state() if state0 is None else state0
        for a in actions:
            pts = sample_pc(state.x, n_points, generator)
            rows.append((pts, pts - state.prim_pos[:, :1].to(torch.float32), norm, a.to(torch.float32)))
            state = sim.step(state, a)
    cat = lambda k: torch.cat([r[k] for r in rows]).contiguous()
    return Dataset(cat(0), cat(1), cat(2), cat(3), mean, std)


def clip_per_tensor_(grads, clipnorm):
    """keras `clipnorm`: every gradient tensor on its own is scaled to an L2 norm of at most clipnorm (tf.clip_by_norm: g clipnorm /
    max(|g|, clipnorm)), not the global norm over all of them.  In place."""
    for g in grads:
        if g is not None:
            g.mul_(clipnorm / torch.clamp(g.norm(), min=clipnorm))
    return grads


class BehaviourCloner:
    """model.compile(Adam(lr, clipnorm=0.1), 'mean_squared_error') + fit of train_para.py:160-191: shuffled mini-batches, the remainder
    dropped, the per-tensor clip before the Adam step (keras Adam: epsilon 1e-7)."""

    def __init__(self, model, lr=1e-3, clipnorm=0.1):
        self.model, self.clipnorm = model, float(clipnorm)
        self.optim = torch.optim.Adam(model.parameters(), lr=float(lr), eps=1e-7)
        self.para = isinstance(model, ClsSsgModelPara)

    def predict(self, points, vector, parameters):
        return self.model(points, vector, parameters) if self.para else self.model(points, vector)

    def train_step(self, points, vector, parameters, action):
        self.optim.zero_grad(set_to_none=True)
        loss = torch.mean((self.predict(points, vector, parameters) - action) ** 2)
        loss.backward()
        clip_per_tensor_([p.grad for p in self.model.parameters()], self.clipnorm)
        self.optim.step()
        return loss.detach()

    def fit(self, data, epochs=1, batch_size=64, generator=None, callback=None):
        """Returns the mean training loss of every epoch."""
        R = data.points.shape[0]
        bs = min(int(batch_size), R)
        history = []
        for epoch in range(int(epochs)):
            order = torch.randperm(R, generator=generator).to(data.points.device)
            losses = [self.train_step(*(t[order[s:s + bs]] for t in (data.points, data.vector, data.parameters, data.action)))
                      for s in range(0, R - bs + 1, bs)]
            history.append(float(torch.stack(losses).mean()))
            if callback is not None:
                callback(epoch, history[-1])
        return history


def evaluate(model, sim, loss, parameters, horizon, state0=None, n_points=200, generator=None):
    """The closed loop of train_para.py:196-235 on B envs: every step samples the plasticine, asks the model for the action and
    steps the simulator.  parameters [B,3]: already normalised (ignored by a ClsSsgModel).  Returns each env's loss summed over the
    steps [B] and the last step's info dict."""
    para = isinstance(model, ClsSsgModelPara)
    with torch.no_grad():
        state = sim.reset() if state0 is None else state0
        loss.reset(state)
        total, info = None, None
        par = None if parameters is None else torch.as_tensor(parameters, dtype=torch.float32, device=sim.device)
        for _ in range(int(horizon)):
            pts = sample_pc(state.x, n_points, generator)
            vec = pts - state.prim_pos[:, :1].to(torch.float32)
            act = model(pts, vec, par) if para else model(pts, vec)
            state = sim.step(state, act.to(torch.float64))
            info = loss.compute_loss(state)
            total = info["loss"] if total is None else total + info["loss"]
    return total, info


class MaterialSolver(Solver):
    """plb_solver.Solver whose start state carries per-env material parameters: B experts for B materials side by side."""

    def __init__(self, sim, loss, E, nu, yield_stress, **kwargs):
        super().__init__(sim, loss, **kwargs)
        f = lambda v: torch.as_tensor(v, dtype=torch.float64, device=sim.device).reshape(sim.batch_size).contiguous()
        self.material = (f(E), f(nu), f(yield_stress))

    def start_state(self):
        E, nu, ys = self.material
        return super().start_state()._replace(E=E, nu=nu, yield_stress=ys)


def lame(E, nu):
    """(mu, lam) of (E, nu): the two numbers the reference's data sets are labelled with."""
    return E / (2 * (1 + nu)), E * nu / ((1 + nu) * (1 - 2 * nu))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="PLB point-cloud policy: optimise experts, clone them with the PointNet++ model, roll it out closed loop")
    ap.add_argument("--env", choices=["torus", "move"], default="move")
    ap.add_argument("--num_envs", type=int, default=2, help="experts (and materials) side by side")
    ap.add_argument("--expert_iters", type=int, default=10, help="iterations of the trajectory optimiser")
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--horizon", type=int, default=5, help="train_para.py's --num_steps")
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--expert_lr", type=float, default=0.1)
    ap.add_argument("--softness", type=float, default=666.0)
    ap.add_argument("--num_points", type=int, default=200, help="train_para.py's --num_plasticine_point")
    ap.add_argument("--goal_steps", type=int, default=5, help="the goal is the grid mass after this many steps of a fixed action")
    ap.add_argument("--no_parameters", action="store_true", help="ClsSsgModel instead of ClsSsgModelPara")
    return ap.parse_args(argv)


def main(argv=None):
    from ..engine.plb_losses import PlbLoss
    from ..engine.plb_simulator import MoveConf, PlbConf, PlbSimulator
    from .plb_solver import make_goal
    args = parse_args(argv)
    torch.manual_seed(args.seed)
    cfg = MoveConf() if args.env == "move" else PlbConf()
    sim = PlbSimulator(cfg, batch_size=args.num_envs)
    B = args.num_envs
    push = [-0.6, 0.0, 0.0] if args.env == "move" else [0.6, 0.0, 0.0]
    goal_actions = torch.tensor([push] * args.goal_steps, dtype=torch.float64, device=sim.device)
    loss = PlbLoss(sim, weights=(1.0, 1.0, 1.0), soft_contact=True).load_target_density(make_goal(sim, goal_actions, args.softness))
    # one material per env, spread around the conf's (the reference draws them per expert run)
    spread = torch.linspace(0.5, 1.5, B, dtype=torch.float64) if B > 1 else torch.ones(1, dtype=torch.float64)
    E, nu, ys = cfg.E * spread, torch.full((B,), cfg.nu, dtype=torch.float64), cfg.yield_stress * spread.flip(0)
    mu, lam = lame(E, nu)
    solver = MaterialSolver(sim, loss, E, nu, ys, horizon=args.horizon, n_iters=args.expert_iters, softness=args.softness, optim="Adam",
                            init_range=0.0001, lr=args.expert_lr)
    gen = torch.Generator(device=sim.device).manual_seed(args.seed)
    data = collect(solver, torch.stack([mu, lam, ys], 1), n_points=args.num_points, generator=gen)
    print("data set: %d rows of %d points" % (data.points.shape[0], data.points.shape[1]), flush=True)
    cpu_gen = torch.Generator().manual_seed(args.seed)
    model = (ClsSsgModel if args.no_parameters else ClsSsgModelPara)(sim.action_dim, generator=cpu_gen).to(sim.device)
    cloner = BehaviourCloner(model, lr=args.lr)
    cloner.fit(data, epochs=args.epochs, batch_size=args.batch_size, generator=cpu_gen,
               callback=lambda epoch, value: print("epoch %3d  mean_squared_error %.9g" % (epoch, value), flush=True))
    per_env, info = evaluate(model, sim, loss, data.parameters[:B], args.horizon, state0=solver.start_state(), n_points=args.num_points,
                             generator=gen)
    for b in range(B):
        print("env %d  closed-loop loss %.9g  incremental_iou %.6f" % (b, float(per_env[b]), float(info["incremental_iou"][b])), flush=True)
    sim.check_status()


if __name__ == "__main__":
    main()
