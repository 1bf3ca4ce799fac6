"""PlbPolicy -- the closed-loop policy of the f64 PLB path: host mirror of the reference's Taichi `MLP`
(GenORM policy/pbm/plb/engine/nn/mlp.py) over a PlbSimulator.

At every env step the policy reads a strided sample of the particle state plus every primitive's pose and produces the clamped action
(mlp.py:63-127, set_action :143-152); the arithmetic runs in libunidom_hip.so (csrc/plb_policy.hip: ud_plb_policy_fwd / _bwd).  The
reference holds one net in Taichi fields and differentiates it with ti.Tape; here `act` is a torch.autograd.Function over the kernel
pair, so `loss.backward()` through act -> PlbSimulator.step -> compute_loss carries the gradient back through physics -> action ->
MLP -> state -> earlier physics.  The parameter gradient does not travel through autograd: like Taichi's W.grad / b.grad fields it is
accumulated in place by the adjoint kernel into `grad`, which the caller zeroes (`zero_grad`).

B envs are batched: `shared=False` holds B independent policies side by side (parameters [B, n_params], B independent reference runs),
`shared=True` one policy read by every env (parameters [1, n_params]; `grad` sums the envs' rows).
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib

ACTIVATIONS = {"relu": 0, "tanh": 1}


def policy_dims(n_particles, n_primitive, action_dim, hidden_dims, n_observed_particles):
    """(obs_step, obs_num, dims) of mlp.py:30-39; a primitive's state is its position and its rotation quaternion (state_dim 7)."""
    if n_particles < n_observed_particles:
        raise ValueError(f"n_particles={n_particles} below n_observed_particles={n_observed_particles}: the reference's obs_step would be 0")
    obs_step = n_particles // n_observed_particles
    obs_num = n_particles // obs_step
    return obs_step, obs_num, (obs_num * 6 + 7 * n_primitive,) + tuple(int(h) for h in hidden_dims) + (int(action_dim),)


def _c(t):
    return t.detach().to(torch.float64).contiguous()


class _PlbPolicyAct(torch.autograd.Function):
    """ud_plb_policy_fwd / _bwd.  `params` is an input only so that the node exists when no state tensor requires grad (the first step
    of a rollout): its gradient is accumulated into policy._grad by the kernel and None is returned for it."""
    @staticmethod
    def forward(ctx, policy, x, v, pp, pr, params):
        L = _lib.lib()
        B = x.shape[0]
        x, v, pp, pr = map(_c, (x, v, pp, pr))
        action = torch.empty((B, policy.dims[-1]), dtype=torch.float64, device=x.device)
        tape = None
        if any(ctx.needs_input_grad):
            tape = torch.empty((L.ud_plb_policy_tape_bytes(B, policy.n_layer, policy._cdims) // 8,), dtype=torch.float64, device=x.device)
        stream = _lib.stream(x.device)
        _lib.check(L.ud_plb_policy_fwd(*policy._shape_args(B), *[_lib.ptr(t) for t in (x, v, pp, pr, params)], policy._param_stride,
                                       _lib.ptr(action), _lib.ptr(tape), stream), "ud_plb_policy_fwd")
        ctx.policy, ctx.B, ctx.shape_args = policy, B, policy._shape_args(B)
        ctx.save_for_backward(tape, params)
        return action

    @staticmethod
    def backward(ctx, g_action):
        L = _lib.lib()
        policy, B = ctx.policy, ctx.B
        tape, params = ctx.saved_tensors
        if tape is None:
            raise _lib.UnidomError("PLB policy backward without a tape (forward ran under no_grad)")
        sim, dev = policy.sim, params.device
        mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        gx, gv, gpp, gpr = mk(B, sim.n_particles, 3), mk(B, sim.n_particles, 3), mk(B, sim.n_primitive, 3), mk(B, sim.n_primitive, 4)
        stream = _lib.stream(dev)
        _lib.check(L.ud_plb_policy_bwd(*ctx.shape_args, _lib.ptr(params), policy._param_stride, _lib.ptr(tape), _lib.ptr(_c(g_action)),
                                       *[_lib.ptr(t) for t in (gx, gv, gpp, gpr, policy._grad)], stream), "ud_plb_policy_bwd")
        return None, gx, gv, gpp, gpr, None


class PlbPolicy:
    def __init__(self, sim, hidden_dims=(256, 256), activation="relu", n_observed_particles=200, shared=False):
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation {activation!r}: one of {sorted(ACTIVATIONS)}")
        if getattr(sim, "chopsticks", False):       # the reference's MLP asserts the same (engine/nn/mlp.py:26-27): its observation has no gap
            raise ValueError("PlbPolicy: a Chopsticks simulator (prim_kind[0] = 6) is not supported: the observation carries seven numbers per "
                             "primitive and the gap is not among them")
        self.sim, self.activation, self.shared = sim, activation, bool(shared)
        self.n_observed_particles = int(n_observed_particles)
        self.obs_step, self.obs_num, self.dims = policy_dims(sim.n_particles, sim.n_primitive, sim.action_dim, hidden_dims,
                                                             self.n_observed_particles)
        self.n_layer = len(self.dims) - 1
        self.n_params = sum(self.dims[i + 1] * self.dims[i] + self.dims[i + 1] for i in range(self.n_layer))
        self.n_rows = 1 if self.shared else int(sim.batch_size)
        self.velocity_weight = 1.0
        dev = torch.device(sim.device)
        # a leaf that requires grad so that `act` always builds its node; its .grad stays None (see _PlbPolicyAct), `grad` is ours
        self.params = torch.zeros((self.n_rows, self.n_params), dtype=torch.float64, device=dev, requires_grad=True)
        self._grad = torch.zeros((int(sim.batch_size), self.n_params), dtype=torch.float64, device=dev)
        self._cdims = (C.c_int * (self.n_layer + 1))(*self.dims)
        self._param_stride = 0 if self.shared else self.n_params
        self._const_rot = None

    def _shape_args(self, B):
        return (int(B), int(self.sim.n_particles), int(self.sim.n_primitive), self.obs_step, self.obs_num, self.n_layer, self._cdims,
                ACTIVATIONS[self.activation], float(self.velocity_weight))

    # ---- parameters (mlp.py:154-182) --------------------------------------------------------------------------------------------
    def get_params(self):
        """[n_rows, n_params]: every policy's W_0, b_0, W_1, b_1, ... (a copy)."""
        return self.params.detach().clone()

    def set_params(self, p):
        """p: [n_params] (every row gets it) or [n_rows, n_params].  One trailing extra element sets velocity_weight (one value for all
        rows: it is a scalar of the kernel call); without it velocity_weight is 1, as in the reference."""
        p = torch.as_tensor(p, dtype=torch.float64, device=self.params.device).detach()
        if p.dim() == 1:
            p = p[None].expand(self.n_rows, -1)
        if p.dim() != 2 or p.shape[0] != self.n_rows or p.shape[1] not in (self.n_params, self.n_params + 1):
            raise ValueError(f"parameters of shape {tuple(p.shape)}: expected [{self.n_rows}, {self.n_params}] (+ 1 for velocity_weight)")
        if p.shape[1] == self.n_params + 1:
            tail = p[:, -1]
            if not bool((tail == tail[0]).all()):
                raise ValueError("velocity_weight is one scalar for all envs: the trailing elements differ")
            self.velocity_weight = float(tail[0])
            p = p[:, :-1]
        else:
            self.velocity_weight = 1.0
        with torch.no_grad():
            self.params.copy_(p)

    def init_params(self, seed=0):
        """The reference's initialisation (solver_nn.py:79-98): torch.manual_seed, an f32 CPU nn.Linear stack of `dims`, flattened in
        parameters() order; row b is seeded with seed + b.  The caller's CPU generator is left as it was."""
        rows = []
        with torch.random.fork_rng(devices=[]):
            for b in range(self.n_rows):
                torch.manual_seed(int(seed) + b)
                layers = [torch.nn.Linear(self.dims[i], self.dims[i + 1]) for i in range(self.n_layer)]
                rows.append(torch.cat([q.detach().reshape(-1) for layer in layers for q in layer.parameters()]))
        self.set_params(torch.stack(rows).to(torch.float64))
        return self

    @property
    def grad(self):
        """[n_rows, n_params]: what the backward calls since zero_grad() accumulated (get_grad); a shared policy sums its envs."""
        return self._grad.sum(0, keepdim=True) if self.shared else self._grad

    def zero_grad(self):
        self._grad.zero_()

    # ---- the policy ---------------------------------------------------------------------------------------------------------------
    def _prim_rot(self, state):
        if getattr(self.sim, "rot_state", False):
            return state.prim_rot
        if self._const_rot is None:      # the conf's constant orientation, observed but not a state
            P = self.sim.n_primitive
            q = torch.tensor([tuple(r) for r in list(self.sim.cfg.prim_rot)[:P]], dtype=torch.float64, device=self.params.device).reshape(P, 4)
            self._const_rot = q[None].repeat(int(self.sim.batch_size), 1, 1).contiguous()
        return self._const_rot

    def act(self, state):
        """MLP.set_action: action [B, action_dim] = clamp(mlp(observation(state)), -1, 1), differentiable in state.x, state.v,
        state.prim_pos (and state.prim_rot on a rot_state simulator); the parameter gradient accumulates into `grad`."""
        assert state.x.shape[0] == self.sim.batch_size, (tuple(state.x.shape), self.sim.batch_size)
        return _PlbPolicyAct.apply(self, state.x, state.v, state.prim_pos, self._prim_rot(state), self.params)
