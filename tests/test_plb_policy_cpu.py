"""CPU: the host side of the PLB closed-loop policy -- PlbPolicy's shapes, parameter surface and initialisation, and SolverNN's loop
over a stub simulator / loss (lr scaling, unbounded parameters, per-env best tracking, total_steps).  No kernel runs here: the
kernels are held to the twin in tests/test_plb_policy_gpu.py."""
import math

import numpy as np
import pytest

from tests import plb_policy_twin as ptw
from tests import plb_target_twin as tw


class _StubSim:
    """Just enough of PlbSimulator for PlbPolicy's constructor and SolverNN: the 'state' carries the actions applied so far."""

    def __init__(self, n_particles=1000, n_primitive=2, action_dim=3, batch_size=2):
        import torch
        self.n_particles, self.n_primitive, self.action_dim, self.batch_size = n_particles, n_primitive, action_dim, batch_size
        self.device = torch.device("cpu")
        self.rot_state = False
        self.softness_seen = []

    def reset(self):
        import torch
        from unidom_amd.engine.plb_simulator import PlbState
        z = torch.zeros((self.batch_size, 1), dtype=torch.float64)
        return PlbState(x=z, v=z, C=z, F=z, prim_pos=z, softness=torch.full((self.batch_size, self.n_primitive), 1.0, dtype=torch.float64),
                        E=z, nu=z, yield_stress=z)

    def step(self, state, action):
        self.softness_seen.append(float(state.softness[0, 0]))
        return state._replace(x=state.x + action.sum(-1, keepdim=True))


@pytest.mark.parametrize("N,n_obs,P,want", [(1000, 200, 2, (5, 200, 1214)), (1500, 200, 1, (7, 214, 1291)), (10000, 200, 1, (50, 200, 1207)),
                                            (23, 5, 1, (4, 5, 37))])
def test_observation_shape_follows_the_reference(N, n_obs, P, want):
    from unidom_amd.engine.plb_policy import PlbPolicy, policy_dims
    assert ptw.obs_dims(N, P, n_obs) == want
    step, num, dims = policy_dims(N, P, 3, (256, 256), n_obs)
    assert (step, num, dims[0]) == want and dims == (want[2], 256, 256, 3)
    assert (num - 1) * step < N                                # every observed particle exists
    pol = PlbPolicy(_StubSim(N, P, 6, 3), hidden_dims=(8,), n_observed_particles=n_obs)
    assert (pol.obs_step, pol.obs_num, pol.dims) == (want[0], want[1], (want[2], 8, 6))
    assert pol.n_params == ptw.n_params(pol.dims) == 8 * want[2] + 8 + 6 * 8 + 6 and pol.n_layer == 2
    assert pol.params.shape == (3, pol.n_params) and pol.grad.shape == (3, pol.n_params)
    shared = PlbPolicy(_StubSim(N, P, 6, 3), hidden_dims=(), n_observed_particles=n_obs, shared=True)
    assert shared.dims == (want[2], 6) and shared.params.shape == (1, shared.n_params) and shared.grad.shape == (1, shared.n_params)


def test_fewer_particles_than_observed_is_a_value_error():
    from unidom_amd.engine.plb_policy import PlbPolicy
    with pytest.raises(ZeroDivisionError):                     # what the reference does (mlp.py:32-33)
        ptw.obs_dims(150, 2, 200)
    with pytest.raises(ValueError, match="n_observed_particles"):
        PlbPolicy(_StubSim(150, 2, 3, 1))
    with pytest.raises(ValueError, match="activation"):
        PlbPolicy(_StubSim(), activation="gelu")


def test_set_params_get_params_round_trip_and_the_velocity_weight_tail():
    import torch
    from unidom_amd.engine.plb_policy import PlbPolicy
    pol = PlbPolicy(_StubSim(23, 1, 3, 2), hidden_dims=(4,), n_observed_particles=5)
    n = pol.n_params
    assert n == 4 * 37 + 4 + 3 * 4 + 3
    rng = np.random.default_rng(0)
    p = rng.normal(size=(2, n))
    pol.set_params(p)
    got = pol.get_params()
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), p) and pol.velocity_weight == 1.0
    got[0, 0] = 99.0                                           # a copy
    assert float(pol.get_params()[0, 0]) == p[0, 0]
    # the flat order is W_0, b_0, W_1, b_1 (mlp.py:161-177)
    (W0, b0), (W1, b1) = ptw.split_params(pol.get_params(), pol.dims)
    assert np.array_equal(W0[1].numpy(), p[1, :148].reshape(4, 37)) and np.array_equal(b0[1].numpy(), p[1, 148:152])
    assert np.array_equal(W1[1].numpy(), p[1, 152:164].reshape(3, 4)) and np.array_equal(b1[1].numpy(), p[1, 164:])
    # one trailing element sets velocity_weight (:178-182); without it, it is 1 again
    pol.set_params(np.concatenate([p, np.full((2, 1), 0.37)], 1))
    assert pol.velocity_weight == 0.37 and np.array_equal(pol.get_params().numpy(), p)
    pol.set_params(p[0])                                       # one vector: every row
    assert pol.velocity_weight == 1.0 and np.array_equal(pol.get_params().numpy(), np.stack([p[0], p[0]]))
    pol.set_params(np.concatenate([p[1], [2.5]]))
    assert pol.velocity_weight == 2.5 and np.array_equal(pol.get_params()[0].numpy(), p[1])
    with pytest.raises(ValueError):
        pol.set_params(np.zeros(n + 2))
    with pytest.raises(ValueError):
        pol.set_params(np.concatenate([p, [[0.1], [0.2]]], 1))   # velocity_weight is one scalar of the call
    pol._grad += 1.0
    pol.zero_grad()
    assert float(pol.grad.abs().sum()) == 0.0


def test_init_params_is_a_freshly_seeded_linear_stack():
    import torch
    from unidom_amd.engine.plb_policy import PlbPolicy
    pol = PlbPolicy(_StubSim(60, 2, 3, 2), hidden_dims=(16, 5), n_observed_particles=7)
    torch.manual_seed(123)
    before = torch.rand(1)
    torch.manual_seed(123)
    pol.init_params(seed=11)
    assert torch.equal(torch.rand(1), before)                  # the caller's generator is untouched
    for b in range(2):
        torch.manual_seed(11 + b)                              # solver_nn.py:79-98: nn.Linear stack, parameters() order, f32
        stack = [torch.nn.Linear(pol.dims[i], pol.dims[i + 1]) for i in range(3)]
        want = np.concatenate([q.data.cpu().numpy().reshape(-1) for m in stack for q in m.parameters()])
        assert want.dtype == np.float32 and np.array_equal(pol.get_params()[b].numpy(), want.astype(np.float64))
    assert not np.array_equal(pol.get_params()[0].numpy(), pol.get_params()[1].numpy())
    shared = PlbPolicy(_StubSim(60, 2, 3, 2), hidden_dims=(16, 5), n_observed_particles=7, shared=True).init_params(seed=11)
    assert np.array_equal(shared.get_params()[0].numpy(), pol.get_params()[0].numpy())


class _ScriptedLoss:
    """loss of iteration it, env b = script[it, b] + w[b] . (sum of the actions so far): a known constant gradient w per step."""

    def __init__(self, script, w):
        import torch
        self.script, self.w = torch.tensor(script), torch.tensor(w)
        self.it, self.resets, self.t = -1, 0, 0

    def reset(self, state):
        self.it += 1
        self.resets += 1
        self.t = 0

    def compute_loss(self, state):
        self.t += 1
        first = self.script[self.it] if self.t == 1 else 0.0   # the scripted part once per iteration
        return {"loss": first + state.x[:, 0] * self.w}


def _into_grad(pol):
    """A tensor hook that adds the action's cotangent [B,3] to the envs' gradient rows, as the adjoint kernel does."""
    def hook(g):
        pol._grad[:, :3].add_(g)
    return hook


def _policy_with_linear_act(sim, n_observed=5):
    """A real PlbPolicy whose `act` is replaced by action = params[:, :3] (no kernel on this machine); the cotangent goes where the
    adjoint kernel would put it, into policy.grad."""
    from unidom_amd.engine.plb_policy import PlbPolicy
    pol = PlbPolicy(sim, hidden_dims=(), n_observed_particles=n_observed)

    def act(state):
        a = pol.params[:, :3] * 1.0
        a.register_hook(_into_grad(pol))
        return a

    pol.act = act
    return pol


def test_solver_nn_loop_over_a_stub():
    import torch
    from unidom_amd.algorithms.plb_solver_nn import SolverNN
    B, H, iters, lr = 2, 3, 4, 50.0
    sim = _StubSim(23, 1, 3, B)
    pol = _policy_with_linear_act(sim)
    p0 = np.zeros((B, pol.n_params))
    p0[:, :3] = [[5.0, -7.0, 2.0], [0.5, 0.25, -3.0]]          # outside [-1, 1] from the start: nothing may clip them
    pol.set_params(p0)
    script = np.array([[5.0, 2.0], [1.0, 4.0], [3.0, 0.5], [9.0, 9.0]])     # env 0 is best at iteration 1, env 1 at iteration 2
    w = np.array([1e-3, -2e-3])
    loss = _ScriptedLoss(script, w)
    seen = []
    solver = SolverNN(sim, loss, pol, horizon=H, n_iters=iters, softness=321.0, optim="Momentum", lr=lr)
    best = solver.solve(callbacks=(lambda s, o, l, g: seen.append((o.lr, o.bounds, l.clone(), g.clone(), s.params.clone())),))
    assert solver.total_steps == H * iters and loss.resets == iters
    assert sim.softness_seen == [321.0] * (H * iters)          # the start state carries the solver's softness
    # lr x 0.001, bounds (-inf, inf) (solver_nn.py:6-7)
    assert all(abs(s[0] - lr * 0.001) < 1e-15 and s[1] == (-math.inf, math.inf) for s in seen)
    # the expected run: d loss_b / d params[b, :3] = w[b] * (H + (H-1) + ... + 1) (action t enters every later state)
    g = np.zeros_like(p0)
    g[:, :3] = (w * (H * (H + 1) / 2))[:, None]
    ref = tw.MomentumTwin(p0, lr=lr * 0.001, bounds=(-np.inf, np.inf))
    params, want_loss = [p0], []
    for it in range(iters):
        want_loss.append(script[it] + w * params[-1][:, :3].sum(-1) * (H * (H + 1) / 2))
        params.append(ref.step(g))
    for it in range(iters):
        assert np.allclose(seen[it][2].numpy(), want_loss[it], rtol=1e-13, atol=0)
        assert np.allclose(seen[it][3].numpy(), g, rtol=1e-13, atol=0) and np.allclose(seen[it][4].numpy(), params[it], rtol=1e-13, atol=0)
    assert np.abs(params[-1][:, :3]).max() > 1.0 and np.abs(params[-1] - p0).max() > 1e-4
    # per-env best: the parameters each env had when ITS loss was lowest, not the last ones and not one iteration for all envs
    arg = np.argmin(np.array(want_loss), 0)
    assert arg.tolist() == [1, 2]
    assert best.shape == (B, pol.n_params) and best.dtype == torch.float64
    assert np.allclose(best[0].numpy(), params[1][0], rtol=1e-13, atol=0) and np.allclose(best[1].numpy(), params[2][1], rtol=1e-13, atol=0)
    assert np.allclose(solver.best_loss.numpy(), np.array(want_loss).min(0), rtol=1e-13, atol=0)


def test_solver_nn_shared_policy_tracks_the_summed_loss():
    from unidom_amd.algorithms.plb_solver_nn import SolverNN
    from unidom_amd.engine.plb_policy import PlbPolicy
    B, H, iters = 2, 1, 3
    sim = _StubSim(23, 1, 3, B)
    pol = PlbPolicy(sim, hidden_dims=(), n_observed_particles=5, shared=True)

    def act(state):
        a = pol.params[:, :3].expand(B, 3) * 1.0
        a.register_hook(_into_grad(pol))
        return a

    pol.act = act
    script = np.array([[5.0, 2.0], [1.0, 4.0], [3.0, 3.5]])   # summed: 7, 5, 6.5 -> iteration 1
    solver = SolverNN(sim, _ScriptedLoss(script, np.array([1e-3, 1e-3])), pol, horizon=H, n_iters=iters, optim="Adam", lr=1.0)
    seen = []
    best = solver.solve(callbacks=(lambda s, o, l, g: seen.append((g.clone(), s.params.clone())),))
    assert best.shape == (1, pol.n_params) and seen[0][0].shape == (1, pol.n_params)
    assert np.allclose(seen[0][0][0, :3].numpy(), 2e-3)        # the shared row's gradient is the sum over the envs
    assert np.array_equal(best.numpy(), seen[1][1].numpy()) and not np.array_equal(best.numpy(), seen[2][1].numpy())
