"""GPU: the PLB closed-loop policy.  First the kernel pair alone (ud_plb_policy_fwd / _bwd, no simulator) against the torch twin
tests/plb_policy_twin.py, then PlbPolicy.act -> PlbSimulator.step -> PlbLoss and SolverNN against the same loop through the twins.

Tolerance of the kernel tests: derived, not chosen.  u = 2^-53, gamma_n = n u / (1 - n u).  Every output is a dot product of length n,
computed once on the device and once by the twin (each with an error of at most gamma_n sum |w| |h|, in any summation order), so
    forward   e_0 = 0 (the observation is copied; v * velocity_weight is the same single rounding on both sides)
              e_{l+1} = |W_l| e_l + 2 gamma_{d_l} (|W_l| |h_l| + |b_l|);  relu, tanh and the clamp are 1-Lipschitz: e(h) = e(z), e(action) = e_L
    adjoint   g_z_L = mask g_action: exact (the mask agrees, see below)
              g_h_l = W_l^T g_z_{l+1}:       e(g_h_l) = |W_l|^T e(g_z_{l+1}) + 2 gamma_{d_{l+1}} |W_l|^T |g_z_{l+1}|
              g_z_l = act'(h_l) g_h_l:       relu: act' in {0, 1} agrees, the product is exact: e(g_z_l) = act' e(g_h_l)
                                             tanh: act' = 1 - h^2, e(act') = 2 |h| e(h) + 4 u; e(g_z_l) = |act'| e(g_h_l) + |g_h_l| e(act') + 2 u |g_z_l|
              g_W_l[i,j] = g_z[i] h_l[j]:    e = e(g_z[i]) |h_l[j]| + |g_z[i]| e(h_l[j]) + 2 u |g_z[i] h_l[j]|;   g_b_l = g_z: e(g_z)
              g_x = g_h_0 (scattered); g_v = g_h_0 velocity_weight: |vw| e(g_h_0) + 2 u |g_h_0 vw|
              a second accumulating call adds p to p, which is exact: twice the gradient within twice the bound.
Condition, asserted on the twin before anything runs on the device, with no exception: no relu pre-activation within its forward
bound of 0 and no clamp input within its bound of +-1 (so every mask is the same on both sides), at least one output clamped and one not."""
import ctypes as C

import numpy as np
import pytest

from tests import plb_policy_twin as ptw

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
PAD, SENT = 64, 12345.678
ACT = {"relu": 0, "tanh": 1}

# off every tile edge: rows per workgroup 4, lanes 64, column slabs of 32 and 256, row groups of 8 and 4
CASES = {
    "tiny_relu": dict(B=1, N=23, n_obs=5, P=1, hidden=(17, 3), act="relu", vw=1.0, adim=3, shared=False, seed=1),
    "tanh_vw": dict(B=3, N=60, n_obs=7, P=2, hidden=(33,), act="tanh", vw=0.37, adim=6, shared=False, seed=2),
    "torus": dict(B=2, N=1000, n_obs=200, P=2, hidden=(256, 256), act="relu", vw=1.0, adim=3, shared=False, seed=3),
    "linear": dict(B=2, N=1500, n_obs=200, P=1, hidden=(), act="relu", vw=1.0, adim=6, shared=False, seed=4),
    "tanh_shared": dict(B=3, N=60, n_obs=7, P=2, hidden=(33,), act="tanh", vw=0.37, adim=3, shared=True, seed=5),
}


def gamma(n):
    return n * U / (1 - n * U)


def _mv(W, h):
    import torch
    return torch.einsum("bij,bj->bi", W, h)


def _mtv(W, g):
    import torch
    return torch.einsum("bij,bi->bj", W, g)


def forward_bounds(hs, wb):
    """[e_0, .., e_L] of the module docstring; hs, wb are the twin's (per-env parameters)."""
    import torch
    e = [torch.zeros_like(hs[0])]
    for l, (W, b) in enumerate(wb):
        A = W.abs()
        e.append(_mv(A, e[-1]) + 2 * gamma(W.shape[2]) * (_mv(A, hs[l].abs()) + b.abs()))
    return e


def kink_margins(hs, wb, e, act):
    """(smallest |z| - e over the relu pre-activations (inf without relu layers), smallest ||h_L| - 1| - e_L, #clamped, #unclamped)."""
    relu = np.inf
    if act == "relu":
        for l in range(len(wb) - 1):
            z = _mv(wb[l][0], hs[l]) + wb[l][1]
            relu = min(relu, float((z.abs() - e[l + 1]).min()))
    hl = hs[-1].abs()
    return relu, float(((hl - 1).abs() - e[-1]).min()), int((hl > 1).sum()), int((hl < 1).sum())


def adjoint_bounds(hs, wb, e, ga, act, vw):
    """(bound on g_params [B, n_params], bound on g_h_0 [B, d_0], g_h_0 itself) of the module docstring."""
    import torch
    L = len(wb)
    gz = ga * (hs[L].abs() <= 1)
    e_gz = torch.zeros_like(gz)
    eP = [None] * L
    for l in range(L - 1, -1, -1):
        W = wb[l][0]
        A = W.abs()
        eW = e_gz[:, :, None] * hs[l].abs()[:, None, :] + gz.abs()[:, :, None] * e[l][:, None, :] + 2 * U * (gz[:, :, None] * hs[l][:, None, :]).abs()
        eP[l] = torch.cat([eW.reshape(eW.shape[0], -1), e_gz], 1)
        gh = _mtv(W, gz)
        e_gh = _mtv(A, e_gz) + 2 * gamma(W.shape[1]) * _mtv(A, gz.abs())
        if l == 0:
            return torch.cat(eP, 1), e_gh, gh
        if act == "relu":
            d = (hs[l] > 0).to(gh.dtype)
            gz, e_gz = d * gh, d * e_gh
        else:
            d = 1 - hs[l] ** 2
            gz = d * gh
            e_gz = d.abs() * e_gh + gh.abs() * (2 * hs[l].abs() * e[l] + 4 * U) + 2 * U * gz.abs()


_REF = {}


def reference(name):
    """The twin's forward, autograd adjoint and the bounds of one case; computed once, shared, never written."""
    if name in _REF:
        return _REF[name]
    import torch
    c = CASES[name]
    B, N, P = c["B"], c["N"], c["P"]
    obs_step, obs_num, d0 = ptw.obs_dims(N, P, c["n_obs"])
    dims = (d0,) + tuple(c["hidden"]) + (c["adim"],)
    gen = torch.Generator().manual_seed(c["seed"])
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    nrm = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    x, v, pp, pr = rnd(B, N, 3), nrm(B, N, 3) * 0.5, rnd(B, P, 3), nrm(B, P, 4)
    pr = pr / pr.norm(dim=-1, keepdim=True)
    R = 1 if c["shared"] else B
    chunks = []
    for l in range(len(dims) - 1):                             # nn.Linear's scale; the last bias spreads the outputs across the clamp
        s = 1.0 / np.sqrt(dims[l])
        chunks.append((rnd(R, dims[l + 1] * dims[l]) * 2 - 1) * s)
        b = (rnd(R, dims[l + 1]) * 2 - 1) * s
        if l == len(dims) - 2:
            b = b + torch.linspace(-1.7, 1.7, dims[-1], dtype=torch.float64)
        chunks.append(b)
    params = torch.cat(chunks, 1)
    assert params.shape == (R, ptw.n_params(dims))
    ga = nrm(B, c["adim"])
    X, V, PP, PR = (t.clone().requires_grad_(True) for t in (x, v, pp, pr))
    PE = params.expand(B, -1).clone().requires_grad_(True)     # per-env rows: the kernel keeps one gradient row per env, shared or not
    action, hs = ptw.policy(X, V, PP, PR, PE, dims, obs_step, obs_num, c["act"], c["vw"])
    (action * ga).sum().backward()
    with torch.no_grad():
        hs = [h.detach() for h in hs]
        wb = ptw.split_params(PE.detach(), dims)
        e = forward_bounds(hs, wb)
        relu_m, clamp_m, n_clamped, n_free = kink_margins(hs, wb, e, c["act"])
        # the condition: zero exceptions
        assert relu_m > 0 and clamp_m > 0 and n_clamped >= 1 and n_free >= 1, (name, relu_m, clamp_m, n_clamped, n_free)
        e_params, e_gh0, gh0 = adjoint_bounds(hs, wb, e, ga, c["act"], c["vw"])
        np6 = 6 * obs_num
        idx = torch.arange(obs_num) * obs_step
        e_x, e_v = torch.zeros(B, N, 3, dtype=torch.float64), torch.zeros(B, N, 3, dtype=torch.float64)
        part, gpart = e_gh0[:, :np6].reshape(B, obs_num, 6), gh0[:, :np6].reshape(B, obs_num, 6)
        e_x[:, idx] = part[..., :3]
        e_v[:, idx] = abs(c["vw"]) * part[..., 3:] + 2 * U * (gpart[..., 3:] * c["vw"]).abs()
        e_prim = e_gh0[:, np6:].reshape(B, P, 7)
        observed = torch.zeros(N, dtype=torch.bool)
        observed[idx] = True
    ref = dict(c, name=name, dims=dims, obs_step=obs_step, obs_num=obs_num, x=x, v=v, pp=pp, pr=pr, params=params, ga=ga,
               action=action.detach(), hs=hs, e_action=e[-1], e_h=e, g_x=X.grad, g_v=V.grad, g_pp=PP.grad, g_pr=PR.grad, g_params=PE.grad,
               e_x=e_x, e_v=e_v, e_pp=e_prim[..., :3].contiguous(), e_pr=e_prim[..., 3:].contiguous(), e_params=e_params, observed=observed)
    _REF[name] = ref
    return ref


class _Guarded:
    """A device f64 array of n elements between two pads of sentinels."""

    def __init__(self, n, fill=SENT):
        import torch
        self.n = n
        self.big = torch.full((n + 2 * PAD,), SENT, dtype=torch.float64, device="cuda")
        self.view = self.big[PAD:PAD + n]
        self.view.fill_(fill)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        return bool((self.big[:PAD] == SENT).all()) and bool((self.big[PAD + self.n:] == SENT).all())

    def cpu(self, *shape):
        return self.view.cpu().reshape(*shape)


class _Device:
    """The case's inputs on the device and the two calls, every output in a guarded buffer."""

    def __init__(self, ref):
        import torch
        from unidom_amd import _lib
        self.L, self.r = _lib.lib(), ref
        r = ref
        self.dev = {k: r[k].contiguous().cuda() for k in ("x", "v", "pp", "pr", "params", "ga")}
        self.cdims = (C.c_int * len(r["dims"]))(*r["dims"])
        self.n_layer = len(r["dims"]) - 1
        self.n_params = int(self.L.ud_plb_policy_n_params(self.n_layer, self.cdims))
        assert self.n_params == ptw.n_params(r["dims"]) == r["params"].shape[1]
        self.stride = 0 if r["shared"] else self.n_params
        self.tape_doubles = int(self.L.ud_plb_policy_tape_bytes(r["B"], self.n_layer, self.cdims)) // 8
        assert self.tape_doubles >= r["B"] * sum(r["dims"])
        self.stream = torch.cuda.current_stream().cuda_stream

    def shape(self, **over):
        r = self.r
        a = dict(B=r["B"], N=r["N"], P=r["P"], obs_step=r["obs_step"], obs_num=r["obs_num"], n_layer=self.n_layer, dims=self.cdims,
                 act=ACT[r["act"]], vw=r["vw"])
        a.update(over)
        return [a[k] for k in ("B", "N", "P", "obs_step", "obs_num", "n_layer", "dims", "act", "vw")]

    def fwd(self, taped=True, **over):
        d, r = self.dev, self.r
        action, tape = _Guarded(r["B"] * r["dims"][-1]), _Guarded(self.tape_doubles)
        rc = self.L.ud_plb_policy_fwd(*self.shape(**over), d["x"].data_ptr(), d["v"].data_ptr(), d["pp"].data_ptr(), d["pr"].data_ptr(),
                                      d["params"].data_ptr(), self.stride, action.ptr, tape.ptr if taped else None, self.stream)
        return rc, action, tape

    def bwd(self, tape, g_params=None, **over):
        d, r = self.dev, self.r
        B, N, P = r["B"], r["N"], r["P"]
        out = dict(g_x=_Guarded(B * N * 3), g_v=_Guarded(B * N * 3), g_pp=_Guarded(B * P * 3), g_pr=_Guarded(B * P * 4),
                   g_params=_Guarded(B * self.n_params, 0.0) if g_params is None else g_params)
        rc = self.L.ud_plb_policy_bwd(*self.shape(**over), d["params"].data_ptr(), self.stride, tape.ptr, d["ga"].data_ptr(), out["g_x"].ptr,
                                      out["g_v"].ptr, out["g_pp"].ptr, out["g_pr"].ptr, out["g_params"].ptr, self.stream)
        return rc, out


def _within(got, want, bound):
    return bool(((got - want).abs() <= bound).all())


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_is_within_the_derived_bound_of_the_twin(name):
    import torch
    r = reference(name)
    dev = _Device(r)
    rc, action, tape = dev.fwd(taped=True)
    assert rc == 0
    B, dims = r["B"], r["dims"]
    got = action.cpu(B, dims[-1])
    worst = float(((got - r["action"]).abs() - r["e_action"]).max())
    print(name, "action: max(|got - twin| - e) =", worst, " max e =", float(r["e_action"].max()))
    assert _within(got, r["action"], r["e_action"])
    assert int((got.abs() == 1).sum()) == int((r["hs"][-1].abs() > 1).sum()) >= 1       # the clamped outputs are exactly +-1
    assert action.intact() and tape.intact()
    # the tape's layer outputs (h_0 exact, the others within their bounds): what the backward will read
    t = tape.cpu(B, -1)
    at = 0
    for l, h in enumerate(r["hs"]):
        assert _within(t[:, at:at + dims[l]], h, r["e_h"][l]), (name, l)
        at += dims[l]
    assert torch.equal(t[:, :dims[0]], r["hs"][0])
    # no tape: the same bits; and a second taped run: the same bits
    rc2, action2, tape2 = dev.fwd(taped=False)
    assert rc2 == 0 and torch.equal(action2.view, action.view) and action2.intact()
    assert bool((tape2.big == SENT).all())                      # nothing written without a tape
    rc3, action3, tape3 = dev.fwd(taped=True)
    assert rc3 == 0 and torch.equal(action3.view, action.view) and torch.equal(tape3.cpu(B, -1)[:, :sum(dims)], t[:, :sum(dims)])


@pytest.mark.parametrize("name", sorted(CASES))
def test_adjoint_is_within_the_derived_bound_of_the_twin(name):
    import torch
    r = reference(name)
    dev = _Device(r)
    rc, action, tape = dev.fwd(taped=True)
    assert rc == 0
    rc, out = dev.bwd(tape)
    assert rc == 0
    B, N, P = r["B"], r["N"], r["P"]
    shapes = dict(g_x=(B, N, 3), g_v=(B, N, 3), g_pp=(B, P, 3), g_pr=(B, P, 4), g_params=(B, dev.n_params))
    for k, shape in shapes.items():
        got, want, bound = out[k].cpu(*shape), r[k], r["e" + k[1:]]
        print(name, k, ": max(|got - twin| - e) =", float(((got - want).abs() - bound).max()), " max e =", float(bound.max()), " max |twin| =",
              float(want.abs().max()))
        assert _within(got, want, bound), (name, k)
        assert out[k].intact(), (name, k)
        assert float(want.abs().max()) > 0
    # unobserved particles: exact zeros, written (the buffers started as sentinels)
    gx, gv = out["g_x"].cpu(B, N, 3), out["g_v"].cpu(B, N, 3)
    assert int((~r["observed"]).sum()) == N - r["obs_num"] > 0
    assert bool((gx[:, ~r["observed"]] == 0).all()) and bool((gv[:, ~r["observed"]] == 0).all())
    assert tape.intact()
    # a second call accumulates: twice the gradient within twice the bound; every other output has the same bits as before
    rc, out2 = dev.bwd(tape, g_params=out["g_params"])
    assert rc == 0
    assert _within(out2["g_params"].cpu(B, dev.n_params), 2 * r["g_params"], 2 * r["e_params"]) and out2["g_params"].intact()
    for k in ("g_x", "g_v", "g_pp", "g_pr"):
        assert torch.equal(out2[k].view, out[k].view), (name, k)
    # a fresh run from zero: bit-identical to the first
    rc, out3 = dev.bwd(tape)
    rc4, out4 = dev.bwd(tape)
    assert rc == 0 and rc4 == 0 and torch.equal(out3["g_params"].view, out4["g_params"].view)
    assert _within(out3["g_params"].cpu(B, dev.n_params), r["g_params"], r["e_params"])


def test_invalid_arguments_return_the_code_and_launch_nothing():
    import torch
    from unidom_amd import _lib
    r = reference("tiny_relu")
    dev = _Device(r)
    rc, action, tape = dev.fwd(taped=True)
    assert rc == 0
    torch.cuda.synchronize()
    arr = lambda *d: (C.c_int * len(d))(*d)
    d = r["dims"]
    bad = [
        dict(dims=arr(d[0] + 1, *d[1:])),                        # dims[0] != 6 obs_num + 7 P
        dict(obs_step=0),
        dict(obs_step=6),                                        # (obs_num - 1) obs_step = 24 >= N = 23
        dict(n_layer=0),
        dict(n_layer=5, dims=arr(d[0], 4, 4, 4, 4, 3)),
        dict(dims=arr(d[0], 0, 3, 3)),                           # a width below 1
        dict(dims=arr(d[0], 17, 1025, 3)),                       # ... and above 1024
        dict(dims=arr(d[0], 17, 3, 1025)),
        dict(act=2),
    ]
    for over in bad:
        rc, a2, t2 = dev.fwd(taped=True, **over)
        assert rc == -1, over                                    # UD_ERR_INVALID
        msg = _lib.lib().ud_last_error().decode()
        assert "ud_plb_policy_fwd" in msg, msg
        rcb, out = dev.bwd(tape, **over)
        assert rcb == -1 and "ud_plb_policy_bwd" in _lib.lib().ud_last_error().decode(), over
        torch.cuda.synchronize()
        assert bool((a2.big == SENT).all()) and bool((t2.big == SENT).all()), over
        assert all(bool((out[k].big == SENT).all()) for k in ("g_x", "g_v", "g_pp", "g_pr")) and bool((out["g_params"].view == 0).all()), over
    L = _lib.lib()
    assert L.ud_plb_policy_n_params(0, dev.cdims) == 0 and L.ud_plb_policy_tape_bytes(1, 5, dev.cdims) == 0
    # the limits the header states are inside the supported range: 3 hidden layers of 1024, d_0 = 6 * 214 + 14
    big = arr(6 * 214 + 14, 1024, 1024, 1024, 6)
    assert L.ud_plb_policy_n_params(4, big) == 1024 * 1298 + 1024 + 2 * (1024 * 1024 + 1024) + 6 * 1024 + 6


# ---- end to end: the configuration of tests/test_plb_goal_gpu.py -----------------------------------------------------------------
H_E2E, N_OBS, HIDDEN = 2, 7, (16,)


def _e2e_dims():
    from tests import test_plb_goal_gpu as goal
    obs_step, obs_num, d0 = ptw.obs_dims(goal.N, 2, N_OBS)
    return obs_step, obs_num, (d0,) + HIDDEN + (3,)


def e2e_params(seed=7, scale=0.25):
    """nn.Linear-initialised rows (as PlbPolicy.init_params builds them), scaled so that the actions stay inside (-1, 1)."""
    import torch
    from tests import test_plb_goal_gpu as goal
    _, _, dims = _e2e_dims()
    rows = []
    for b in range(goal.B):
        torch.manual_seed(seed + b)
        stack = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)]
        rows.append(torch.cat([q.detach().reshape(-1) for m in stack for q in m.parameters()]).to(torch.float64))
    return torch.stack(rows) * scale


def twin_rollout(params, horizon=H_E2E, detach_obs=False):
    """policy twin -> PlbTorchTwin.step -> twin loss, `horizon` times from the reset state: (per-env summed loss [B] with its graph,
    the largest |h_L| seen, the smallest relu |pre-activation| seen)."""
    import torch
    from oracle.twin.plb_twin import torus_particles
    from oracle.twin.plb_twin_torch import PlbTorchTwin
    from tests import test_plb_goal_gpu as goal
    B, N, CONF = goal.B, goal.N, goal.CONF
    g = goal._goal()
    twin = PlbTorchTwin(CONF)
    obs_step, obs_num, dims = _e2e_dims()
    td, ts = torch.tensor(g["td"].reshape(-1)), torch.tensor(g["ts"].reshape(-1))
    f64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    rep = lambda a: f64(a)[None].repeat((B,) + (1,) * np.ndim(a))
    x = rep(torus_particles(N))
    v, Cm, F = torch.zeros((B, N, 3), dtype=torch.float64), torch.zeros((B, N, 3, 3), dtype=torch.float64), rep(np.eye(3)[None].repeat(N, 0))
    p = rep(np.array([[0.475, 0.05, 0.5], [0.5, 0.55, 0.5]]))
    rot = rep(np.array([[1.0, 0.0, 0.0, 0.0]] * 2))              # the conf's constant orientation
    soft = torch.full((B, 2), 666.0, dtype=torch.float64)
    E, nu, ys, fr = (torch.full((B,), val, dtype=torch.float64) for val in (CONF.E, CONF.nu, CONF.yield_stress, CONF.ground_friction))
    per_env, top, low = 0.0, 0.0, np.inf
    for _ in range(horizon):
        ox, ov, op = (t.detach() for t in (x, v, p)) if detach_obs else (x, v, p)
        a, hs = ptw.policy(ox, ov, op, rot, params, dims, obs_step, obs_num, "relu", 1.0)
        with torch.no_grad():
            wb = ptw.split_params(params, dims)
            top = max(top, float(hs[-1].abs().max()))
            low = min(low, float((_mv(wb[0][0], hs[0]) + wb[0][1]).abs().min()))
        x, v, Cm, F, p = twin.step(x, v, Cm, F, p, a, soft, E, nu, ys, fr)
        per_env = per_env + twin.loss(x, p, td, ts, goal.WEIGHTS, soft_contact=True)[0]
    return per_env, top, low


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-300)


def _hip_setup(params):
    from tests import test_plb_goal_gpu as goal
    from unidom_amd.engine.plb_losses import PlbLoss
    from unidom_amd.engine.plb_policy import PlbPolicy
    sim = goal._sim()
    loss = PlbLoss(sim, weights=goal.WEIGHTS, soft_contact=True).load_target_density(goal._goal()["td"])
    pol = PlbPolicy(sim, hidden_dims=HIDDEN, activation="relu", n_observed_particles=N_OBS)
    assert pol.dims == _e2e_dims()[2]
    pol.set_params(params)
    return sim, loss, pol


def test_loss_and_parameter_gradient_through_act_step_loss_match_the_twins():
    import torch
    torch.set_num_threads(8)
    params = e2e_params()
    P = params.clone().requires_grad_(True)
    per_env, top, low = twin_rollout(P)
    assert top < 0.9, top                                       # the actions stay inside (-1, 1)
    assert low > 1e-6, low                                      # and no relu unit sits where the 1e-9 forward bar could flip it
    per_env.sum().backward()
    g_ref = P.grad.numpy()
    assert np.abs(g_ref).max() > 0
    # part of that gradient arrives through the observed state (step 1 observes what step 0's action did), not only through the action
    Pd = params.clone().requires_grad_(True)
    twin_rollout(Pd, detach_obs=True)[0].sum().backward()
    through_state = _rel(Pd.grad.numpy(), g_ref)
    print("share of the parameter gradient through the state:", through_state)
    assert through_state > 1e-4, through_state                  # two orders above the 1e-6 bar below: the comparison sees it
    sim, loss, pol = _hip_setup(params)
    st0 = sim.reset()
    loss.reset(st0)
    pol.zero_grad()
    state, total = st0, 0.0
    for _ in range(H_E2E):
        state = sim.step(state, pol.act(state))
        total = total + loss.compute_loss(state)["loss"]
    total.sum().backward()
    sim.check_status()
    assert pol.params.grad is None and pol.grad.shape == params.shape
    f_err, g_err = _rel(total.detach().cpu().numpy(), per_env.detach().numpy()), _rel(pol.grad.cpu().numpy(), g_ref)
    print("end to end: loss rel", f_err, " gradient rel", g_err)
    assert f_err < 1e-9 and g_err < 1e-6


def twin_solve_nn(params0, n_iters, lr, horizon=H_E2E):
    """SolverNN's loop through the twins with the NumPy Momentum: (best parameters per env, per-iteration per-env losses, last parameters)."""
    import torch
    from tests import plb_target_twin as tw
    opt = tw.MomentumTwin(params0.numpy(), lr=lr * 0.001, bounds=(-np.inf, np.inf))
    params, losses, seen = params0.numpy().copy(), [], []
    for _ in range(n_iters):
        P = torch.tensor(params).requires_grad_(True)
        per_env = twin_rollout(P, horizon)[0]
        per_env.sum().backward()
        losses.append(per_env.detach().numpy())
        seen.append(params.copy())
        params = opt.step(P.grad.numpy())
    losses = np.array(losses)
    best = np.stack([seen[int(np.argmin(losses[:, b]))][b] for b in range(params0.shape[0])])
    return best, losses, params


SOLVE_LR = 10.0            # x 0.001 in SolverNN: chosen on the twin so that the summed loss falls and the two envs are best at different iterations


def test_solver_nn_with_momentum_follows_the_twin_loop():
    import torch
    from unidom_amd.algorithms.plb_solver_nn import SolverNN
    torch.set_num_threads(8)
    iters = 3
    params = e2e_params()
    ref_best, ref_losses, ref_last = twin_solve_nn(params, iters, SOLVE_LR)
    assert ref_losses[2].sum() < ref_losses[0].sum(), ref_losses   # first: the reference loop itself descends on this input
    assert len(set(np.argmin(ref_losses, 0).tolist())) == 2, ref_losses   # and the envs are best at different iterations: per-env tracking shows
    assert np.abs(ref_last - params.numpy()).max() > 1e-4       # and the optimiser really moved the parameters
    sim, loss, pol = _hip_setup(params)
    seen = []
    solver = SolverNN(sim, loss, pol, horizon=H_E2E, n_iters=iters, softness=666.0, optim="Momentum", lr=SOLVE_LR)
    got = solver.solve(callbacks=(lambda s, o, l, g: seen.append((l.cpu().numpy(), o.parameters.cpu().numpy())),))
    sim.check_status()
    assert got.shape == params.shape and solver.total_steps == H_E2E * iters
    losses = np.array([s[0] for s in seen])
    print("solver: losses rel", _rel(losses, ref_losses), " last parameters rel", _rel(seen[-1][1], ref_last), " best rel", _rel(got.cpu().numpy(), ref_best))
    assert _rel(losses, ref_losses) < 1e-9 and losses[2].sum() < losses[0].sum()
    assert _rel(seen[-1][1], ref_last) < 1e-6 and _rel(got.cpu().numpy(), ref_best) < 1e-6
