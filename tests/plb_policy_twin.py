"""Specification of the PLB closed-loop policy: a torch float64 restatement of the reference's Taichi MLP
(GenORM policy/pbm/plb/engine/nn/mlp.py), batched over B envs and differentiable by autograd.  No product code, no physics.

    obs_dims      mlp.py:32-34   obs_step = n_particle // n_observed_particles, obs_num = n_particle // obs_step,
                                 inp_dim = obs_num * 6 + primitives.state_dim (7 per primitive: position + quaternion)
    observation   mlp.py:68-86   input_particles / input_primitives
    layers        mlp.py:111-125 weights (h1_prev += W[i, j] * h0[j]) / bias (+ b[i], relu or tanh; none on the last layer, :58-60)
    policy        mlp.py:92-99   set_action: max(min(h, 1), -1)
    split_params  mlp.py:161-177 get_params / set_params: W_0, b_0, W_1, b_1, ... flat
"""
import torch

DT = torch.float64


def obs_dims(n_particles, n_primitive, n_observed):
    obs_step = n_particles // n_observed                      # mlp.py:32 (ZeroDivisionError below for n_particles < n_observed, as there)
    obs_num = n_particles // obs_step                         # :33
    return obs_step, obs_num, obs_num * 6 + 7 * n_primitive   # :34


def n_params(dims):
    return sum(dims[i + 1] * dims[i] + dims[i + 1] for i in range(len(dims) - 1))


def split_params(params, dims):
    """params [R, n_params] -> [(W_l [R, d_{l+1}, d_l], b_l [R, d_{l+1}])] (mlp.py:168-177)."""
    out, at = [], 0
    for i in range(len(dims) - 1):
        n = dims[i + 1] * dims[i]
        W = params[:, at:at + n].reshape(-1, dims[i + 1], dims[i])
        at += n
        b = params[:, at:at + dims[i + 1]]
        at += dims[i + 1]
        out.append((W, b))
    assert at == params.shape[1]
    return out


def observation(x, v, prim_pos, prim_rot, obs_step, obs_num, velocity_weight=1.0):
    """x, v [B,N,3]; prim_pos [B,P,3]; prim_rot [B,P,4] -> h_0 [B, 6 obs_num + 7 P]."""
    B = x.shape[0]
    idx = torch.arange(obs_num) * obs_step                                              # :72 x[.., i * obs_step]
    part = torch.cat([x[:, idx], v[:, idx] * velocity_weight], -1).reshape(B, -1)       # :72-74: h[i*6 + j] = x_j, h[i*6 + 3 + j] = v_j * vw
    prim = torch.cat([prim_pos, prim_rot], -1).reshape(B, -1)                           # :82-86: h[base + i*7 + j] = pos_j, + 3 + j = rot_j
    return torch.cat([part, prim], -1)


def layers(h0, params, dims, activation="relu"):
    """h_0 [B, d_0], params [B or 1, n_params] -> [h_0, h_1, ..., h_L] (hidden layers after the activation, the last one before the clamp)."""
    hs = [h0]
    wb = split_params(params, dims)
    for l, (W, b) in enumerate(wb):
        z = torch.einsum("rij,bj->bi", W, hs[-1]) if W.shape[0] == 1 else torch.einsum("bij,bj->bi", W, hs[-1])   # :113-115
        z = z + b                                                                        # :120
        if l != len(wb) - 1:                                                             # :58-60
            z = torch.relu(z) if activation == "relu" else torch.tanh(z)                 # :121-124
        hs.append(z)
    return hs


def policy(x, v, prim_pos, prim_rot, params, dims, obs_step, obs_num, activation="relu", velocity_weight=1.0):
    """The clamped action [B, d_L] (:98) and the list of layer outputs."""
    hs = layers(observation(x, v, prim_pos, prim_rot, obs_step, obs_num, velocity_weight), params, dims, activation)
    return torch.clamp(hs[-1], -1.0, 1.0), hs
