"""PlbLoss -- the goal side of the f64 PLB path: host mirror of the reference's `Loss` surface (engine/losses/loss.py).

A goal is a target density, i.e. the grid mass of a goal state (`PlbSimulator.get_grid_mass`; create_goal1.py saves
`taichi_env.get_grid_mass(0)`).  Loading one derives the target SDF from it on the device (Loss.load_target_density -> update_target ->
update_target_sdf, :46-106; csrc/plb_target.hip) and the soft IoU of the target with itself (:55-57).  `compute_loss` then reports what
every `env.step` of the reference reports (:269-298): the differentiable loss (through PlbSimulator.compute_loss, the existing kernels)
and its three parts, `iou`, `target_iou`, `reward` and `incremental_iou`, per env [B], all device tensors: nothing is copied to the host.
One target is shared by all envs, as ud_plb_loss_* takes it.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib


def target_sdf(density, threshold=1e-4, sweeps=0, want_nearest=False):
    """ud_plb_target_sdf.  density: device f64 [n,n,n] (one target) or [T,n,n,n]; returns (sdf, nearest or None, sweeps_run [T] int32) in the
    shape of the input.  sweeps = 0: the reference's 2 n_grid sweeps (later sweeps of a target at its fixed point return at entry)."""
    L = _lib.lib()
    assert density.is_cuda and density.dtype == torch.float64 and density.dim() in (3, 4), "density: device float64 [n,n,n] or [T,n,n,n]"
    d = density.contiguous()
    n = d.shape[-1]
    assert d.shape[-3:] == (n, n, n)
    T = 1 if d.dim() == 3 else d.shape[0]
    sdf = torch.empty_like(d)
    nearest = torch.empty(d.shape, dtype=torch.int32, device=d.device) if want_nearest else None
    run = torch.empty((T,), dtype=torch.int32, device=d.device)
    nbytes = L.ud_plb_target_work_bytes(n, T)
    work = torch.empty((max(int(nbytes), 4) // 4,), dtype=torch.int32, device=d.device)
    _lib.check(L.ud_plb_target_sdf(n, T, _lib.ptr(d), float(threshold), int(sweeps), *[_lib.ptr(t) for t in (sdf, nearest, run, work)],
                                   _lib.stream(d.device)), "ud_plb_target_sdf")
    return sdf, nearest, run


def density_iou(a, b):
    """ud_plb_density_iou (iou_kernel, :239-254).  a: device f64 [T, ...]; b: the same shape (per t) or a's without the leading axis (shared).
    Returns [T].  Deterministic: fixed-order sums.  max a = 0 or max b = 0 gives what IEEE gives (NaN)."""
    L = _lib.lib()
    assert a.is_cuda and a.dtype == torch.float64 and b.dtype == torch.float64 and b.device == a.device
    a, b = a.contiguous(), b.contiguous()
    T = a.shape[0]
    G = a[0].numel()
    batched = b.numel() == a.numel()
    assert batched or b.numel() == G, (tuple(a.shape), tuple(b.shape))
    out = torch.empty((T,), dtype=torch.float64, device=a.device)
    work = torch.empty((int(L.ud_plb_density_iou_work_bytes(T)) // 8,), dtype=torch.float64, device=a.device)
    _lib.check(L.ud_plb_density_iou(G, T, _lib.ptr(a), _lib.ptr(b), int(batched), _lib.ptr(out), _lib.ptr(work), _lib.stream(a.device)),
               "ud_plb_density_iou")
    return out


class PlbLoss:
    """Loss of engine/losses/loss.py over a PlbSimulator.  weights = (contact, density, sdf), the order of PlbSimulator.compute_loss."""

    def __init__(self, sim, weights=(1.0, 1.0, 1.0), soft_contact=True):
        self.sim = sim
        self.soft_contact = bool(soft_contact)
        self.set_weights(*weights)
        self.target_density = self.target_sdf = self.target_iou = None
        self._start_loss = self._init_iou = None

    def set_weights(self, contact, density, sdf, soft_contact=None):
        self.weights = torch.tensor([float(contact), float(density), float(sdf)], dtype=torch.float64, device=self.sim.device)
        if soft_contact is not None:
            self.soft_contact = bool(soft_contact)

    def load_target_density(self, grids, threshold=1e-4):
        """grids: a grid mass [n,n,n] (array, tensor) or the path of a .npy holding one (:46-57)."""
        if isinstance(grids, (str, bytes)) or hasattr(grids, "__fspath__"):
            grids = np.load(grids, allow_pickle=True)
        n = self.sim.n_grid
        if not torch.is_tensor(grids):
            grids = np.array(grids, dtype=np.float64)            # a copy, as the reference takes one
        td = torch.as_tensor(grids, dtype=torch.float64, device=self.sim.device).reshape(n, n, n).contiguous()
        self.target_density = td
        self.target_sdf = target_sdf(td, threshold)[0]
        self.target_iou = density_iou(td[None], td)          # [1]: broadcasts over the envs
        return self

    def _loss_and_iou(self, state):
        assert self.target_density is not None, "load_target_density first"
        loss, parts = self.sim.compute_loss(state, self.target_density, self.target_sdf, self.weights, self.soft_contact)
        iou = density_iou(self.sim.get_grid_mass(state), self.target_density)
        return loss, parts, iou

    def reset(self, state):
        """Loss.reset (:281-286): the loss and the IoU of the start state, against which reward and incremental_iou are taken."""
        with torch.no_grad():
            loss, _, iou = self._loss_and_iou(state)
        self._start_loss, self._init_iou = loss.detach(), iou
        return self

    def compute_loss(self, state):
        assert self._start_loss is not None, "reset(state) first"
        loss, parts, iou = self._loss_and_iou(state)
        tiou = self.target_iou.expand_as(iou)
        return {"loss": loss, "contact_loss": parts[:, 0], "density_loss": parts[:, 1], "sdf_loss": parts[:, 2], "iou": iou, "target_iou": tiou,
                "reward": self._start_loss - loss.detach(),
                "incremental_iou": incremental_iou_of(iou, self._init_iou, tiou)}


class PlbTrajectoryLoss:
    """The identification loss of PlasticineLab's sim2sim / real2sim trees (engine/losses/loss.py: new_target_density[f], update_target_density):
    a recording is a sequence of target densities, one per env step, and a rollout is scored frame by frame against it, the density term
    only.  All the frames of a rollout go through ONE PlbSimulator.density_seq_loss call."""

    def __init__(self, sim):
        self.sim = sim
        self.targets = None      # [T,n,n,n]
        self.n_frames = 0
        self.per_env = False

    def update_target_density(self, grids):
        """grids: [K,n,n,n], one recording shared by the envs, or [B,K,n,n,n], one per env (array, tensor, or the path of a .npy)."""
        if isinstance(grids, (str, bytes)) or hasattr(grids, "__fspath__"):
            grids = np.load(grids, allow_pickle=True)
        n, B = self.sim.n_grid, self.sim.batch_size
        if not torch.is_tensor(grids):
            grids = np.array(grids, dtype=np.float64)            # a copy, as the reference takes one
        g = torch.as_tensor(grids, dtype=torch.float64, device=self.sim.device)
        assert g.dim() in (4, 5) and tuple(g.shape[-3:]) == (n, n, n), tuple(g.shape)
        self.per_env = g.dim() == 5
        assert not self.per_env or g.shape[0] == B, (tuple(g.shape), B)
        self.n_frames = int(g.shape[-4])
        self.targets = g.detach().reshape(-1, n, n, n).contiguous().clone()
        return self

    def loss_of(self, states, frames):
        """states: a list of PlbState (or of x tensors [B,N,3]); frames: the target frame of each.  Returns [len(states), B]."""
        assert self.targets is not None, "update_target_density first"
        frames = [int(f) for f in frames]
        assert len(frames) == len(states) and all(0 <= f < self.n_frames for f in frames), (frames, self.n_frames)
        x = torch.stack([s.x if hasattr(s, "x") else s for s in states])        # [L,B,N,3]
        B = x.shape[1]
        fr = torch.tensor(frames, dtype=torch.int32, device=self.sim.device)[:, None].expand(-1, B)
        if self.per_env:
            assert B == self.sim.batch_size
            fr = fr + torch.arange(B, dtype=torch.int32, device=self.sim.device)[None] * self.n_frames
        return self.sim.density_seq_loss(x, self.targets, fr.contiguous())


def incremental_iou_of(iou, init_iou, target_iou):
    """incremental_iou of Loss.compute_loss (:294): clip((iou - init) / (target - init), 0, 1)."""
    return torch.clamp((iou - init_iou) / (target_iou - init_iou), 0.0, 1.0)
