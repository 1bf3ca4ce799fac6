"""PlbSimulator -- host mirror of GenORM's Taichi MPMSimulator + Primitives + Loss for the Torus task and PlasticineLab's
sim2sim Writer task (float64).

Mirrors /root/reference/GenORM/policy/pbm/plb/engine/mpm_simulator.py (constants :14-32, step :438-449 in copy
mode, substep_grad :271-289), the two Sphere primitives of envs/torus.yml, the Capsule of PlasticineLab/sim2sim/plb/envs/
writer.yml (engine/primitive/primive_base.py:57-115, primitives.py:55-73) and engine/losses/loss.py:112-243; the
physics runs in libunidom_hip.so (csrc/plb.hip forward, csrc/plb_adj.hip adjoint + losses).  The reference holds one
env per process in Taichi fields and differentiates with ti.Tape; here B independent envs are batched in one call and
`step` / `compute_loss` are torch.autograd Functions over the forward / adjoint kernel pairs, so
`loss.backward()` plays the role of the tape: gradients reach the particle state, the action, the primitive position and
the parameter leaves E, nu, yield_stress (PlasticineLab/sim2sim/plb/engine/mpm_simulator.py:27-29,485-498,
get_parameter_grad) and the ground friction (optimize_ground_friction, :57-58; `PlbSimulator.ground_friction_grad`).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from .. import _lib


class PlbState(NamedTuple):
    x: torch.Tensor          # [B,N,3] float64
    v: torch.Tensor          # [B,N,3]
    C: torch.Tensor          # [B,N,3,3]
    F: torch.Tensor          # [B,N,3,3]
    prim_pos: torch.Tensor   # [B,n_prim,3]
    softness: torch.Tensor   # [B,n_prim]
    E: torch.Tensor          # [B]
    nu: torch.Tensor         # [B]
    yield_stress: torch.Tensor  # [B]
    prim_rot: Optional[torch.Tensor] = None   # [B,n_prim,4] (w, x, y, z): a rot_state simulator only
    prim_gap: Optional[torch.Tensor] = None   # [B,n_prim]: a Chopsticks simulator only (the opening of primitive 0; primitive 1's entry is carried along)


class PlbConf:
    """cfg.SIMULATOR of plb/config/default_config.py:10-24 overridden by envs/torus.yml."""
    dim = 3
    quality = 1.0
    n_particles = 1000
    E = 5e3
    nu = 0.35
    yield_stress = 1762.2
    gravity = (0.0, -0.4, 0.0)
    ground_friction = 0.5
    dtype = "float64"
    # SHAPES / PRIMITIVES of torus.yml
    box_width = (0.028, 0.5, 0.028)
    box_init_pos = (0.5, 0.3, 0.5)
    prim_radius = (0.025, 0.025)
    prim_init_pos = ((0.475, 0.05, 0.5), (0.5, 0.55, 0.5))
    lower_bound = (0.0, 0.0, 0.0)
    upper_bound = (1.0, 1.0, 1.0)
    # per primitive (ud_plb_conf, include/unidom_hip.h): kind 0 = sticky Sphere, 1 = Capsule of height prim_h, constant orientation
    # prim_rot (w, x, y, z) and contact friction prim_friction; action_scale: v = clip(action) * scale / substeps (primitive 0)
    prim_kind = (0, 0)
    prim_h = (0.0, 0.0)
    prim_rot = ((1.0, 0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))
    prim_friction = (0.0, 0.0)
    # prim_kind 3 = Box, 4 = Cylinder, 5 = Torus (the base class's contact, as the Capsule): prim_shape holds the Box's three half extents
    # `size`, the Cylinder's (h, r, -) -- h the radial half extent, r the axial one -- or the Torus's (tx, ty, -); prim_radius and prim_h of
    # such a primitive are ignored (prim_radius still sets the number of primitives).  Kinds 0 to 2 ignore prim_shape
    prim_shape = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    action_scale = (1.0, 1.0, 1.0)
    # rotating primitives (ud_plb_conf.rot_state): every primitive's orientation is per-env state (PlbState.prim_rot, reset to prim_rot) and
    # turns once per substep; action_dim 6 = (v, w) of the base class, w scaled by action_scale_w; prim_kind 2 = RollingPin (three
    # action dimensions (dw, dth, dy), its own kinematics)
    rot_state = False
    action_dim = 3
    action_scale_w = (1.0, 1.0, 1.0)
    # prim_kind 6 = Chopsticks (primitive 0 only; needs rot_state and action_dim 7 = (v, w, gap_vel)): two Capsules of (prim_h, prim_radius) whose
    # opening is state (PlbState.prim_gap, reset to prim_init_gap) and closes once per substep by gap_vel = clip(action[6]) * action_scale_gap /
    # substeps, never below prim_min_gap
    prim_min_gap = (0.0, 0.0)
    prim_init_gap = (0.0, 0.0)
    action_scale_gap = 1.0
    # an actuated primitive 1 (ud_plb_conf.action_dim1): 0 = unactuated (the handle of before), 3 = it takes v, 6 = (v, w) of the base class
    # (needs rot_state).  The action row is [A0 + action_dim1] with primitive 0's A0 columns first (Primitives.set_action's running offsets,
    # primitives.py:307-311); primitive 1 is scaled by action_scale1 / action_scale_w1 and always follows the base class's kinematics
    action_dim1 = 0
    action_scale1 = (1.0, 1.0, 1.0)
    action_scale_w1 = (1.0, 1.0, 1.0)
    softness = 666.0         # Primitive cfg default, set_softness()
    # True: the handle is created with the unit action scale and `step` applies action.clamp(-1, 1) * action_scale in torch (the kernel's own
    # clip is then the identity; torch's clamp passes the cotangent at equality, as the header specifies) -- a Sphere handle with a scale
    # thereby runs the persistent kernels (launch_plan() == 2).  Every |action_scale| must be <= 1.  Not with rot_state.
    # With action_dim1 = 3 primitive 1's block is scaled by action_scale1 likewise
    action_scale_on_host = False


class TorusConf(PlbConf):
    """PlbConf (envs/torus.yml's SIMULATOR / SHAPES / PRIMITIVES) with the file's RENDERER block and colours: the directional light and the
    camera the Torus experts of solve_action are drawn through (algorithms/plb_release.py).  PlbConf itself carries neither, so its render()
    keeps the default camera and the sky light."""
    particle_color = 100                      # SHAPES[0].color
    prim_color = ((0.7, 0.7, 0.7), (0.7, 0.7, 0.7))   # PRIMITIVES[0..1].color
    render_overrides = {"use_directional_light": True, "camera_pos": (0.5, 0.27, 2.5), "camera_rot": (0.0, 0.0)}   # RENDERER


class MoveConf(PlbConf):
    """PlasticineLab/sim2sim/plb/envs/move.yml over sim2sim/plb/config/default_config.py, the env of the reference's identification runs:
    a 1000-particle rod lying on the floor and one Sphere at its end, action.scale 0.005.  E and nu are default_config's (the file sets
    neither).  The file's `mu` / `lam` entries (354.0, 2220.4) are read by nothing: mpm_simulator.py:26 takes cfg.E and cfg.nu, so they
    are not mirrored here.  The scale is applied on the host, so the handle runs the persistent path."""
    n_particles = 1000
    E = 5e3
    nu = 0.35
    yield_stress = 1762.2
    gravity = (0.0, -0.4, 0.0)
    ground_friction = 0.5
    box_width = (0.5, 0.028, 0.028)
    box_init_pos = (0.5, 0.0125, 0.5)
    prim_kind = (0,)
    prim_radius = (0.025,)
    prim_h = (0.0,)
    prim_init_pos = ((0.745, 0.02, 0.5),)
    prim_rot = ((1.0, 0.0, 0.0, 0.0),)
    prim_friction = (0.0,)
    action_scale = (0.005, 0.005, 0.005)
    action_scale_on_host = True


class BimanualConf(MoveConf):
    """A two-handed task.  THIS PROJECT'S OWN CHOICE: the reference's Primitives slices one action vector over any number of primitives
    (primitives.py:280-319) but ships no two-handed yml, so there is no file to mirror.  MoveConf's rod with a Sphere of radius 0.025 at each
    end, each taking three action dimensions (the action row is [B,6]: primitive 0's v, then primitive 1's) with action.scale 0.005.  Both
    scales are applied on the host, so the handle runs the persistent path."""
    prim_kind = (0, 0)
    prim_radius = (0.025, 0.025)
    prim_h = (0.0, 0.0)
    prim_init_pos = ((0.745, 0.02, 0.5), (0.255, 0.02, 0.5))
    prim_rot = ((1.0, 0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))
    prim_friction = (0.0, 0.0)
    action_dim1 = 3
    action_scale1 = (0.005, 0.005, 0.005)


class RopeConf(PlbConf):
    """GenORM/policy/pbm/plb/envs/rope.yml over plb/config/default_config.py, the paper's "unfold cloth" task: a 1500-particle sheet
    0.4 x 0.01 x 0.4 hanging over one Sphere that lifts and drops it.  The scale is applied on the host, so a handle of up to 1024 particles runs
    the persistent path; at the file's 1500 an env has more parts than one XCD holds and the library picks the multi-kernel path (launch_plan() == 1)."""
    n_particles = 1500                        # SHAPES[0].n_particles
    E = 5e3                                   # default_config.py (the file sets neither E nor nu)
    nu = 0.35                                 # default_config.py
    yield_stress = 50.0                       # default_config.py:15 (rope.yml does not set it; table.yml, move.yml and torus.yml set 1762.2)
    gravity = (0.0, -0.4, 0.0)                # SIMULATOR.gravity
    ground_friction = 0.5                     # SIMULATOR.ground_friction
    box_width = (0.4, 0.01, 0.4)              # SHAPES[0].width
    box_init_pos = (0.5, 0.04, 0.5)           # SHAPES[0].init_pos
    particle_color = 100                      # SHAPES[0].color: the key is given twice, ((0<<8) + (150<<16) + 150) then 100; the second wins: blue
    prim_kind = (0,)                          # PRIMITIVES[0].shape: Sphere
    prim_radius = (0.025,)                    # PRIMITIVES[0].radius
    prim_h = (0.0,)                           # (a Sphere has none)
    prim_init_pos = ((0.5, 0.05, 0.5),)       # PRIMITIVES[0].init_pos
    prim_rot = ((1.0, 0.0, 0.0, 0.0),)        # Primitive default init_rot
    prim_friction = (0.0,)                    # (read by no Sphere kernel: the Sphere is sticky)
    prim_color = ((0.7, 0.7, 0.7),)           # PRIMITIVES[0].color
    action_scale = (0.005, 0.005, 0.005)      # PRIMITIVES[0].action.scale
    action_scale_on_host = True               # the Sphere kernels (see PlbConf)
    # RENDERER: the top-down camera the experts of solve_action are selected through (use_directional_light is commented out: the default, off)
    render_overrides = {"camera_pos": (0.5, 2.0, 0.5), "camera_rot": (1.57, 0.0)}


class TableConf(PlbConf):
    """GenORM/policy/pbm/plb/envs/table.yml over plb/config/default_config.py, the paper's "lift cloth" task: the same sheet lying on the floor,
    one Sphere beside its corner.  The scale is applied on the host; which path runs: see RopeConf."""
    n_particles = 1500                        # SHAPES[0].n_particles
    E = 5e3                                   # default_config.py
    nu = 0.35                                 # default_config.py
    yield_stress = 1762.2                     # SIMULATOR.yield_stress
    gravity = (0.0, -0.4, 0.0)                # SIMULATOR.gravity
    ground_friction = 0.5                     # SIMULATOR.ground_friction
    box_width = (0.4, 0.01, 0.4)              # SHAPES[0].width
    box_init_pos = (0.5, 0.01, 0.5)           # SHAPES[0].init_pos
    particle_color = 100                      # SHAPES[0].color
    prim_kind = (0,)                          # PRIMITIVES[0].shape: Sphere
    prim_radius = (0.035,)                    # PRIMITIVES[0].radius
    prim_h = (0.0,)                           # (a Sphere has none)
    prim_init_pos = ((0.65, 0.025, 0.35),)    # PRIMITIVES[0].init_pos
    prim_rot = ((1.0, 0.0, 0.0, 0.0),)        # Primitive default init_rot
    prim_friction = (0.0,)                    # (read by no Sphere kernel)
    prim_color = ((0.7, 0.7, 0.7),)           # PRIMITIVES[0].color
    action_scale = (0.005, 0.005, 0.005)      # PRIMITIVES[0].action.scale
    action_scale_on_host = True               # the Sphere kernels (see PlbConf)
    render_overrides = {"use_directional_light": False}   # RENDERER.use_directional_light: False (the default camera)


class WriterConf(PlbConf):
    """PlasticineLab/sim2sim/plb/envs/writer.yml over sim2sim/plb/config/default_config.py: a 10 000-particle box on the floor
    (ground_friction 100: the floor stops what touches it) and one frictionless Capsule.  Runs the multi-kernel path."""
    n_particles = 10000
    E = 5e3
    nu = 0.35
    yield_stress = 50.0
    gravity = (0.0, -1.0, 0.0)
    ground_friction = 100.0
    box_width = (0.3, 0.1, 0.3)
    box_init_pos = (0.5, 0.05, 0.5)
    prim_kind = (1,)
    prim_radius = (0.03,)
    prim_h = (0.06,)
    prim_init_pos = ((0.5, 0.13, 0.5),)
    prim_rot = ((0.0, 0.0, 0.0, 1.0),)
    prim_friction = (0.0,)
    action_scale = (0.01, 0.01, 0.01)
    lower_bound = (0.0, 0.05, 0.0)
    upper_bound = (1.0, 1.0, 1.0)


class ChopsticksConf(PlbConf):
    """A small Chopsticks task.  THIS PROJECT'S OWN CHOICE: the reference registers a `Chopsticks` env name (plb/envs/__init__.py:6) but ships no
    chopsticks.yml, so there is no file to mirror.  The primitive takes the reference's defaults (primitives.py:166-173: h 0.06, r 0.03,
    minimal_gap 0.06, init_gap 0.06); the body is a 600-particle block on the floor, the sticks hang over it with their top end (the
    primitive's position) at y = 0.2 and open to 0.1, and the seven action dimensions are scaled as the Writer's.  Runs the multi-kernel path."""
    n_particles = 600
    E = 5e3
    nu = 0.35
    yield_stress = 50.0
    gravity = (0.0, -1.0, 0.0)
    ground_friction = 100.0
    box_width = (0.1, 0.1, 0.1)
    box_init_pos = (0.5, 0.05, 0.5)
    prim_kind = (6,)
    prim_radius = (0.03,)
    prim_h = (0.06,)
    prim_init_pos = ((0.5, 0.2, 0.5),)
    prim_rot = ((1.0, 0.0, 0.0, 0.0),)
    prim_friction = (0.9,)
    prim_min_gap = (0.06,)
    prim_init_gap = (0.1,)
    rot_state = True
    action_dim = 7
    action_scale = (0.01, 0.01, 0.01)
    action_scale_w = (0.05, 0.05, 0.05)
    action_scale_gap = 0.01
    lower_bound = (0.0, 0.05, 0.0)
    upper_bound = (1.0, 1.0, 1.0)


def _c(t):
    return t.detach().to(torch.float64).contiguous()


class _PlbStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sim, x, v, Cm, F, pp, so, action, E, nu, ys):
        L = _lib.lib()
        B = x.shape[0]
        x, v, Cm, F, pp, so, action, E, nu, ys = map(_c, (x, v, Cm, F, pp, so, action, E, nu, ys))
        xo, vo, Co, Fo, po = (torch.empty_like(t) for t in (x, v, Cm, F, pp))
        ckpt = None
        if any(ctx.needs_input_grad):
            ckpt = torch.empty((L.ud_plb_ckpt_bytes(sim._h, B) // 8,), dtype=torch.float64, device=x.device)
        stream = _lib.stream(x.device)
        ev = sim._prof_begin("fwd")
        args = (x, v, Cm, F, pp, so, action, E, nu, ys, xo, vo, Co, Fo, po, ckpt)
        _lib.check(L.ud_plb_step_fwd(sim._h, B, *[_lib.ptr(t) for t in args], stream), "ud_plb_step_fwd")
        sim._prof_end(ev)
        ctx.sim, ctx.B = sim, B
        ctx.save_for_backward(ckpt, so, action, E, nu, ys)
        return xo, vo, Co, Fo, po

    @staticmethod
    def backward(ctx, gx, gv, gC, gF, gpp):
        L = _lib.lib()
        sim, B = ctx.sim, ctx.B
        ckpt, so, action, E, nu, ys = ctx.saved_tensors
        if ckpt is None:
            raise _lib.UnidomError("PLB step backward without a checkpoint (forward ran under no_grad)")
        N, P, dev = sim.n_particles, sim.n_primitive, so.device
        g = lambda t: None if t is None else _c(t)
        gx, gv, gC, gF, gpp = map(g, (gx, gv, gC, gF, gpp))
        mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        ox, ov, oC, oF, op, oa = mk(B, N, 3), mk(B, N, 3), mk(B, N, 3, 3), mk(B, N, 3, 3), mk(B, P, 3), mk(B, sim.action_dim)
        oE, onu, oys, ofr = mk(B), mk(B), mk(B), mk(B)
        stream = _lib.stream(dev)
        ev = sim._prof_begin("bwd")
        args = (ckpt, so, action, E, nu, ys, gx, gv, gC, gF, gpp, ox, ov, oC, oF, op, oa, oE, onu, oys, ofr)
        _lib.check(L.ud_plb_step_bwd(sim._h, B, *[_lib.ptr(t) for t in args], stream), "ud_plb_step_bwd")
        sim._prof_end(ev)
        sim.ground_friction_grad = ofr if sim.ground_friction_grad is None else sim.ground_friction_grad + ofr
        return None, ox, ov, oC, oF, op, None, oa, oE, onu, oys


class _PlbStepRot(torch.autograd.Function):
    """_PlbStep over ud_plb_step_fwd_rot / _bwd_rot: prim_rot [B,P,4] is a state tensor and a differentiable leaf, action [B,action_dim]."""
    @staticmethod
    def forward(ctx, sim, x, v, Cm, F, pp, pr, so, action, E, nu, ys):
        L = _lib.lib()
        B = x.shape[0]
        x, v, Cm, F, pp, pr, so, action, E, nu, ys = map(_c, (x, v, Cm, F, pp, pr, so, action, E, nu, ys))
        xo, vo, Co, Fo, po, ro = (torch.empty_like(t) for t in (x, v, Cm, F, pp, pr))
        ckpt = None
        if any(ctx.needs_input_grad):
            ckpt = torch.empty((L.ud_plb_ckpt_bytes(sim._h, B) // 8,), dtype=torch.float64, device=x.device)
        stream = _lib.stream(x.device)
        ev = sim._prof_begin("fwd")
        args = (x, v, Cm, F, pp, pr, so, action, E, nu, ys, xo, vo, Co, Fo, po, ro, ckpt)
        _lib.check(L.ud_plb_step_fwd_rot(sim._h, B, *[_lib.ptr(t) for t in args], stream), "ud_plb_step_fwd_rot")
        sim._prof_end(ev)
        ctx.sim, ctx.B = sim, B
        ctx.save_for_backward(ckpt, so, action, E, nu, ys)
        return xo, vo, Co, Fo, po, ro

    @staticmethod
    def backward(ctx, gx, gv, gC, gF, gpp, gpr):
        L = _lib.lib()
        sim, B = ctx.sim, ctx.B
        ckpt, so, action, E, nu, ys = ctx.saved_tensors
        if ckpt is None:
            raise _lib.UnidomError("PLB step backward without a checkpoint (forward ran under no_grad)")
        N, P, dev = sim.n_particles, sim.n_primitive, so.device
        g = lambda t: None if t is None else _c(t)
        gx, gv, gC, gF, gpp, gpr = map(g, (gx, gv, gC, gF, gpp, gpr))
        mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        ox, ov, oC, oF, op, orot, oa = mk(B, N, 3), mk(B, N, 3), mk(B, N, 3, 3), mk(B, N, 3, 3), mk(B, P, 3), mk(B, P, 4), mk(B, sim.action_dim)
        oE, onu, oys, ofr = mk(B), mk(B), mk(B), mk(B)
        stream = _lib.stream(dev)
        ev = sim._prof_begin("bwd")
        args = (ckpt, so, action, E, nu, ys, gx, gv, gC, gF, gpp, gpr, ox, ov, oC, oF, op, orot, oa, oE, onu, oys, ofr)
        _lib.check(L.ud_plb_step_bwd_rot(sim._h, B, *[_lib.ptr(t) for t in args], stream), "ud_plb_step_bwd_rot")
        sim._prof_end(ev)
        sim.ground_friction_grad = ofr if sim.ground_friction_grad is None else sim.ground_friction_grad + ofr
        return None, ox, ov, oC, oF, op, orot, None, oa, oE, onu, oys


class _PlbStepGap(torch.autograd.Function):
    """_PlbStepRot over ud_plb_step_fwd_gap / _bwd_gap: prim_gap [B,P] is a state tensor and a differentiable leaf as well, action [B,7]."""
    @staticmethod
    def forward(ctx, sim, x, v, Cm, F, pp, pr, pg, so, action, E, nu, ys):
        L = _lib.lib()
        B = x.shape[0]
        x, v, Cm, F, pp, pr, pg, so, action, E, nu, ys = map(_c, (x, v, Cm, F, pp, pr, pg, so, action, E, nu, ys))
        xo, vo, Co, Fo, po, ro, go = (torch.empty_like(t) for t in (x, v, Cm, F, pp, pr, pg))
        ckpt = None
        if any(ctx.needs_input_grad):
            ckpt = torch.empty((L.ud_plb_ckpt_bytes(sim._h, B) // 8,), dtype=torch.float64, device=x.device)
        stream = _lib.stream(x.device)
        ev = sim._prof_begin("fwd")
        args = (x, v, Cm, F, pp, pr, pg, so, action, E, nu, ys, xo, vo, Co, Fo, po, ro, go, ckpt)
        _lib.check(L.ud_plb_step_fwd_gap(sim._h, B, *[_lib.ptr(t) for t in args], stream), "ud_plb_step_fwd_gap")
        sim._prof_end(ev)
        ctx.sim, ctx.B = sim, B
        ctx.save_for_backward(ckpt, so, action, E, nu, ys)
        return xo, vo, Co, Fo, po, ro, go

    @staticmethod
    def backward(ctx, gx, gv, gC, gF, gpp, gpr, gpg):
        L = _lib.lib()
        sim, B = ctx.sim, ctx.B
        ckpt, so, action, E, nu, ys = ctx.saved_tensors
        if ckpt is None:
            raise _lib.UnidomError("PLB step backward without a checkpoint (forward ran under no_grad)")
        N, P, dev = sim.n_particles, sim.n_primitive, so.device
        g = lambda t: None if t is None else _c(t)
        gx, gv, gC, gF, gpp, gpr, gpg = map(g, (gx, gv, gC, gF, gpp, gpr, gpg))
        mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        ox, ov, oC, oF, op, orot, ogap, oa = mk(B, N, 3), mk(B, N, 3), mk(B, N, 3, 3), mk(B, N, 3, 3), mk(B, P, 3), mk(B, P, 4), mk(B, P), mk(B, sim.action_dim)
        oE, onu, oys, ofr = mk(B), mk(B), mk(B), mk(B)
        stream = _lib.stream(dev)
        ev = sim._prof_begin("bwd")
        args = (ckpt, so, action, E, nu, ys, gx, gv, gC, gF, gpp, gpr, gpg, ox, ov, oC, oF, op, orot, ogap, oa, oE, onu, oys, ofr)
        _lib.check(L.ud_plb_step_bwd_gap(sim._h, B, *[_lib.ptr(t) for t in args], stream), "ud_plb_step_bwd_gap")
        sim._prof_end(ev)
        sim.ground_friction_grad = ofr if sim.ground_friction_grad is None else sim.ground_friction_grad + ofr
        return None, ox, ov, oC, oF, op, orot, ogap, None, oa, oE, onu, oys


class _PlbLossGap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sim, x, pp, pr, pg, td, ts, wt, soft):
        L = _lib.lib()
        B = x.shape[0]
        x, pp, pr, pg = _c(x), _c(pp), _c(pr), _c(pg)
        loss = torch.empty((B,), dtype=torch.float64, device=x.device)
        parts = torch.empty((B, 3), dtype=torch.float64, device=x.device)
        stream = _lib.stream(x.device)
        _lib.check(L.ud_plb_loss_fwd_gap(sim._h, B, *[_lib.ptr(t) for t in (x, pp, pr, pg, td, ts, wt)], int(soft), _lib.ptr(loss),
                                         _lib.ptr(parts), stream), "ud_plb_loss_fwd_gap")
        ctx.sim, ctx.B, ctx.soft = sim, B, soft
        ctx.save_for_backward(x, pp, pr, pg, td, ts, wt)
        ctx.mark_non_differentiable(parts)
        return loss, parts

    @staticmethod
    def backward(ctx, gl, _gparts):
        L = _lib.lib()
        x, pp, pr, pg, td, ts, wt = ctx.saved_tensors
        gl = _c(gl)
        gx, gpp, gpr, gpg = torch.empty_like(x), torch.empty_like(pp), torch.empty_like(pr), torch.empty_like(pg)
        stream = _lib.stream(x.device)
        _lib.check(L.ud_plb_loss_bwd_gap(ctx.sim._h, ctx.B, *[_lib.ptr(t) for t in (x, pp, pr, pg, td, ts, wt)], int(ctx.soft),
                                         *[_lib.ptr(t) for t in (gl, gx, gpp, gpr, gpg)], stream), "ud_plb_loss_bwd_gap")
        return None, gx, gpp, gpr, gpg, None, None, None, None


class _PlbLossRot(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sim, x, pp, pr, td, ts, wt, soft):
        L = _lib.lib()
        B = x.shape[0]
        x, pp, pr = _c(x), _c(pp), _c(pr)
        loss = torch.empty((B,), dtype=torch.float64, device=x.device)
        parts = torch.empty((B, 3), dtype=torch.float64, device=x.device)
        stream = _lib.stream(x.device)
        _lib.check(L.ud_plb_loss_fwd_rot(sim._h, B, *[_lib.ptr(t) for t in (x, pp, pr, td, ts, wt)], int(soft), _lib.ptr(loss),
                                         _lib.ptr(parts), stream), "ud_plb_loss_fwd_rot")
        ctx.sim, ctx.B, ctx.soft = sim, B, soft
        ctx.save_for_backward(x, pp, pr, td, ts, wt)
        ctx.mark_non_differentiable(parts)
        return loss, parts

    @staticmethod
    def backward(ctx, gl, _gparts):
        L = _lib.lib()
        x, pp, pr, td, ts, wt = ctx.saved_tensors
        gl = _c(gl)
        gx, gpp, gpr = torch.empty_like(x), torch.empty_like(pp), torch.empty_like(pr)
        stream = _lib.stream(x.device)
        _lib.check(L.ud_plb_loss_bwd_rot(ctx.sim._h, ctx.B, *[_lib.ptr(t) for t in (x, pp, pr, td, ts, wt)], int(ctx.soft),
                                         *[_lib.ptr(t) for t in (gl, gx, gpp, gpr)], stream), "ud_plb_loss_bwd_rot")
        return None, gx, gpp, gpr, None, None, None, None


class _PlbLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sim, x, pp, td, ts, wt, soft):
        L = _lib.lib()
        B = x.shape[0]
        x, pp = _c(x), _c(pp)
        loss = torch.empty((B,), dtype=torch.float64, device=x.device)
        parts = torch.empty((B, 3), dtype=torch.float64, device=x.device)
        stream = _lib.stream(x.device)
        _lib.check(L.ud_plb_loss_fwd(sim._h, B, *[_lib.ptr(t) for t in (x, pp, td, ts, wt)], int(soft), _lib.ptr(loss), _lib.ptr(parts),
                                     stream), "ud_plb_loss_fwd")
        ctx.sim, ctx.B, ctx.soft = sim, B, soft
        ctx.save_for_backward(x, pp, td, ts, wt)
        ctx.mark_non_differentiable(parts)
        return loss, parts

    @staticmethod
    def backward(ctx, gl, _gparts):
        L = _lib.lib()
        x, pp, td, ts, wt = ctx.saved_tensors
        gl = _c(gl)
        gx, gpp = torch.empty_like(x), torch.empty_like(pp)
        stream = _lib.stream(x.device)
        _lib.check(L.ud_plb_loss_bwd(ctx.sim._h, ctx.B, *[_lib.ptr(t) for t in (x, pp, td, ts, wt)], int(ctx.soft), _lib.ptr(gl),
                                     _lib.ptr(gx), _lib.ptr(gpp), stream), "ud_plb_loss_bwd")
        return None, gx, gpp, None, None, None, None


class _PlbDensitySeq(torch.autograd.Function):
    """ud_plb_density_seq_fwd / _bwd: x [M,N,3], targets [T,G], index [M] int32 or None -> loss [M].  Keeps x and the sign field."""
    @staticmethod
    def forward(ctx, sim, x, targets, index, work_bytes):
        L = _lib.lib()
        x = _c(x)
        M, dev = x.shape[0], x.device
        loss = torch.empty((M,), dtype=torch.float64, device=dev)
        sign = None
        if ctx.needs_input_grad[1]:
            sign = torch.empty((int(L.ud_plb_density_seq_sign_bytes(sim._h, M)) // 8,), dtype=torch.int64, device=dev)
        nbytes = int(L.ud_plb_density_seq_work_bytes(sim._h, M)) if work_bytes is None else int(work_bytes)
        work = torch.empty((max(nbytes // 8, 1),), dtype=torch.float64, device=dev)
        stream = _lib.stream(dev)
        _lib.check(L.ud_plb_density_seq_fwd(sim._h, M, _lib.ptr(x), _lib.ptr(targets), int(targets.shape[0]),
                                            *[_lib.ptr(t) for t in (index, loss, sign, work)], nbytes, stream), "ud_plb_density_seq_fwd")
        ctx.sim, ctx.M = sim, M
        ctx.save_for_backward(x, sign)
        return loss

    @staticmethod
    def backward(ctx, gl):
        x, sign = ctx.saved_tensors
        gl = _c(gl)
        gx = torch.empty_like(x)
        stream = _lib.stream(x.device)
        _lib.check(_lib.lib().ud_plb_density_seq_bwd(ctx.sim._h, ctx.M, *[_lib.ptr(t) for t in (x, sign, gl, gx)], stream),
                   "ud_plb_density_seq_bwd")
        return None, gx, None, None, None


class PlbSimulator:
    def __init__(self, cfg=None, batch_size=1, device="cuda"):
        cfg = PlbConf() if cfg is None else cfg
        assert cfg.dtype == "float64"                               # mpm_simulator.py:8
        self.cfg, self.batch_size, self.device = cfg, batch_size, torch.device(device)
        quality = cfg.quality * 0.5 if cfg.dim == 3 else cfg.quality   # :14-16
        self.n_particles = cfg.n_particles
        self.n_grid = int(128 * quality)
        self.dx, self.inv_dx = 1 / self.n_grid, float(self.n_grid)
        self.dt = 0.5e-4 / quality
        # :32 (float floor-division); `cfg.substeps` overrides it (ud_plb_conf.substeps is a handle constant): short horizons for tests
        self.substeps = int(getattr(cfg, "substeps", 0)) or int(2e-3 // self.dt)
        self.p_vol = (self.dx * 0.5) ** 2
        self.p_mass = self.p_vol * 1
        self.n_primitive = len(cfg.prim_radius)
        # include/unidom_hip.h: the checkpoint also keeps the touched grid cells and the adjoint restores them instead of running p2g
        # again (27 = every cell a substep can touch: never falls back; 36 B x 27 n_particles per env and substep of checkpoint)
        self.grid_ckpt_cells = int(getattr(cfg, "grid_ckpt_cells", 27))
        # kernel selection, fixed at create (include/unidom_hip.h): path 0 = the library's choice (one persistent launch per step call
        # where it fits), 1 = multi-kernel, 2 = persistent; lanes / sort_every: diagnostics of the multi-kernel path / the spatial order
        self.path, self.lanes, self.sort_every = (int(getattr(cfg, k, 0)) for k in ("path", "lanes", "sort_every"))
        P = self.n_primitive
        # action_scale_on_host: the handle gets the unit scale, step() scales the clamped action in torch
        self._host_scale = None
        handle_scale = tuple(float(s) for s in cfg.action_scale)
        if getattr(cfg, "action_scale_on_host", False):
            if any(abs(s) > 1.0 for s in handle_scale):
                raise ValueError(f"action_scale_on_host needs every |action_scale| <= 1 (the kernel clips the scaled action to [-1, 1]): {handle_scale}")
            if getattr(cfg, "rot_state", False):
                raise ValueError("action_scale_on_host is not available on a rot_state handle")
            self._host_scale = torch.tensor(handle_scale, dtype=torch.float64, device=self.device)
            handle_scale = (1.0, 1.0, 1.0)
        pad = lambda seq, fill: (list(seq)[:P] + [fill] * 2)[:2]
        self.prim_kind = tuple(int(k) for k in pad(cfg.prim_kind, 0))[:P]
        self.rot_state = bool(getattr(cfg, "rot_state", False))
        # the action row: primitive 0's A0 columns (3, 6, or the Chopsticks' 7), then primitive 1's action_dim1 (Primitives.action_dims)
        A0 = int(getattr(cfg, "action_dim", 3)) or 3
        self.action_dim1 = int(getattr(cfg, "action_dim1", 0))
        self.action_dim = A0 + self.action_dim1
        self.action_dims = (0, A0, self.action_dim)
        handle_scale1 = tuple(float(s) for s in getattr(cfg, "action_scale1", (1.0, 1.0, 1.0)))
        if self._host_scale is not None and self.action_dim1:
            if any(abs(s) > 1.0 for s in handle_scale1):
                raise ValueError(f"action_scale_on_host needs every |action_scale1| <= 1: {handle_scale1}")
            self._host_scale = torch.cat([self._host_scale, torch.tensor(handle_scale1, dtype=torch.float64, device=self.device)])
            handle_scale1 = (1.0, 1.0, 1.0)
        self.chopsticks = P > 0 and self.prim_kind[0] == 6          # the _gap entry points: PlbState.prim_gap is state
        rot = (C.c_double * 4 * 2)(*[(C.c_double * 4)(*q) for q in pad(cfg.prim_rot, (0.0, 0.0, 0.0, 0.0))])
        shape = (C.c_double * 3 * 2)(*[(C.c_double * 3)(*(list(sc) + [0.0] * 3)[:3]) for sc in pad(getattr(cfg, "prim_shape", ()), (0.0, 0.0, 0.0))])
        cc = _lib.ud_plb_conf(
            n_particles=self.n_particles, n_grid=self.n_grid, substeps=self.substeps, dt=self.dt,
            gravity=(C.c_double * 3)(*cfg.gravity), ground_friction=float(cfg.ground_friction), n_primitives=self.n_primitive,
            radius=(C.c_double * 2)(*(list(cfg.prim_radius) + [0.0])[:2]),
            lower_bound=(C.c_double * 3)(*cfg.lower_bound), upper_bound=(C.c_double * 3)(*cfg.upper_bound),
            grid_ckpt_cells=int(self.grid_ckpt_cells), max_envs=int(batch_size), path=self.path, lanes=self.lanes, sort_every=self.sort_every,
            prim_kind=(C.c_int * 2)(*pad(cfg.prim_kind, 0)), capsule_h=(C.c_double * 2)(*pad(cfg.prim_h, 0.0)), prim_rot=rot,
            prim_friction=(C.c_double * 2)(*pad(cfg.prim_friction, 0.0)), action_scale=(C.c_double * 3)(*handle_scale),
            rot_state=int(self.rot_state), action_dim=int(getattr(cfg, "action_dim", 3)),
            action_scale_w=(C.c_double * 3)(*getattr(cfg, "action_scale_w", (1.0, 1.0, 1.0))), prim_shape=shape,
            min_gap=(C.c_double * 2)(*pad(getattr(cfg, "prim_min_gap", ()), 0.0)), action_scale_gap=float(getattr(cfg, "action_scale_gap", 1.0)),
            action_dim1=self.action_dim1, action_scale1=(C.c_double * 3)(*handle_scale1),
            action_scale_w1=(C.c_double * 3)(*getattr(cfg, "action_scale_w1", (1.0, 1.0, 1.0))))
        self._h = C.c_void_p()
        self.profile = None    # {"fwd": [], "bwd": []}: HIP-event pairs around every step call, on its stream (bench.py)
        self.ground_friction_grad = None   # [B], accumulated by backward() (optimize_ground_friction.grad); reset it by hand
        _lib.check(_lib.lib().ud_plb_create(C.byref(cc), C.byref(self._h)), "ud_plb_create")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.lib().ud_plb_destroy(self._h)
        except Exception:
            pass

    def _prof_begin(self, kind):
        if self.profile is None:
            return None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(torch.cuda.current_stream(self.device))
        return (kind, a, b)

    def _prof_end(self, ev):
        if ev is not None:
            ev[2].record(torch.cuda.current_stream(self.device))
            self.profile[ev[0]].append((ev[1], ev[2]))

    def launch_plan(self, B=None):
        """ud_plb_launch_plan: 1 = multi-kernel path, 2 = one persistent launch per step call and direction"""
        return int(_lib.lib().ud_plb_launch_plan(self._h, self.batch_size if B is None else B))

    def check_status(self):
        """Synchronises the current stream; raises if a workgroup of the persistent kernels gave up waiting (outputs NaN); the handle is usable
        again afterwards (ud_plb_poll_timeouts resets its exchange arena)."""
        stream = _lib.stream(self.device)
        n = int(_lib.lib().ud_plb_poll_timeouts(self._h, stream))
        if n != 0:
            raise _lib.UnidomError(_lib.lib().ud_last_error().decode())

    def reset(self) -> PlbState:
        """Shapes.add_box with np.random.seed(0) (shape_maker.py:21-31,49-58) + primitive init (torus.yml / writer.yml)."""
        cfg, B, dev = self.cfg, self.batch_size, self.device
        st = np.random.get_state()
        np.random.seed(0)
        p = (np.random.random((cfg.n_particles, 3)) * 2 - 1) * (0.5 * np.array(cfg.box_width)) + np.array(cfg.box_init_pos)
        np.random.set_state(st)
        f64 = lambda a: torch.tensor(np.asarray(a, np.float64), device=dev)
        rep = lambda t: t[None].repeat((B,) + (1,) * t.dim()).contiguous()
        N = cfg.n_particles
        return PlbState(x=rep(f64(p)), v=torch.zeros((B, N, 3), dtype=torch.float64, device=dev),
                        C=torch.zeros((B, N, 3, 3), dtype=torch.float64, device=dev),
                        F=rep(torch.eye(3, dtype=torch.float64, device=dev)[None].repeat(N, 1, 1)),
                        prim_pos=rep(f64(cfg.prim_init_pos)),
                        softness=torch.full((B, self.n_primitive), float(cfg.softness), dtype=torch.float64, device=dev),   # set_softness()
                        E=torch.full((B,), float(cfg.E), dtype=torch.float64, device=dev),
                        nu=torch.full((B,), float(cfg.nu), dtype=torch.float64, device=dev),
                        yield_stress=torch.full((B,), float(cfg.yield_stress), dtype=torch.float64, device=dev),
                        prim_rot=rep(f64([tuple(q) for q in list(cfg.prim_rot)[:self.n_primitive]])) if self.rot_state else None,
                        prim_gap=rep(f64((list(getattr(cfg, "prim_init_gap", ())) + [0.0, 0.0])[:self.n_primitive])) if self.chopsticks else None)

    def step(self, state: PlbState, action) -> PlbState:
        """TaichiEnv.step(action) in copy mode: one call = `substeps` substeps for every env.  Differentiable: when any of
        the state tensors / the action / E / nu / yield_stress requires grad, the forward keeps a checkpoint and backward()
        runs the adjoint kernels (substep_grad)."""
        B = state.x.shape[0]
        if self.chopsticks:     # action [B,7 (+ action_dim1)]; orientation and gap are stepped with the position
            action = torch.as_tensor(action, dtype=torch.float64, device=self.device).reshape(B, self.action_dim)
            xo, vo, Co, Fo, po, ro, go = _PlbStepGap.apply(self, state.x, state.v, state.C, state.F, state.prim_pos, state.prim_rot, state.prim_gap,
                                                           state.softness, action, state.E, state.nu, state.yield_stress)
            return state._replace(x=xo, v=vo, C=Co, F=Fo, prim_pos=po, prim_rot=ro, prim_gap=go)
        if self.rot_state:      # action [B,action_dim]; the orientation is stepped with the position
            action = torch.as_tensor(action, dtype=torch.float64, device=self.device).reshape(B, self.action_dim)
            xo, vo, Co, Fo, po, ro = _PlbStepRot.apply(self, state.x, state.v, state.C, state.F, state.prim_pos, state.prim_rot, state.softness,
                                                       action, state.E, state.nu, state.yield_stress)
            return state._replace(x=xo, v=vo, C=Co, F=Fo, prim_pos=po, prim_rot=ro)
        action = torch.as_tensor(action, dtype=torch.float64, device=self.device).reshape(B, self.action_dim)
        if self._host_scale is not None:
            action = action.clamp(-1.0, 1.0) * self._host_scale
        xo, vo, Co, Fo, po = _PlbStep.apply(self, state.x, state.v, state.C, state.F, state.prim_pos, state.softness, action,
                                            state.E, state.nu, state.yield_stress)
        return state._replace(x=xo, v=vo, C=Co, F=Fo, prim_pos=po)

    def compute_loss(self, state: PlbState, target_density, target_sdf, weights=(1.0, 1.0, 1.0), soft_contact=True):
        """Loss.compute_loss_kernel (engine/losses/loss.py:190-214): (loss [B], parts [B,3] = contact, density, sdf).
        target_density / target_sdf: [n_grid, n_grid, n_grid] float64; weights = (contact, density, sdf) as in :158-162."""
        td = torch.as_tensor(target_density, dtype=torch.float64, device=self.device).reshape(-1).contiguous()
        ts = torch.as_tensor(target_sdf, dtype=torch.float64, device=self.device).reshape(-1).contiguous()
        assert td.numel() == self.n_grid ** 3 == ts.numel()
        wt = torch.as_tensor(weights, dtype=torch.float64, device=self.device).reshape(3).contiguous()
        if self.chopsticks:
            return _PlbLossGap.apply(self, state.x, state.prim_pos, state.prim_rot, state.prim_gap, td, ts, wt, bool(soft_contact))
        if self.rot_state:
            return _PlbLossRot.apply(self, state.x, state.prim_pos, state.prim_rot, td, ts, wt, bool(soft_contact))
        return _PlbLoss.apply(self, state.x, state.prim_pos, td, ts, wt, bool(soft_contact))

    def get_grid_mass(self, state: PlbState):
        """TaichiEnv.get_grid_mass: the loss's grid mass of the state, [B, n_grid, n_grid, n_grid] (ud_plb_grid_mass).  A goal's target
        density is this field of the goal state.  No gradient."""
        x = _c(state.x)
        B, n = x.shape[0], self.n_grid
        gm = torch.empty((B, n, n, n), dtype=torch.float64, device=x.device)
        stream = _lib.stream(x.device)
        _lib.check(_lib.lib().ud_plb_grid_mass(self._h, B, _lib.ptr(x), _lib.ptr(gm), stream), "ud_plb_grid_mass")
        return gm

    def density_seq_loss(self, x, targets, index=None, work_bytes=None):
        """The identification loss of a sequence of clouds (sim2sim / real2sim compute_loss with new_target_density[f]; ud_plb_density_seq_*):
        x [..., N, 3]; targets [T, n, n, n]; index: the target of every cloud, x's leading shape (None = target 0).  Returns
        sum_I |grid_mass(x)_I - targets[index]_I| in x's leading shape, differentiable in x.  The number of clouds is not bound by
        batch_size.  An index outside [0, T) gives NaN and no gradient.  work_bytes: the scratch of the forward (None = the library's
        choice); it is taken in chunks of work_bytes / (8 n^3) clouds."""
        n, N = self.n_grid, self.n_particles
        assert x.shape[-2:] == (N, 3), tuple(x.shape)
        lead = tuple(x.shape[:-2])
        td = torch.as_tensor(targets, dtype=torch.float64, device=self.device)
        assert td.dim() == 4 and tuple(td.shape[1:]) == (n, n, n), tuple(td.shape)
        td = td.detach().reshape(td.shape[0], -1).contiguous()
        xf = x.reshape(-1, N, 3)
        idx = None
        if index is not None:
            idx = torch.as_tensor(index, device=self.device).to(torch.int32).reshape(-1).contiguous()
            assert idx.numel() == xf.shape[0], (tuple(idx.shape), lead)
        return _PlbDensitySeq.apply(self, xf, td, idx, work_bytes).reshape(lead)

    def chamfer(self, a, b, index=None, return_mins=False):
        """Chamfer distance (solver.py:187-196; ud_plb_chamfer): a [..., Na, 3]; b [Nb, 3] or [Tb, Nb, 3]; index: the cloud of b every cloud of a is
        held against (None = cloud 0).  mean_i min_j |a_i - b_j| + mean_j min_i |a_i - b_j| in a's leading shape; no gradient.
        return_mins: also the two sets of minima [..., Na] and [..., Nb]."""
        a = torch.as_tensor(a, dtype=torch.float64, device=self.device).detach()
        b = torch.as_tensor(b, dtype=torch.float64, device=self.device).detach()
        if b.dim() == 2:
            b = b[None]
        assert a.shape[-1] == 3 and b.dim() == 3 and b.shape[-1] == 3, (tuple(a.shape), tuple(b.shape))
        lead, Na, (Tb, Nb) = tuple(a.shape[:-2]), a.shape[-2], b.shape[:2]
        af, b = a.reshape(-1, Na, 3).contiguous(), b.contiguous()
        M = af.shape[0]
        idx = None
        if index is not None:
            idx = torch.as_tensor(index, device=self.device).to(torch.int32).reshape(-1).contiguous()
            assert idx.numel() == M
        out = torch.empty((M,), dtype=torch.float64, device=self.device)
        # always given: with both arrays the minima are taken by many workgroups per item (include/unidom_hip.h)
        mab = torch.empty((M, Na), dtype=torch.float64, device=self.device)
        mba = torch.empty((M, Nb), dtype=torch.float64, device=self.device)
        stream = _lib.stream(self.device)
        _lib.check(_lib.lib().ud_plb_chamfer(M, int(Na), _lib.ptr(af), int(Tb), int(Nb), *[_lib.ptr(t) for t in (b, idx, out, mab, mba)],
                                             stream), "ud_plb_chamfer")
        if return_mins:
            return out.reshape(lead), mab.reshape(lead + (Na,)), mba.reshape(lead + (Nb,))
        return out.reshape(lead)

    def render(self, state: PlbState, spp=None, seed=0, mode="rgb_array", render_conf=None, color=None, strict=True):
        """TaichiEnv.render (taichi_env.py:88-94) of every env of `state`: engine/plb_render.py's PlbRenderer, created on the first call from
        the conf's RENDERER overrides (or `render_conf`) and kept.  uint8 [B,H,W,3] ("rgb_array") or the f32 image ("float"); color and strict
        as PlbRenderer.render takes them.  Passing a `render_conf` OBJECT other than the one the kept renderer was made from (compared by
        identity, not by value) frees that renderer's arenas and creates a new one: keep one RenderConf and pass it every time, or none."""
        from .plb_render import PlbRenderer
        if getattr(self, "_renderer", None) is None or (render_conf is not None and render_conf is not self._renderer.conf):
            self._renderer = PlbRenderer(self.cfg, render_conf, self.batch_size, self.device)
        return self._renderer.render(state, spp=spp, seed=seed, mode=mode, color=color, strict=strict)

    @staticmethod
    def set_softness1(state: PlbState, softness) -> PlbState:   # primitives.py: Primitives.set_softness1
        so = state.softness.clone()
        so[:, 0] = softness
        return state._replace(softness=so)
