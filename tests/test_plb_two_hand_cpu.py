"""Both primitives actuated on the PLB f64 path: the torch restatement the HIP kernels are held to (tests/plb_multi_twin.py) against the
twins it extends, central differences and a serial NumPy kinematics.  No GPU."""
import numpy as np
import pytest
import torch

from oracle.twin.plb_twin import PlbConf
from tests import plb_two_hand_cases as K
from tests.plb_chopsticks_twin import PlbChopsticksTwin
from tests.plb_multi_twin import PlbTwoHandRotTwin, kinematics_numpy
from tests.plb_prim_twin import PlbPrimTwin
from tests.plb_rot_twin import PlbRotTwin
from tests.plb_shape_twin import PlbShapeTwin

S2 = 2          # substeps of the CPU runs: the chain rule across a substep boundary is in, the cost stays low


def _conf(c):
    return PlbConf(quality=0.5, n_particles=c["N"], radius=tuple(c["radius"]), upper_bound=tuple(c["upper"]))


def _parent(c, name):
    """The existing twin of the case's legacy handle (primitive 1 unactuated)."""
    if name == "prim":
        return PlbPrimTwin(_conf(c), kinds=c["kinds"], h=c["h"], rot=c["const_rot"], mu=c["mu"], action_scale=c["scale"], substeps=S2)
    if name == "rot":
        return PlbRotTwin(_conf(c), kinds=c["kinds"], h=c["h"], mu=c["mu"], action_scale=c["scale"], action_scale_w=c["scale_w"],
                          action_dim=c["action_dim"], substeps=S2)
    if name == "shape":
        return PlbShapeTwin(_conf(c), kinds=c["kinds"], shape=c["shape"], h=c["h"], rot=c["const_rot"], mu=c["mu"], action_scale=c["scale"],
                            action_scale_w=c["scale_w"], action_dim=c["action_dim"], substeps=S2, rot_state=c["rot_state"])
    return PlbChopsticksTwin(_conf(c), kinds=c["kinds"], h=c["h"], mu=c["mu"], min_gap=c["min_gap"], action_scale=c["scale"],
                             action_scale_w=c["scale_w"], action_scale_gap=c["scale_gap"], substeps=S2)


def _mine(c, name):
    if name == "rot":           # twin_of picks the shape twin for a rot_state handle; the rot subclass is held to its parent here
        return PlbTwoHandRotTwin(_conf(c), kinds=c["kinds"], h=c["h"], mu=c["mu"], action_scale=c["scale"], action_scale_w=c["scale_w"],
                                 action_dim=c["action_dim"], substeps=S2, action_dim1=c["action_dim1"], action_scale1=c["scale1"],
                                 action_scale_w1=c["scale_w1"])
    return K.twin_of(c, substeps=S2)


def _run(tw, c, grad=()):
    leaves = {k: K.T(c[k], k in grad) for k in K.state_names(c) + ("act", "E", "nu", "ys")}
    return leaves, K.twin_step(tw, c, leaves)


# the legacy handles the parents can express: primitive 1 a sticky Sphere on rot_state, anything PlbPrimTwin / PlbShapeTwin take without it
LEGACY = {"prim": lambda: K.spheres(33), "rot": lambda: K.rot_pair(33, "cap6_sph3"), "shape": lambda: K.capsule_box(33),
          "shape_rot": lambda: K.rot_pair(33, "cap6_sph3"), "chop": lambda: K.chop_sphere(33)}


@pytest.mark.parametrize("name", sorted(LEGACY))
def test_unactuated_and_zero_block_are_the_existing_twins(name):
    """action_dim1 = 0: the new twin returns exactly what the twin it extends returns; action_dim1 = 3 with a zero block: the same."""
    torch.set_num_threads(4)
    c = LEGACY[name]()
    kind = name.split("_")[0]
    legacy, zero = K.legacy_of(c), K.zero_block_of(c)
    with torch.no_grad():
        want = _run(_parent(legacy, kind), legacy)[1]
        got0 = _run(_mine(legacy, kind), legacy)[1]
        got3 = _run(_mine(zero, kind), zero)[1]
    assert float((want[1] - K.T(c["v"])).abs().max()) > 0 and float((want[4] - K.T(c["prim"])).abs().max()) > 0
    for n, w, a, b in zip(K.state_names(c), want, got0, got3):
        assert torch.equal(w, a), (name, n, "action_dim1 = 0")
        assert torch.equal(w, b), (name, n, "zero block")


FD_CASES = {"spheres": lambda: K.spheres(33), "capsule_box": lambda: K.capsule_box(33), "cap6_cap6": lambda: K.rot_pair(33, "cap6_cap6"),
            "pin_cap3": lambda: K.rot_pair(33, "pin_cap3"), "cap6_box6": lambda: K.rot_pair(33, "cap6_box6"), "chop": lambda: K.chop_sphere(33)}


@pytest.mark.parametrize("name", sorted(FD_CASES))
def test_autograd_in_primitive_1s_block_is_the_derivative(name):
    """Central differences in every component of primitive 1's action block (env 0), through two substeps (the Chopsticks case: its own
    three, for which its gaps were chosen): h = 1e-6, |fd - an| < 1e-5 max(1, |an|), the rule of test_torch_twin_is_the_numpy_twin_and_its_autograd_is_the_derivative.  A
    difference means something only while both of its runs take the same contact branches (a cell that changes arm between -h and +h adds
    an O(1) jump over 2h): the number of active and of sliding cells per substep and primitive is asserted equal on both sides."""
    torch.set_num_threads(4)
    c = FD_CASES[name]()
    rng = np.random.default_rng(5)
    w = [rng.normal(size=np.shape(c[k])) for k in K.state_names(c)]
    value = lambda out: sum((o * K.T(wi)).sum() for o, wi in zip(out, w))
    S = c["substeps"] if c["chop"] else S2
    tw = K.twin_of(c, substeps=S)
    leaves, out = _run(tw, c, grad=("act",))
    K.check_honesty(tw, c)
    value(out).backward()
    A0, A = c["action_dim"], c["act"].shape[1]
    entries = [("act", (0, d)) for d in range(A0, A)]
    h = 1e-6
    arms = lambda t: [(int((d["occ"] & d["active"]).sum()), int((d["occ"] & d["active"] & d["flag"]).sum())) for d in t.diag]
    for key, idx in entries:
        up, dn = dict(c), dict(c)
        up[key], dn[key] = c[key].copy(), c[key].copy()
        up[key][idx] += h
        dn[key][idx] -= h
        tu, td = K.twin_of(up, substeps=S), K.twin_of(dn, substeps=S)
        with torch.no_grad():
            fd = (float(value(_run(tu, up)[1])) - float(value(_run(td, dn)[1]))) / (2 * h)
        assert arms(tu) == arms(td), (name, key, idx)
        an = float(leaves[key].grad[idx])
        assert an != 0.0, (key, idx)
        assert abs(fd - an) < 1e-5 * max(1.0, abs(an)), (name, key, idx, fd, an)


@pytest.mark.parametrize("name", ["cap6_cap6", "cap6_sph3", "cap6_box6", "pin_cap3", "chop", "spheres"])
def test_kinematics_alone_against_serial_numpy(name):
    """Primitive 1's trajectory over a whole step, one env and primitive at a time in NumPy (as the device's prologue thread runs it), against
    the twin's kinematics: 1e-14 absolute and 1e-12 relative, the bar of tests/test_plb_rot_gpu.py's header.  One env clipped at +-1 and one
    that meets upper_bound in y."""
    c = {"chop": K.chop_sphere, "spheres": K.spheres}.get(name, lambda N: K.rot_pair(N, name))(33)
    A0, d1, S = c["action_dim"], c["action_dim1"], c["substeps"]
    act = c["act"].copy()
    act[1, A0] = -1.3                                                    # outside the clip
    act[2, A0 + 1] = 0.8                                                 # a large move up (every scale1 here is 1) ...
    c = dict(c, act=act, upper=(1.0, float(c["prim"][2, 1, 1] + 0.1), 1.0))   # ... into a bound 0.1 above env 2's primitive 1
    tw = K.twin_of(c)
    a = torch.clamp(K.T(act), -1, 1)
    pos, rot = K.T(c["prim"]), K.T(c["rot"] if c["rot_state"] else np.tile([1.0, 0.0, 0.0, 0.0], (K.B, 2, 1)))
    gap = K.T(c["gap"]) if c["chop"] else None
    P, R = [pos[:, 1].numpy()], [rot[:, 1].numpy()]
    lo, hi = torch.tensor(c["lower"] if "lower" in c else (0.0, 0.0, 0.0), dtype=torch.float64), torch.tensor(c["upper"], dtype=torch.float64)
    for _ in range(S):
        if c["chop"]:
            pos, rot, gap = tw.kinematics(pos, rot, gap, a)
        elif c["rot_state"]:
            pos, rot = tw.kinematics(pos, rot, a)
        else:                                                            # the plain step has no kinematics function: its one line
            pv = torch.stack([a[:, :3] * tw.action_scale / S, tw.block1(a)[0]], 1)
            pos = torch.maximum(torch.minimum(pos + pv, hi), lo)
        P.append(pos[:, 1].numpy())
        R.append(rot[:, 1].numpy())
    P, R = np.stack(P, 1), np.stack(R, 1)                                # [B,S+1,..]
    hit = False
    for b in range(K.B):
        Pn, Rn = kinematics_numpy(c["prim"][b, 1], R[b, 0], act[b, A0:A0 + d1], c["scale1"], c["scale_w1"], S, lo.numpy(), hi.numpy())
        hit |= bool((Pn[:, 1] == c["upper"][1]).any())
        np.testing.assert_allclose(P[b], Pn, rtol=1e-12, atol=1e-14)
        if c["rot_state"]:
            np.testing.assert_allclose(R[b], Rn, rtol=1e-12, atol=1e-14)
            assert (d1 != 6) or np.abs(Rn[-1] - Rn[0]).max() > 1e-4     # it turned
    assert hit and np.abs(P[:, -1] - P[:, 0]).max() > 1e-3
