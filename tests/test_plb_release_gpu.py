"""GPU: algorithms/plb_release.py (the Torus branch of the reference's solve_action) cut down to 13 actions and two envs, against a plain
step loop written here with the same parameters and the same softness switch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

APPROACH, HOLD, TAIL, VERSION = 6, 3, 4, 1


def test_release_small(tmp_path):
    from unidom_amd.algorithms import plb_release
    from unidom_amd.engine.plb_simulator import PlbSimulator, TorusConf
    out = tmp_path / "torus.npz"
    res = plb_release.main(["--env", "torus", "--num_envs", "2", "--version", str(VERSION), "--approach", str(APPROACH), "--hold", str(HOLD),
                            "--tail", str(TAIL), "--image_res", "24", "16", "--spp", "1", "--out", str(out)])
    # the plain loop: solver.py:127-144 and :299-331 typed out
    conf = TorusConf()
    sim = PlbSimulator(conf, batch_size=2)
    st = sim.reset()
    E, nu = [], []
    for i in range(2):
        rs = np.random.RandomState(VERSION * 1000 + i)
        E.append(rs.uniform(500, 10500)); nu.append(rs.uniform(0.2, 0.4))
    f64 = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")
    st = st._replace(E=f64(E), nu=f64(nu), yield_stress=f64([200.0, 200.0]))
    p0, start = np.array(conf.prim_init_pos[0]), np.array([0.2, 0.3, 0.5])
    pts = np.linspace(p0, start, APPROACH)
    actions = np.concatenate([np.diff(pts, axis=0), np.diff(pts, axis=0)[:1], np.zeros((HOLD + TAIL, 3))])
    assert actions.shape == (13, 3)
    bottom = [int(np.argmin(st.x[b, :, 1].cpu().numpy())) for b in range(2)]
    best, best_at, release_point = [0.0, 0.0], [-1, -1], None
    with torch.no_grad():
        for idx, act in enumerate(actions):
            st = sim.step(st, f64(np.stack([act, act])))
            if idx == APPROACH + HOLD - 1:
                release_point = st.prim_pos[:, 0].cpu().numpy().copy()
                st = sim.set_softness1(st, 0.0)
            for b in range(2):
                x = float(st.x[b, bottom[b], 0])
                if x > best[b]:
                    best[b], best_at[b] = x, idx
    sim.check_status()
    print(f"max_x {best} reached after action {best_at}; release() gave {res['max_x'].tolist()}; "
          f"largest |x - x'| of the two final states {float((res['state'].x - st.x).abs().max()):.3e}")
    assert np.array_equal(res["release_point"], release_point) and res["release_point"].shape == (2, 3)
    assert np.array_equal(res["max_x"], np.array(best)) and (res["max_x"] > 0.4).all()
    assert np.array_equal(res["action"], actions) and np.array_equal(res["E"], np.array(E)) and np.array_equal(res["Poisson"], np.array(nu))
    # the particles of two rollouts agree to the last bits only (the step's grid sums are f64 atomics, in arrival order): 1e-9 of a unit box
    # is a million times that and a million times below anything a wrong action, parameter or release step would move
    assert float((res["state"].x - st.x).abs().max()) < 1e-9
    assert float(res["state"].softness[0, 0]) == 0.0 and float(res["state"].softness[0, 1]) == 666.0
    # the Sphere was carried to start_pos and stayed there; both envs' Spheres move alike, their rods do not (E and nu differ)
    assert np.abs(release_point - (start + np.diff(pts, axis=0)[0])).max() < 1e-12 and np.array_equal(release_point[0], release_point[1])
    assert E[0] != E[1] and nu[0] != nu[1] and not torch.equal(st.x[0], st.x[1])
    assert bool(torch.isfinite(st.x).all())
    # one frame, the final state's, under torus.yml's light; and the file
    assert res["frames"].shape == (1, 2, 16, 24, 3) and res["frames"].dtype == np.uint8 and res["frames"].any() and res["frame_steps"].tolist() == [12]
    z = np.load(out)
    assert {"release_point", "max_x", "action", "E", "Poisson", "yield_stress", "env_name"} <= set(z.files)
    assert np.array_equal(z["release_point"], res["release_point"]) and np.array_equal(z["max_x"], res["max_x"]) and str(z["env_name"]) == "Torus-v1"
    assert np.array_equal(z["yield_stress"], np.array([200.0, 200.0])) and z["action"].shape == (13, 3)


def test_release_renders_every_nth_action():
    from unidom_amd.algorithms.plb_release import release
    from unidom_amd.engine.plb_render import render_conf_of
    from unidom_amd.engine.plb_simulator import TorusConf
    conf = TorusConf()
    rc = render_conf_of(conf, image_res=(24, 16), spp=1, voxel_res=(72, 96, 40))      # the dragged rod spans 0.3 in x: 45 cells and the margin
    res = release(conf, 2, VERSION, APPROACH, HOLD, TAIL, frames_every=5, render_conf=rc)
    assert res["frame_steps"].tolist() == [0, 5, 10] and res["frames"].shape == (3, 2, 16, 24, 3)
    assert not np.array_equal(res["frames"][0], res["frames"][2])
