#!/usr/bin/env python3
"""bench.py -- headline benchmark of the hot path on MI355X (contract: see the task statement / DESIGN.md).

Metric (BASELINE.json): differentiable-physics substeps/sec, forward + backward, on `fold_cloth1` with
num_envs=4 per GPU, ep_len=3 (the reference's `apg_no_para --env fold_cloth1 --ep_len 3 --num_envs 4` iteration;
fold_cloth1 is the mass-spring cloth simulator).  One "step" = one full APG update:
policy forward, 3 x env.step_diff (each 40 macro actions x 50 substeps inside ONE kernel launch), loss,
backward through everything (the adjoint kernel streams the per-substep checkpoints back), gradient
nan_to_num + clip, the RCCL all-reduce of the flat policy gradient when N > 1, and the Adam step.

    python bench.py --gpus 1 --steps 5 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
    python bench.py --gpus N ...        # no RANK in the environment: bench.py starts that torch.distributed.run itself

Weak scaling: every rank owns 4 envs; `value` is the whole-job aggregate.  Rank 0 prints ONE JSON line.

A plain run of the headline line does only what `value` needs: set up, warm up, time --steps updates, print the line.  `--full` adds
the forward-only rate, the same update in the reference's operation order (`reference_order`), the many-env saturation probe and the
CPU baselines.  `--dump-outputs DIR` writes what the last timed update computed as DIR/<name>.npy (float32).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

NUM_ENVS_PER_GPU = 4
EP_LEN = 3
MACRO, SUBSTEPS, P = 40, 50, 512
# algorithmic bytes per env-substep (recompute passes not counted)
BYTES_FWD = 48 * P     # read x,v + write x,v
BYTES_BWD = 72 * P     # read saved x,v + read g_x,g_v + write g_x,g_v
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s


def self_launch(argv):
    """`--gpus N` (N > 1) without RANK in the environment: start the N ranks ourselves -- one child
    `python -m torch.distributed.run --nproc-per-node N bench.py <same flags>` -- BEFORE this process makes any GPU call,
    relay rank 0's single JSON line, and exit non-zero if the launcher or any rank does (the reference: one process driving
    `--gpus` devices through jax.pmap, apg.py:83-85, :269-271)."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    n = int(argv[argv.index("--gpus") + 1]) if "--gpus" in argv else int([a for a in argv if a.startswith("--gpus=")][0].split("=")[1])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    for ln in r.stdout.splitlines():
        if ln not in lines:
            print(ln, file=sys.stderr)
    if r.returncode != 0 or len(lines) != 1:
        print(f"bench.py: the {n}-rank launch failed (exit code {r.returncode}, {len(lines)} result lines)", file=sys.stderr)
        raise SystemExit(r.returncode or 1)
    print(lines[0], flush=True)
    raise SystemExit(0)


def bench_selftest(args, rank, world, device):
    """The N-rank plumbing of this file without a simulator: init_distributed, the barrier-bracketed timed region, the
    max-over-ranks timing, the per-update gradient all-reduce of GradSync, rank 0's single JSON line.  Used by the CPU test
    (gloo, 2 ranks, UNIDOM_DIST_BACKEND=gloo); it measures nothing about the hot path."""
    from unidom_amd.algorithms.apg.core import GradSync, Policy
    pol = Policy(32, 6, hidden=(64, 32), seed=0).to(device)
    sync = GradSync(pol, 1e-3, 0.3)
    x = torch.linspace(-1, 1, 4 * 32, device=device).reshape(4, 32) * (1 + rank)

    def one():
        sync.zero_grad()
        (pol(x) ** 2).sum().backward()
        sync.step()

    grouped = dist.is_initialized()     # world > 1, or a one-rank group joined on purpose (UNIDOM_DIST_JOIN_SINGLE=1: the RCCL smoke test)

    def barrier():
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        if grouped:
            dist.barrier()

    for _ in range(args.warmup):
        one()
    sync.profile = []
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one()
    barrier()
    dt_rank = time.perf_counter() - t0
    tm = torch.tensor([dt_rank], device=device, dtype=torch.float64)
    if grouped:
        dist.all_reduce(tm, op=dist.ReduceOp.MAX)
    ranks = rank_report(world, device, dt_rank, None, sync)
    flat = torch.cat([p.detach().reshape(-1) for p in pol.parameters()])
    same = torch.ones((), device=device)
    probe_ok = None
    if grouped:
        lo, hi = flat.clone(), flat.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        same = (lo == hi).all().float()
        probe = torch.arange(1, 1025, device=device, dtype=torch.float32) * (1 + rank)      # known answer: sum over ranks = i * W (W + 1) / 2
        dist.all_reduce(probe, op=dist.ReduceOp.SUM)
        probe_ok = bool((probe == torch.arange(1, 1025, device=device, dtype=torch.float32) * (world * (world + 1) // 2)).all().item())
    ar_ms = sync.allreduce_ms()
    if rank == 0:
        print(json.dumps({"metric": "selftest_updates_per_sec", "value": world * args.steps / float(tm[0]), "unit": "updates/s",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": float(tm[0]) / args.steps * 1e3,
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                          "config": {"workload": "selftest (no simulator): policy gradient all-reduce + Adam"},
                          "n_ranks_seen": dist.get_world_size() if dist.is_initialized() else 1,
                          "allreduce_bytes_per_update": sync.n_params * 4 if world > 1 else 0,
                          "replicas_identical": bool(same.item()),
                          "collective": {"backend": dist.get_backend() if grouped else None, "device": str(device), "known_answer_allreduce_ok": probe_ok,
                                         "gradient_allreduces_timed": len(ar_ms), "gradient_allreduce_ms_mean": float(np.mean(ar_ms)) if ar_ms else None,
                                         "HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")}, **ranks}), flush=True)
    if grouped:
        dist.barrier()
        dist.destroy_process_group()


def rank_report(world, device, dt, k_ms=None, sync=None):
    """What makes an N-rank line explain itself (the first hardware run happens at round end, on a node this session never sees): per rank
    the wall time of the timed region, the mean kernel time of the simulator's forward / adjoint launches (HIP events on the launch stream)
    and the mean time of the one collective per update (events / perf_counter around dist.all_reduce in GradSync.step) -- gathered with ONE
    all_gather after the timed region.  `value` is still units / max-over-ranks time; a spread between max and min rank time, or an
    all-reduce time far above 3.7 MB / link bandwidth, says where a poor scaling figure comes from."""
    if world <= 1:
        return {}
    ar = sync.allreduce_ms() if sync is not None else []
    mine = torch.tensor([dt, (k_ms or {}).get("fwd", float("nan")), (k_ms or {}).get("bwd", float("nan")),
                         float(np.mean(ar)) if ar else float("nan"), float(np.max(ar)) if ar else float("nan")], device=device, dtype=torch.float64)
    allr = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(allr, mine)
    rows = torch.stack(allr).cpu().numpy()
    fin = lambda col: [None if not np.isfinite(v) else float(v) for v in rows[:, col]]
    return {"ranks": {"time_s": {"max": float(rows[:, 0].max()), "min": float(rows[:, 0].min()), "per_rank": fin(0)},
                      "kernel_ms": {"fwd": fin(1), "bwd": fin(2)}, "allreduce_ms": {"mean": fin(3), "max": fin(4)},
                      "note": "per rank, in rank order; value = units / time_s.max"}}


def dist_info(world, allreduce_params=0):
    """What the line says about the N-rank run: the world size torch.distributed reports (not the flag), and the bytes of the
    one collective per update (the policy-gradient mean, apg.py:235); 0 for simulator-only workloads (replicas, no collective)."""
    return {"n_ranks_seen": dist.get_world_size() if dist.is_initialized() else 1,
            "allreduce_bytes_per_update": allreduce_params * 4 if world > 1 else 0}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every array as out_dir/<name>.npy in float32 (the tensors come off the device here, after the timed region), so that
    two builds run with the same arguments -- hence the same seeds and inputs -- can be compared output for output."""
    host = {k: torch.as_tensor(v).detach().float().cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in host.values())
    if total > DUMP_LIMIT_BYTES:
        raise ValueError(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(out_dir, exist_ok=True)
    for k, a in host.items():
        np.save(os.path.join(out_dir, f"{k}.npy"), a)


def lg_label(dom, sim, B):
    """kernels of the many-workgroup MPM path for this call shape, as the library reports them (ud_mpm_launch_plan): forward = one
    persistent launch per step call (parts of 32 particles handing grid cells to each other through HBM) or clear+FK, p2g, grid op, g2p
    per substep; backward with the grid checkpoint = two launches per substep (grid-op adjoint || restore; p2g adjoint -> g2p adjoint)
    or four (restore, g2p adjoint, grid-op adjoint, p2g adjoint); six when it recomputes the grid"""
    plan = sim.launch_plan(B)
    if dom == "fwd":
        return "mpm many-workgroup path (fwd: clm_fwd_kernel, one persistent launch per step call)" if plan & 2 else "mpm many-workgroup path (fwd: 2 kernels/substep)"
    n = (2 if plan & 4 else 4) if sim.grid_ckpt_cells > 0 else 6
    return f"mpm many-workgroup path (bwd: {n} kernels/substep)"


def lg_issue(key, kernel_ms):
    """instruction-issue roof of the many-workgroup kernels of one step call: VALU + SALU wave-instructions of all its launches (PMC pass,
    tools/pmc_large.sh) per second / what 256 CUs can issue -- they are VALU-bound where they are not latency-bound"""
    r = issue_roof(key, kernel_ms, None, 256, None)
    if r:
        r["note"] = "all launches of one step call; 256 CUs x 4 SIMDs x 0.6 G wave-instr/s"
    return r


def plb_issue(key, step_ms):
    """instruction-issue roof of the PlasticineLab lines: VALU + SALU wave-instructions of every plb_* launch of one bench step (PMC pass,
    tools/pmc_plb.sh) / the step's wall time / what 256 CUs can issue.  8 envs x 1000 particles occupy a fraction of the chip's wave slots, so
    this fraction is small by construction; what it says is that neither HBM nor issue binds these lines -- latency of one wave's chain does."""
    r = issue_roof(key, step_ms, None, 256, None)
    if r:
        r["note"] = "all plb_* launches of one bench step over the step's wall time; 256 CUs x 4 SIMDs x 0.6 G wave-instr/s"
    return r


def pmc_traffic(key):
    """HBM bytes per launch from the committed counter passes (profiles/pmc_traffic.json), or None when there is no
    entry or the kernel sources have changed since the passes were taken (the entry carries their hash)."""
    tj = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if not os.path.exists(tj):
        return None
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import src_hash
    e = json.load(open(tj)).get(key)
    if not e or e.get("src_sha16") != src_hash.sha16(key):
        return None
    return e.get("hbm_bytes_per_launch")


VALU_CLOCK_HZ = 2.4e9     # MI355X_MICROARCH.md: a SIMD issues one wave64 VALU instruction per 4 clocks -> 0.6e9 per SIMD and second at the peak clock
# static VALU + SALU wave-instructions per wave-substep of the one-workgroup cloth kernels (tools/asm_loop_stats.py on the inner loops,
# DESIGN.md 3.1) -- used ONLY when profiles/pmc_traffic.json holds no SQ_INSTS_* pass for the current sources (see issue_roof)
STATIC_INSTR_PER_SUBSTEP = {"cloth_rollout_fwd_v2_kernel": 392, "cloth_rollout_bwd_fast_kernel": 707}


def issue_roof(kname, kernel_ms, waves, busy_cus, substeps):
    """What bounds a one-workgroup-per-env kernel is instruction issue on the few CUs it occupies, not HBM: `frac` = wave-instructions
    the launch executes per second / what the busy SIMDs can issue (busy CUs x 4 SIMDs x clock / 4).  ONE count for every launch shape:
    the EXECUTED VALU + SALU wave-instructions of the SQ_INSTS_* counter pass (SALU shares the issue port with VALU at 2 waves per SIMD,
    DESIGN.md 3.1) in profiles/pmc_traffic.json, taken on the headline shape and scaled by waves of this launch / SQ_WAVES of the pass
    (every env runs the same substeps: the count per wave does not depend on how many envs a launch holds).  Only when there is no pass
    for the current sources: the static count of the inner loop, which also counts the blocks a wave-uniform branch skips at run time
    (no lane on the ground, no lane grasped) and therefore overstates the executed count (707 static vs 541 executed per wave-substep in
    the cloth adjoint) -- `source` says which one a line carries."""
    tj = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    src, per_launch = None, None
    if os.path.exists(tj):
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import src_hash
        e = json.load(open(tj)).get(kname) or {}
        if e.get("insts") and e.get("src_sha16") == src_hash.sha16(kname):
            per_launch = e["insts"].get("SQ_INSTS_VALU", 0.0) + e["insts"].get("SQ_INSTS_SALU", 0.0)
            pass_waves = int(e["insts"].get("SQ_WAVES", 0))
            src = "rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU (profiles/pmc_traffic.json)"
            if waves and pass_waves and waves != pass_waves:
                per_launch *= waves / pass_waves
                src += f", scaled from the pass's {pass_waves} waves to this launch's {waves}"
            waves = waves or pass_waves
    if per_launch is None and kname in STATIC_INSTR_PER_SUBSTEP and waves and substeps:
        per_launch = STATIC_INSTR_PER_SUBSTEP[kname] * waves * substeps
        src = "static count of the inner loop (tools/asm_loop_stats.py) x waves x substeps: an upper bound of the executed count"
    if per_launch is None:
        return None
    rate = per_launch / (kernel_ms * 1e-3)
    peak = busy_cus * 4 * VALU_CLOCK_HZ / 4
    out = {"bound": "valu_issue", "wave_instructions_per_launch": per_launch, "achieved": rate / 1e9, "peak": peak / 1e9, "unit": "G wave-instr/s",
           "frac": rate / peak, "busy_cus": busy_cus, "waves": waves, "source": src,
           "note": "the binding roof of this kernel: one workgroup per env, the substeps of a launch are sequential (see roofline.note)"}
    if waves and substeps:
        out["per_wave_substep"] = per_launch / waves / substeps
    return out


def host_cores():
    """Cores this process may really use: the smaller of the affinity mask and the cgroup CPU quota (a GPU box shows 256 logical CPUs but
    gives one GPU's job a share of 16: round 2's "all cores" leg started 256 threads on them and scaled 8x -- that was the quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(float(txt[0]) / float(txt[1]) + 0.5)))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, int(q / per + 0.5)))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


def cpu_baseline(sample_envs=4, ep_len=EP_LEN, gpu_order=2):
    """Oracle (CPU restatement, NOT JAX-CPU), rebuilt here with -O3 -march=native, timed on the host cores: forward + adjoint
    of the headline workload (4 envs x ep_len step_diffs) on min(4, nproc) threads, the same on ONE thread, and nproc envs on
    nproc threads (all cores busy) -- in BOTH operation orders the restatement has: order 1 = the reference's literal order
    (cloth_simulator.py:264-268: k*r/len*(len-L0)/L0, 48 IEEE divisions + 10 sqrt per particle-substep), order 2 = the
    re-associated order "v2" the default GPU forward runs (8 divisions).  `value` is the order the GPU leg of this line ran
    (`gpu_order`), so the stated baseline is like for like; the other order sits beside it under `reference_order` / `v2_order`.
    The oracle is only the thing timed here, never the product path."""
    from oracle import pyoracle
    from tests.conftest import fold_cloth1_mask, make_cloth_case
    build = "-O3 -march=native built on this host"
    try:
        pyoracle.use_native()
    except Exception as e:      # no compiler on this host: time the portable build that travelled with the repo, and say so
        build = f"-O3 baseline x86-64 (the native rebuild failed: {type(e).__name__})"
    nproc = host_cores()

    def legs(order):
        orc = pyoracle.ClothOracle(fold_cloth1_mask(), order=order)

        def run(envs, threads, reps):
            rng = np.random.default_rng(0)
            x, v, prim, k, mu, actions = make_cloth_case(rng, envs, MACRO, deform=0.0005, v_scale=0.01)
            actions *= 0.2
            g = [rng.normal(size=a.shape).astype(np.float32) for a in (x, v, prim)]
            t0 = time.time()
            for _ in range(reps):
                orc.rollout_fwd(x, v, prim, k, mu, actions, nthreads=threads)
            t_f = time.time() - t0
            t0 = time.time()
            for _ in range(reps):
                orc.rollout_bwd(x, v, prim, k, mu, actions, g[0], g[1], g[2], normalize=True, nthreads=threads)
            t_b = time.time() - t0
            return envs * reps * MACRO * SUBSTEPS, t_f, t_b

        threads = min(sample_envs, nproc)
        n, t_f, t_b = run(sample_envs, threads, ep_len)
        n1, t_f1, t_b1 = run(1, 1, ep_len)
        nn, t_fn, t_bn = run(nproc, nproc, ep_len)
        name = {1: "the reference's literal operation order (cloth_simulator.py:257-337 as written)",
                2: "operation order v2 (the reference's formulas re-associated, what the default GPU forward runs)"}[order]
        return {"value": n / (t_f + t_b), "unit": "substeps/s", "cores": threads, "kind": "port", "order": order,
                "sample": f"CPU restatement (C++ {build}, f32, {name}, no FMA contraction; not "
                          f"JAX-CPU) on a SYNTHETIC cloth state (tests/conftest.make_cloth_case: deformed lattice + a lifting macro-action sequence, "
                          f"not the env state the GPU leg runs; the work per substep does not depend on the data): "
                          f"{sample_envs} envs x {ep_len} step_diff x {MACRO * SUBSTEPS} substeps, forward {t_f:.2f}s + adjoint "
                          f"{t_b:.2f}s; the adjoint call recomputes the forward states itself (it keeps no checkpoint), so its time "
                          f"includes one more forward; OpenMP over envs ({threads} threads; substeps are sequential)",
                "fwd_only_value": n / t_f,
                "one_thread": {"value": n1 / (t_f1 + t_b1), "fwd_only_value": n1 / t_f1, "cores": 1, "sample": f"1 env x {ep_len} step_diff"},
                "all_cores": {"value": nn / (t_fn + t_bn), "fwd_only_value": nn / t_fn, "cores": nproc,
                              "sample": f"{nproc} envs x {ep_len} step_diff on {nproc} threads = the cores this job may use (affinity mask and cgroup quota; "
                                        f"the box shows {os.cpu_count()} logical CPUs); more envs than the headline workload has"}}

    out = legs(gpu_order)
    other = 1 if gpu_order == 2 else 2
    out["value_is"] = (f"order {gpu_order}: the operation order of the GPU leg's forward (`value` of this line); "
                       f"the order-{other} figure is under `{'reference_order' if other == 1 else 'v2_order'}`")
    out["reference_order" if other == 1 else "v2_order"] = legs(other)
    return out


def cpu_baseline_tshirt(env, st, sample_envs=4, macro=4):
    """Oracle (CPU restatement, NOT JAX-CPU) beside the fold_tshirt line: the env's own reset state (3573 particles on the 180x180
    lattice, k = 5000, dt = 0.5e-3), `macro` of the 40 macro actions of a step_diff (a lifting sequence; the work per substep does not
    depend on the data), forward + adjoint, OpenMP over envs.  Checker only, never the product path."""
    pyoracle, build = _oracle_native()
    conf = env.conf
    mask = env.cloth_mask.cpu().numpy() if hasattr(env.cloth_mask, "cpu") else np.asarray(env.cloth_mask)
    order = 1 if (getattr(conf, "kernel_mode", 0) == 1 or getattr(conf, "one_workgroup_per_env", False)) else 2   # what the GPU leg runs
    orc = pyoracle.ClothOracle(mask, N=int(conf.N), gravity=float(conf.gravity), damping=float(conf.damping), dt=float(conf.dt),
                               max_v=float(conf.max_v), small_num=float(conf.small_num), substeps=SUBSTEPS, order=order)
    npy = lambda t: np.ascontiguousarray(t.detach().float().cpu().numpy()[:sample_envs])
    x, v = npy(st.x), npy(st.v)
    prim = np.stack([npy(st.primitive0), npy(st.primitive1)], 1)
    k, mu = npy(st.stiffness.float()), npy(st.mu)
    acts = np.zeros((macro, sample_envs, 8), np.float32)
    acts[:, :, 1] = 0.006 * 50
    acts[:, :, 3] = 1
    prim[:, 0, :3] = x[:, x.shape[1] // 2] + np.float32([0, 0.002, 0])
    rng = np.random.default_rng(0)
    g = [rng.normal(size=a.shape).astype(np.float32) for a in (x, v, prim)]
    threads = min(sample_envs, host_cores())
    t0 = time.time()
    orc.rollout_fwd(x, v, prim, k, mu, acts, nthreads=threads)
    t_f = time.time() - t0
    t0 = time.time()
    orc.rollout_bwd(x, v, prim, k, mu, acts, g[0], g[1], g[2], normalize=True, nthreads=threads)
    t_b = time.time() - t0
    n = sample_envs * macro * SUBSTEPS
    return {"value": n / (t_f + t_b), "unit": "substeps/s", "cores": threads, "kind": "port", "fwd_only_value": n / t_f,
            "order": order,
            "sample": f"CPU restatement (C++ {build}, f32, operation order {order} = the order the GPU leg of this line runs ({'v2, re-associated' if order == 2 else 'reference, literal'}); not JAX-CPU): {sample_envs} envs x {macro} macro actions x {SUBSTEPS} substeps of the env's "
                      f"reset state (P={x.shape[1]}), forward {t_f:.2f}s + adjoint (with its own forward recompute) {t_b:.2f}s, OpenMP over envs ({threads} threads)"}


def saturation_probe(env, device, num_envs=1024, reps=3):
    """NOT the headline metric: the same two kernels with enough environments to fill the chip (the headline
    workload has 4 envs = 4 workgroups on 256 CUs, so its HBM fraction is fixed by the workload, not the kernel).
    One step_diff worth of substeps (40 x 50), forward with checkpoints + adjoint, kernel time from HIP events."""
    from unidom_amd.engine.cloth_simulator import ClothSimulator, _Rollout
    sim = ClothSimulator(env.conf, num_envs, env.get_collision_func(), env.cloth_mask, device=device, mode=env.simulator.mode)
    st = sim.reset_jax()
    g = torch.Generator(device=device).manual_seed(0)
    x = (st.x + 1e-4 * torch.randn(st.x.shape, device=device, generator=g)).abs().requires_grad_(True)
    v = (0.01 * torch.randn(st.v.shape, device=device, generator=g)).requires_grad_(True)
    prim = torch.stack([st.primitive0, st.primitive1], 1).contiguous()
    k = st.stiffness.to(torch.float32)
    pick = x.detach()[:, 100, :]
    acts = torch.zeros((MACRO, num_envs, 8), device=device)
    acts[:3, :, :3] = (pick - prim[:, 0, :3])[None] / 3 * 50 / 50
    acts[:3, :, 3] = 1
    acts[3:13, :, 1] = 0.006
    acts[13:33, :, 0] = 0.004
    acts[33:, :, 3] = 1
    sim.profile = {"fwd": [], "bwd": []}
    for _ in range(reps + 1):
        xo, vo, po = _Rollout.apply(sim, x, v, prim, k, st.mu, acts, False)
        (xo.sum() + vo.sum()).backward()
    torch.cuda.synchronize(device)
    ms = {kk: float(np.mean([a.elapsed_time(b) for a, b in vv[1:]])) for kk, vv in sim.profile.items()}
    n = num_envs * MACRO * SUBSTEPS
    tot = (ms["fwd"] + ms["bwd"]) * 1e-3
    # what the kernels really move: the per-substep checkpoint stream (written by the forward, read back by the adjoint); state and
    # cotangents never leave registers / LDS.  The PMC passes at the headline shape measure exactly that (98.9 MB per launch =
    # 4 envs x 2001 records x 12 352 B, profiles/pmc_traffic.json), so the counter bytes of a 1024-env launch are its checkpoint size.
    from unidom_amd import _lib
    import ctypes as C
    ck = float(_lib.lib().ud_cloth_ckpt_bytes(sim._h, C.c_int(num_envs), C.c_int(MACRO)))
    return {"note": "same kernels, chip filled; not the headline workload.  hbm_frac = checkpoint-stream bytes (what the FETCH_SIZE / WRITE_SIZE "
                    "counters see) / kernel time / 8 TB/s; hbm_frac_algorithmic uses SURVEY 8(d)'s 48 / 72 B per particle-substep, bytes these "
                    "kernels never move (state and cotangents stay on chip) -- quoted only for comparison with round 2's line",
            "num_envs": num_envs, "kernel_ms": ms, "substeps_per_sec_fwd_bwd": n / tot, "hbm_bytes_per_launch": ck,
            "achieved_GBs": {"fwd": ck / (ms["fwd"] * 1e-3) / 1e9, "bwd": ck / (ms["bwd"] * 1e-3) / 1e9},
            "hbm_frac": {"fwd": ck / (ms["fwd"] * 1e-3) / 1e9 / HBM_PEAK_GBS, "bwd": ck / (ms["bwd"] * 1e-3) / 1e9 / HBM_PEAK_GBS},
            "hbm_frac_algorithmic": {"fwd": n * BYTES_FWD / (ms["fwd"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                     "bwd": n * BYTES_BWD / (ms["bwd"] * 1e-3) / 1e9 / HBM_PEAK_GBS},
            "issue": {k: issue_roof({"fwd": "cloth_rollout_fwd_v2_kernel", "bwd": "cloth_rollout_bwd_fast_kernel"}[k], ms[k], 8 * num_envs,
                                    min(256, num_envs), MACRO * SUBSTEPS) for k in ("fwd", "bwd")} if sim.mode == 0 else None}


def touched_cells(x, n_grid=64):
    """G_act of SURVEY.md 8(d): number of grid cells with >= 1 particle contribution, counted on the host."""
    base = (x * n_grid - 0.5).astype(np.int32)
    cells = set()
    for b in base:
        for i in range(3):
            for j in range(3):
                for k in range(3):
                    cells.add((b[0] + i, b[1] + j, b[2] + k))
    return len(cells)


def device_active_cells(sim, run_once, device):
    """G_act of SURVEY.md 8(d) as the DEVICE counted it: one more (untimed) forward + backward with the simulator keeping a reference to its
    checkpoint, then ud_mpm_ckpt_cells = the grid-checkpoint records of that step call per env / substeps.  0.0 where the handle keeps no grid
    checkpoint (one workgroup per env): the host count of the input state stands then.  (The host count is taken on ONE env's input state; the
    device count is the mean over all envs and all substeps of a step call, during which a pushed rope or a poured liquid spreads.)"""
    sim.keep_last_ckpt = True
    run_once()
    torch.cuda.synchronize(device)
    g = sim.active_cells_per_substep()
    sim.keep_last_ckpt, sim._last_ckpt = False, None
    return g


def bench_whip_rope(args, rank, world, device, name="whip_rope"):
    """Secondary lines: the APG update (policy, ep_len x step_diff, loss, backward, clip, Adam) on an MPM env, 32 envs per GPU,
    ep_len 3.  whip_rope: N=67, res 32^3, 70 substeps/step, one workgroup per env.  pour_water: 702 liquid particles, two bowls
    with the container SDF in soft-contact mode, res 26x20x26, 23 substeps/step, many-workgroup path.  pour_soup: the same bowls at
    n_grid 128 (res 128x64x128, 25 substeps/step) with 7631 particles of mixed material per env."""
    from unidom_amd.algorithms.apg.core import APG
    from unidom_amd.envs.registration import env_functions
    from unidom_amd.utils import prng
    B, ep = (args.envs if name == "whip_rope" else 32), EP_LEN
    env = env_functions[name](batch_size=B, seed=0, aux_reward=True, device=device)
    _, state = env.reset(prng.split(prng.PRNGKey(0), world)[rank])
    learner = APG(env, ep, learning_rate=1e-4, max_gradient_norm=0.3, seed=0)

    def sync():
        torch.cuda.synchronize(device)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(device)

    want_graph = name == "whip_rope" and world == 1 and not args.no_graph
    if want_graph:                                           # the learner's whole life on one non-default stream (APG.capture)
        work = torch.cuda.Stream(device)
        work.wait_stream(torch.cuda.current_stream(device))
        torch.cuda.set_stream(work)
    restore, box = capture_step_inputs(env.simulator)        # the first simulator.step's inputs, for the CPU baseline (untimed)
    for _ in range(args.warmup):
        learner.minimize(state)
    restore()
    env.simulator.check_status()
    # whip_rope (one workgroup per env, ~200 launches per update of which 6 are the simulator's): the update replayed as ONE HIP graph
    # (APG.capture).  Kernel times for the roofline come from an eager pass beside the timed region (a graph has no event hooks).
    graphed = False
    if want_graph:
        env.simulator.profile = {"fwd": [], "bwd": []}
        learner.minimize(state)
        sync()
        prof, env.simulator.profile = env.simulator.profile, None
        try:
            learner.capture(state)
            learner.minimize_captured()
            graphed = True
        except Exception as e:                               # stays a measured eager line, and says so
            print(f"[bench] graph capture failed, eager update instead: {type(e).__name__}: {e}", file=sys.stderr)
    if not graphed:
        env.simulator.profile = {"fwd": [], "bwd": []}
    learner.sync.profile = []
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        if graphed:
            learner.minimize_captured()
        else:
            learner.minimize(state)
    sync()
    dt = time.perf_counter() - t0
    if not graphed:
        prof, env.simulator.profile = env.simulator.profile, None
    env.simulator.check_status()
    ranks = rank_report(world, device, dt, {k: float(np.mean([a.elapsed_time(b) for a, b in v])) for k, v in prof.items() if v}, learner.sync)
    tm = torch.tensor([dt], device=device, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(tm, op=dist.ReduceOp.MAX)
    dt = float(tm[0])
    if rank == 0:
        S, N = env.conf.steps, env.simulator.n_particles
        units = world * B * ep * S * args.steps
        g_host = touched_cells(state.x[0].detach().cpu().numpy() + 0.0, env.conf.n_grid)
        g_act = device_active_cells(env.simulator, lambda: learner.minimize(state), device) or g_host
        k_ms = {k: float(np.mean([a.elapsed_time(b) for a, b in v])) for k, v in prof.items() if v}
        dom = max(k_ms, key=k_ms.get)
        per_sub = (192 * N + 56 * g_act) if dom == "fwd" else (288 * N + 112 * g_act)
        per_launch = B * S * per_sub
        achieved = per_launch / (k_ms[dom] * 1e-3) / 1e9
        cpu = None
        if not args.no_cpu_baseline and world == 1 and "st" in box:
            big = N > 2000
            cpu = cpu_baseline_mpm(env.simulator, env.conf, box["st"], 4 if big else 8, 1 if big else 6,
                                   f"the first simulator.step of the timed update ({name}: the env's own state and primitive actions)")
        traffic = None          # PMC passes exist for the default shapes only (32 envs per launch)
        if name == "whip_rope" and B == 32:
            traffic = pmc_traffic("mpm_step_fwd_kernel" if dom == "fwd" else "mpm_step_bwd_ws_kernel")
        elif B == 32:                             # many-workgroup path: all kernels of one step call (tools/pmc_large.sh)
            traffic = pmc_traffic(f"large_path:{name}:{dom}")
        print(json.dumps({
            "metric": "mpm_substeps_per_sec_fwd_bwd", "value": units / dt, "unit": "substeps/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic", **dist_info(world, learner.n_params),
            "config": {"workload": f"{name} (MLS-MPM, N={N}, res {'x'.join(str(r) for r in env.conf.res)}, {S} substeps/step) APG loss+grad+update: "
                                   f"{B} envs per GPU, ep_len={ep}" + (", the update replayed as one HIP graph" if graphed else ""), "touched_cells": g_act,
                       "touched_cells_host_count_of_one_input_state": g_host,
                       "hip_graph": graphed},
            "roofline": {"bound": "hbm", "kernel": lg_label(dom, env.simulator, B) if env.simulator.n_primitive > 1 or N > 128 else
                         ("mpm_step_fwd_kernel" if dom == "fwd" else ("mpm_step_bwd_ws_kernel" if N <= 96 else "mpm_step_bwd_kernel")),
                         "achieved": achieved, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "kernel_ms": k_ms,
                         "algorithmic_bytes_per_launch": per_launch,
                         **({"issue": issue_roof("mpm_step_fwd_kernel" if dom == "fwd" else "mpm_step_bwd_ws_kernel", k_ms[dom],
                                                 B * ((4 * N + 63) // 64 + (0 if dom == "fwd" else (N + 63) // 64)), min(B, 256), S)}
                            if N <= 128 and env.simulator.n_primitive == 1 else {"issue": lg_issue(f"large_path:{name}:{dom}", k_ms[dom]) if B == 32 else None}),
                         "note": f"one workgroup per env ({min(B, 256)} of 256 CUs busy), latency bound: LDS atomics + barriers" if N <= 128 and env.simulator.n_primitive == 1
                         else f"latency / issue bound: small launches on {B} x {N} particles"},
            **ranks, **({"cpu_baseline": cpu} if cpu else {})}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def cpu_baseline_torus(sim, st, action, grad, budget_s=20.0):
    """CPU beside the PlasticineLab lines (parity of this path is unpinned: taichi is absent).  Forward: the C++ restatement
    (oracle/csrc/plb_oracle.hpp: f64, dense n_grid^3 grid, OpenMP over envs) on the bench's own envs.  Forward + adjoint: the C++
    restatement has no adjoint -- the CPU reference of the adjoint is torch.autograd through the twin (oracle/twin/plb_twin_torch.py,
    dense grid, all substeps taped), timed on ONE env.step of ONE env and only at n_grid 64 (at 128 the tape needs ~10 GB and minutes)."""
    pyoracle, build = _oracle_native()
    cfg = sim.cfg
    B = min(8, st.x.shape[0])
    npy = lambda t: t.detach().cpu().numpy()[:B]
    cur = dict(x=npy(st.x), v=npy(st.v), C=npy(st.C), F=npy(st.F), prim_pos=npy(st.prim_pos))
    soft, E, nu, ys, act = npy(st.softness), npy(st.E), npy(st.nu), npy(st.yield_stress), npy(action)
    orc = pyoracle.PlbOracle(N=sim.n_particles, n_grid=sim.n_grid, substeps=sim.substeps, dt=sim.dt, gravity=tuple(cfg.gravity),
                             ground_friction=float(cfg.ground_friction), radius=tuple(cfg.prim_radius))
    threads = min(B, host_cores())
    t, done = 0.0, 0
    while done < 10 and t < budget_s * (0.4 if grad else 1.0):
        t0 = time.time()
        cur = orc.step(cur["x"], cur["v"], cur["C"], cur["F"], cur["prim_pos"], soft, act, E, nu, ys, nthreads=threads)
        t += time.time() - t0
        done += 1
    fwd_rate = B * done * sim.substeps / t
    out = {"value": fwd_rate, "unit": "substeps/s", "cores": threads, "kind": "port",
           "sample": f"forward only: C++ restatement ({build}, f64, dense {sim.n_grid}^3 grid; not Taichi): {B} envs x {done} env.steps x {sim.substeps} "
                     f"substeps in {t:.2f}s, OpenMP over envs ({threads} threads)"}
    if grad and sim.n_grid <= 64:
        import torch as _t
        from oracle.twin.plb_twin import PlbConf as TwinConf
        from oracle.twin.plb_twin_torch import PlbTorchTwin
        nthr = min(8, host_cores())
        _t.set_num_threads(nthr)
        tw = PlbTorchTwin(TwinConf(quality=float(cfg.quality), n_particles=sim.n_particles))
        T = lambda a, r=False: _t.tensor(np.asarray(a, np.float64)[:1], requires_grad=r)
        x = T(npy(st.x), True)
        t0 = time.time()
        o = tw.step(x, T(npy(st.v)), T(npy(st.C)), T(npy(st.F)), T(npy(st.prim_pos)), T(act, True), T(soft), T(E, True), T(nu), T(ys),
                    _t.full((1,), float(cfg.ground_friction), dtype=_t.float64))
        (o[0].sum() + o[1].sum()).backward()
        tt = time.time() - t0
        out = {"value": sim.substeps / tt, "unit": "substeps/s", "cores": nthr, "kind": "port", "fwd_only_value": fwd_rate,
               "sample": f"forward + adjoint: torch.autograd through the twin (f64, dense {sim.n_grid}^3 grid, {nthr} torch threads): 1 env x 1 env.step x "
                         f"{sim.substeps} substeps in {tt:.2f}s; fwd_only_value = the C++ restatement's forward ({out['sample']})"}
    elif grad:
        out["sample"] = ("forward ONLY (no CPU adjoint at this grid: the autograd twin's tape of 39 dense 128^3 substeps needs ~10 GB and minutes; "
                         "the n_grid 64 line carries the forward + adjoint CPU figure) -- ") + out["sample"]
    return out


def bench_torus(args, rank, world, device):
    """BASELINE config 5: PlasticineLab Torus (f64 elasto-plastic MPM, N=1000), 8 envs per GPU (64 on 8 GPUs), forward
    only like the reference's scripted rollout (solver.py:290-350).  --n-grid 64 = quality 1 (19 substeps/step),
    --n-grid 128 = quality 2 (the "128^3 grid" of BASELINE.json, dt 5e-5, 39 substeps/step).  One "step" = 10 env.steps.
    --plb-grad: the differentiable route instead (solver.py:41-54, ti.Tape): 10 env.steps forward with checkpoints, the
    density / SDF / contact loss of the last state, and the backward through all of them to the actions and E / nu / yield stress."""
    from unidom_amd.engine.plb_simulator import PlbConf, PlbSimulator
    cfg = PlbConf()
    cfg.quality = 2.0 if args.n_grid == 128 else 1.0
    B = 8 if args.envs == 32 else args.envs
    sim = PlbSimulator(cfg, B, device=device)
    st = sim.reset()
    start = np.array([0.2, 0.3, 0.5])
    p0 = np.array(cfg.prim_init_pos[0])
    act = np.diff(np.linspace(p0, start, 200), axis=0)[0]          # solver.py:299-302: constant displacement per env.step
    action = torch.tensor(np.repeat(act[None], B, 0), dtype=torch.float64, device=device)
    inner = 10
    grad = bool(getattr(args, "plb_grad", False))
    if grad:
        G = sim.n_grid ** 3
        target_density = torch.zeros(G, dtype=torch.float64, device=device)
        target_sdf = torch.linspace(0.0, 1.0, G, dtype=torch.float64, device=device)
        st = st._replace(prim_pos=st.prim_pos.clone())
        st.prim_pos[:, 0] = st.x[:, 7]                               # sphere 0 on the rope: the action gets a gradient
        leaves = dict(action=action.clone().requires_grad_(True), E=st.E.clone().requires_grad_(True),
                      nu=st.nu.clone().requires_grad_(True), ys=st.yield_stress.clone().requires_grad_(True))

    def sync():
        torch.cuda.synchronize(device)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(device)

    def one_grad():
        for t in leaves.values():
            t.grad = None
        s = st._replace(E=leaves["E"], nu=leaves["nu"], yield_stress=leaves["ys"])
        for _ in range(inner):
            s = sim.step(s, leaves["action"])
        loss, _ = sim.compute_loss(s, target_density, target_sdf, (1.0, 1.0, 1.0), True)
        loss.sum().backward()

    for _ in range(args.warmup):           # a warm-up step is a whole bench step in both modes (inner env.steps)
        if grad:
            one_grad()
        else:
            for _ in range(inner):
                st = sim.step(st, action)
    sim.check_status()                         # a part of the persistent kernels that gave up in the warm-up would poison every later step (NaN)
    sim.profile = {"fwd": [], "bwd": []}      # HIP events around every step call, on its stream
    sync()
    t0 = time.perf_counter()
    if grad:
        for _ in range(args.steps):
            one_grad()
    else:
        for _ in range(args.steps * inner):
            st = sim.step(st, action)
    sync()
    dt = time.perf_counter() - t0
    prof, sim.profile = sim.profile, None
    sim.check_status()                         # ... and a line must never be a rate over NaN state: raises if any part timed out in the timed region
    tm = torch.tensor([dt], device=device, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(tm, op=dist.ReduceOp.MAX)
    dt = float(tm[0])
    if rank == 0:
        assert torch.isfinite(st.x).all()
        if grad:
            assert all(torch.isfinite(t.grad).all() for t in leaves.values()) and float(leaves["action"].grad.abs().sum()) > 0
        cpu = None if (args.no_cpu_baseline or world > 1) else cpu_baseline_torus(sim, st, action, grad)
        units = world * B * sim.substeps * inner * args.steps
        g_act = touched_cells(st.x[0].detach().cpu().numpy().astype(np.float64), sim.n_grid)
        per_sub = 2 * ((480 if grad else 192) * sim.n_particles + (168 if grad else 56) * g_act)   # f64: double the f32 figure
        # the dominant kernel of a step call and its mean duration (HIP events on the launch stream): on the persistent path a step call IS one
        # launch (pcl_fwd_kernel / pcl_bwd_kernel); on the multi-kernel path the events bracket all launches of the call
        k_ms = {k: float(np.mean([a.elapsed_time(b) for a, b in v])) for k, v in prof.items() if v}
        dom = max(k_ms, key=k_ms.get)
        per_call = B * sim.substeps * 2 * ((192 * sim.n_particles + 56 * g_act) if dom == "fwd" else (288 * sim.n_particles + 112 * g_act))
        persistent = sim.launch_plan(B) == 2
        kname = ("pcl_bwd_kernel" if dom == "bwd" else "pcl_fwd_kernel") if persistent else "plb multi-kernel path (" + ("5" if dom == "bwd" else "2") + " kernels/substep)"
        achieved = per_call / (k_ms[dom] * 1e-3) / 1e9
        print(json.dumps({
            "metric": "plb_substeps_per_sec_fwd_bwd" if grad else "plb_substeps_per_sec_fwd", "value": units / dt, "unit": "substeps/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic", **dist_info(world),
            "config": {"workload": f"PlasticineLab Torus (f64 von-Mises MPM, N={sim.n_particles}, n_grid={sim.n_grid}, "
                                   f"{sim.substeps} substeps/env.step), " + ("forward with checkpoints + loss + adjoint" if grad else "forward rollout")
                                   + f", {B} envs per GPU, step = {inner} env.steps",
                       "touched_cells": g_act, "parity": "unpinned (taichi absent)"},
            "roofline": {"bound": "hbm", "kernel": kname, "achieved": achieved, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "kernel_ms": k_ms, "algorithmic_bytes_per_launch": per_call,
                         "launch": "one step call = one env.step (" + f"{sim.substeps} substeps, {B} envs)" + ("; one persistent launch" if persistent else ""),
                         "traffic": pmc_traffic(f"{kname}:{'grad' if grad else 'fwd'}:ngrid{sim.n_grid}") if (B == 8 and persistent) else None,
                         "traffic_per_bench_step": pmc_traffic(f"plb:{'grad' if grad else 'fwd'}:ngrid{sim.n_grid}") if B == 8 else None,
                         "algorithmic_bytes_per_bench_step": units / world / args.steps * per_sub,
                         "issue": issue_roof(f"{kname}:{'grad' if grad else 'fwd'}:ngrid{sim.n_grid}", k_ms[dom], None, 256, sim.substeps) if (B == 8 and persistent) else None,
                         "issue_per_bench_step": plb_issue(f"plb:{'grad' if grad else 'fwd'}:ngrid{sim.n_grid}", dt / args.steps * 1e3) if B == 8 else None,
                         "note": "latency bound: 8 envs x 1000 particles = one workgroup of one wave per SIMD on every CU; traffic / issue = the dominant kernel's "
                                 "counters per launch; *_per_bench_step = all plb / pcl kernels of a bench step (loss included)"},
            **({"cpu_baseline": cpu} if cpu else {})}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def bench_mpm_scaled(args, rank, world, device):
    """Scaling stress test: whip_rope's rope seeded at n_grid 128 / 256 (N = 798 / 6675, res 64^3 /
    128^3), one simulator.step (70 substeps) forward + adjoint per "step"; dt = 1e-4 is kept, so the CFL number is
    2x / 4x the default config's -- a throughput measurement, not a physics claim."""
    from unidom_amd.engine.mpm_simulator import SimpleMPMSimulator, _Step
    from unidom_amd.envs.whip_rope_env import DefaultConf
    conf = DefaultConf()
    ng = args.n_grid
    conf.n_grid, conf.res = ng, (ng // 2,) * 3
    conf.dx, conf.inv_dx = 1 / ng, float(ng)
    conf.p_vol = (conf.dx * 0.5) ** 2
    conf.p_mass = conf.p_vol * conf.p_rho
    B = args.envs
    sim = SimpleMPMSimulator(conf, B, use_position_control=True, device=device)
    sim.grid_ckpt_cells = args.grid_ckpt   # measured: the rope touches 0.58 (n_grid 128) / 0.30 (256) cells per particle
    st0 = sim.add_box(conf, None, size=conf.rope_width, init_pos=[0.25, 0.01, 0.25], z_rotation_angle=conf.rope_z_rotation_angle,
                      material=1, density=2.75, hardness=1.0)
    N = st0.x.shape[0]
    sim.n_particles = N
    sim._make_handle()
    S = conf.steps
    g = torch.Generator(device=device).manual_seed(rank)
    x = st0.x[None].repeat(B, 1, 1).contiguous().requires_grad_(True)
    v = torch.zeros((B, N, 3), device=device, requires_grad=True)
    Cm = torch.zeros((B, N, 3, 3), device=device, requires_grad=True)
    F = torch.eye(3, device=device)[None, None].repeat(B, N, 1, 1).contiguous().requires_grad_(True)
    J = torch.ones((B, N), device=device)
    ppos = torch.zeros((B, S, 3), device=device); ppos[:, 0] = torch.tensor([0.25, 0.01, 0.05], device=device)
    prot = torch.zeros((B, S, 4), device=device); prot[..., 0] = 1
    psize = torch.full((B, 3), 0.02, device=device)
    fr = torch.full((B, 1), 0.1, device=device); mu = torch.full((B, 1), 45.45, device=device); la = torch.full((B, 1), 11.36, device=device)
    act = (torch.tanh(torch.randn((B, 6), device=device, generator=g)) / 50).requires_grad_(True)

    def one():
        out = _Step.apply(sim, x, v, Cm, F, J, ppos, prot, psize, fr, mu, la, act)
        (out[0].sum() + out[1].sum()).backward()

    def sync():
        torch.cuda.synchronize(device)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(device)

    for _ in range(args.warmup):
        one()
    sim.profile = {"fwd": [], "bwd": []}
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one()
    sync()
    dt = time.perf_counter() - t0
    prof, sim.profile = sim.profile, None
    tm = torch.tensor([dt], device=device, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(tm, op=dist.ReduceOp.MAX)
    dt = float(tm[0])
    if rank == 0:
        units = world * B * S * args.steps
        cpu = None
        if not args.no_cpu_baseline and world == 1:
            npy = lambda t: t.detach().float().cpu().numpy()
            sto = dict(x=npy(x), v=npy(v), C=npy(Cm), F=npy(F), J=npy(J), ppos=npy(ppos), prot=npy(prot), psize=npy(psize), friction=npy(fr).reshape(-1),
                       mu=npy(mu).reshape(-1), lamda=npy(la).reshape(-1), action=npy(act))
            cpu = cpu_baseline_mpm(sim, conf, sto, 8 if N < 2000 else 2, 2 if N < 2000 else 1, f"the bench's own inputs (rope seeded at n_grid {ng})")
        g_host = touched_cells(st0.x.detach().cpu().numpy(), ng)
        g_act = device_active_cells(sim, one, device) or g_host
        k_ms = {k: float(np.mean([a.elapsed_time(b) for a, b in vv])) for k, vv in prof.items() if vv}
        dom = max(k_ms, key=k_ms.get)
        per_launch = B * S * ((192 * N + 56 * g_act) if dom == "fwd" else (288 * N + 112 * g_act))
        achieved = per_launch / (k_ms[dom] * 1e-3) / 1e9
        print(json.dumps({
            "metric": "mpm_substeps_per_sec_fwd_bwd", "value": units / dt, "unit": "substeps/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic", **dist_info(world),
            "config": {"workload": f"whip_rope rope seeded at n_grid={ng} (N={N}, res {ng // 2}^3, {S} substeps/step), "
                                   f"simulator.step forward+adjoint, {B} envs per GPU; scaling stress test", "touched_cells": g_act,
                       "touched_cells_host_count_of_one_input_state": g_host},
            "roofline": {"bound": "hbm", "kernel": lg_label(dom, sim, B),
                         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": pmc_traffic(f"large_path:whip_rope_ngrid{ng}:{dom}") if B == 32 else None,
                         "issue": lg_issue(f"large_path:whip_rope_ngrid{ng}:{dom}", k_ms[dom]) if B == 32 else None,
                         "kernel_ms": k_ms, "algorithmic_bytes_per_launch": per_launch},
            **({"cpu_baseline": cpu} if cpu else {})}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _oracle_native():
    from oracle import pyoracle
    try:
        pyoracle.use_native()
        return pyoracle, "-O3 -march=native built on this host"
    except Exception as e:
        return pyoracle, f"-O3 baseline x86-64 (the native rebuild failed: {type(e).__name__})"


def capture_step_inputs(sim):
    """Record the arguments of the next simulator.step_jax call (the exact inputs the HIP step receives inside env.step_diff):
    returns (restore, box) -- box["st"] is the oracle's input dict once a step has run."""
    box = {}
    orig = sim.step_jax

    def spy(state, action):
        if "st" not in box:
            P = sim.n_primitive
            npy = lambda t: t.detach().float().cpu().numpy()
            prims = state.primitives
            if P == 1:
                ppos, prot, psize = npy(prims[0].position), npy(prims[0].rotation), npy(prims[0].size)
            else:
                ppos, prot, psize = (np.stack([npy(getattr(q, k)) for q in prims], 1) for k in ("position", "rotation", "size"))
            box["st"] = dict(x=npy(state.x), v=npy(state.v), C=npy(state.C), F=npy(state.F), J=npy(state.J), ppos=ppos, prot=prot, psize=psize,
                             friction=npy(state.friction).reshape(-1), mu=npy(state.mu).reshape(-1), lamda=npy(state.lamda).reshape(-1),
                             action=npy(action[:, :6 * P]))
        return orig(state, action)

    sim.step_jax = spy
    return (lambda: setattr(sim, "step_jax", orig)), box


def cpu_baseline_mpm(sim, conf, st, sample_envs, steps, what, budget_s=25.0):
    """Oracle (CPU restatement of mpm_simulator.py:413-429 + adjoint, dense `res` grid like the reference; NOT JAX-CPU), rebuilt
    here with -O3 -march=native, timed on the host cores: `steps` chained simulator.steps (conf.steps substeps each) forward +
    adjoint for `sample_envs` envs (OpenMP over envs, substeps sequential), stopping early once `budget_s` is spent.  The oracle's
    adjoint call recomputes the forward states itself.  Checker only, never the product path."""
    pyoracle, build = _oracle_native()
    N, S = st["x"].shape[1], int(conf.steps)
    st = {k: np.ascontiguousarray(v[:sample_envs]) for k, v in st.items()}
    orc = pyoracle.MpmOracle(N, n_grid=int(conf.n_grid), res=tuple(conf.res), steps=S, dt=float(conf.dt), position_control=bool(sim.use_position_control),
                             material=np.asarray(sim.material), hardness=np.asarray(sim.h), prim_friction=float(sim.prim_friction),
                             prim_softness=float(sim.prim_softness), n_prim=int(sim.n_primitive), sdf=sim.sdf_kind)
    rng = np.random.default_rng(0)
    pa = (sim.n_primitive,) if sim.n_primitive > 1 else ()
    g = dict(gx=rng.normal(size=st["x"].shape).astype(np.float32), gv=np.zeros_like(st["x"]), gC=np.zeros_like(st["C"]), gF=np.zeros_like(st["F"]),
             gppos=np.zeros((sample_envs,) + pa + (S, 3), np.float32))
    threads = min(sample_envs, host_cores())
    t_f = t_b = 0.0
    done = 0
    for _ in range(steps):
        t0 = time.time()
        o = orc.step_fwd(st, nthreads=threads)
        t_f += time.time() - t0
        t0 = time.time()
        orc.step_bwd(st, g, clip=True, nthreads=threads)
        t_b += time.time() - t0
        st.update(x=o["x"], v=o["v"], C=o["C"], F=o["F"], J=o["J"], ppos=o["ppos"], prot=o["prot"])
        done += 1
        if t_f + t_b > budget_s:
            break
    n = sample_envs * done * S
    return {"value": n / (t_f + t_b), "unit": "substeps/s", "cores": threads, "kind": "port", "fwd_only_value": n / t_f,
            "sample": f"CPU restatement (C++ {build}, f32, dense res grid like the reference; not JAX-CPU) on {what}: {sample_envs} envs x {done} "
                      f"simulator.steps x {S} substeps, forward {t_f:.2f}s + adjoint (with its own state recompute) {t_b:.2f}s, OpenMP over envs "
                      f"({threads} threads)"}


def cpu_baseline_shape_rope(env, st, act, sample_envs=8, steps=6):   # ~11 s of host work
    """Oracle (CPU restatement, dense 64x6x64 grid, NOT JAX-CPU) on the host cores: `steps` scanned simulator.steps
    (133 substeps each) forward + adjoint for `sample_envs` of the bench's envs.  Checker only, never the product path."""
    from oracle import pyoracle
    try:
        pyoracle.use_native()
    except Exception:
        pass                     # portable build instead
    MpmOracle = pyoracle.MpmOracle
    conf = env.conf
    N, S = st.x.shape[1], conf.steps
    npy = lambda t: t.detach().cpu().numpy()[:sample_envs]
    x0 = npy(st.x)
    shift = (np.array(conf.res, np.float32) * np.float32(0.5) / np.float32(conf.n_grid) - x0.mean(1, dtype=np.float32)).astype(np.float32)
    shift[:, 1] = 0
    a = npy(act)
    start, end = a[:, :3] + shift, a[:, 3:] + shift
    start[:, 1] = end[:, 1] = 0.01
    nrm = np.linalg.norm(end - start, axis=-1, keepdims=True).astype(np.float32) + np.float32(1e-8)
    push = ((end - start) / nrm * np.clip(nrm, 0, 0.3) / np.float32(conf.primitive_action_steps)).astype(np.float32)
    push[:, 1] = 0
    ppos = np.zeros((sample_envs, S, 3), np.float32)
    ppos[:, 0] = start
    prot = np.zeros((sample_envs, S, 4), np.float32)
    prot[..., 0] = 1
    ost = dict(x=x0 + shift[:, None], v=npy(st.v), C=npy(st.C), F=npy(st.F), J=npy(st.J), ppos=ppos, prot=prot,
               psize=npy(st.primitives[0].size), friction=npy(st.friction).reshape(-1), mu=npy(st.mu).reshape(-1),
               lamda=npy(st.lamda).reshape(-1), action=np.concatenate([push, np.zeros_like(push)], -1))
    orc = MpmOracle(N, n_grid=conf.n_grid, res=conf.res, steps=S, dt=conf.dt, position_control=False, material=np.full(N, 2))
    rng = np.random.default_rng(0)
    g = dict(gx=rng.normal(size=x0.shape).astype(np.float32), gv=np.zeros_like(x0), gC=np.zeros((sample_envs, N, 3, 3), np.float32),
             gF=np.zeros((sample_envs, N, 3, 3), np.float32), gppos=np.zeros((sample_envs, S, 3), np.float32))
    threads = min(sample_envs, os.cpu_count() or 1)
    t_f = t_b = 0.0
    for _ in range(steps):
        t0 = time.time()
        o = orc.step_fwd(ost, nthreads=threads)
        t_f += time.time() - t0
        t0 = time.time()
        orc.step_bwd(ost, g, clip=True, nthreads=threads)
        t_b += time.time() - t0
        ost.update(x=o["x"], v=o["v"], C=o["C"], F=o["F"], J=o["J"], ppos=o["ppos"], prot=o["prot"])
    n = sample_envs * steps * S
    return {"value": n / (t_f + t_b), "unit": "substeps/s", "cores": threads, "kind": "port",
            "sample": f"CPU restatement (C++ -O3 -march=native, f32, dense res grid like the reference; not JAX-CPU): {sample_envs} envs x {steps} "
                      f"simulator.steps x {S} substeps, forward {t_f:.2f}s + adjoint (with its own state recompute) {t_b:.2f}s, "
                      f"OpenMP over envs ({threads} threads)"}


def bench_fold_tshirt(args, rank, world, device):
    """fold_tshirt: 3573-particle T-shirt, k = 5000, dt = 0.5e-3, 4 envs per GPU like the headline.
    One "step" = one env.step_diff (40 x 50 substeps) + the backward of the reward to the pick-and-place action."""
    import torch.distributed as dist
    from unidom_amd.envs.registration import env_functions
    B = args.cloth_envs or 4
    env = env_functions["fold_tshirt"](batch_size=B, aux_reward=True, device=device)
    _, st = env.reset(np.array([0, 5 + rank], np.uint32))
    g = torch.Generator(device=device).manual_seed(rank)
    xm = st.x.mean(1)
    off = (torch.rand((B, 2), device=device, generator=g) - 0.5) * 0.2
    act = torch.stack([xm[:, 0] + off[:, 0], torch.zeros_like(off[:, 0]), xm[:, 2] + off[:, 1],
                       xm[:, 0] - off[:, 0], torch.zeros_like(off[:, 0]), xm[:, 2] - off[:, 1]], -1).contiguous().requires_grad_(True)

    def one():
        act.grad = None
        _, reward, _, _ = env.step_diff(act, st)
        reward.sum().backward()

    def sync():
        torch.cuda.synchronize(device)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(device)

    for _ in range(args.warmup):
        one()
    env.simulator.profile = {"fwd": [], "bwd": []}
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one()
    sync()
    dt = time.perf_counter() - t0
    prof, env.simulator.profile = env.simulator.profile, None
    assert torch.isfinite(act.grad).all()
    tm = torch.tensor([dt], device=device, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(tm, op=dist.ReduceOp.MAX)
    dt = float(tm[0])
    if rank == 0:
        P = st.x.shape[1]
        cluster = not getattr(env.conf, "one_workgroup_per_env", False)   # csrc/cloth.hip::cloth_use_cluster; launches of <= n_cu // parts envs
        units = world * B * MACRO * SUBSTEPS * args.steps
        k_ms = {k: float(np.mean([a.elapsed_time(b) for a, b in vv])) for k, vv in prof.items() if vv}
        dom = max(k_ms, key=k_ms.get)
        per_launch = B * MACRO * SUBSTEPS * P * (72 if dom == "bwd" else 48)     # 48 / 72 B per particle-substep
        achieved = per_launch / (k_ms[dom] * 1e-3) / 1e9
        print(json.dumps({
            "metric": "substeps_per_sec_fwd_bwd", "value": units / dt, "unit": "substeps/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic", **dist_info(world),
            "config": {"workload": f"fold_tshirt (mass-spring cloth, P={P} on a 180x180 lattice) step_diff + backward to the action, {B} envs per GPU"},
            "roofline": {"bound": "hbm", "kernel": ("cloth_cluster_bwd_kernel" if dom == "bwd" else "cloth_cluster_fwd_kernel") if cluster
                         else ("cloth_big_bwd_kernel" if dom == "bwd" else "cloth_big_fwd_kernel"), "achieved": achieved,
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": pmc_traffic("cloth_cluster_bwd_kernel" if dom == "bwd" else "cloth_cluster_fwd_kernel") if cluster and B == 4 else None,
                         "kernel_ms": k_ms, "algorithmic_bytes_per_launch": per_launch,
                         "issue": issue_roof("cloth_cluster_bwd_kernel" if dom == "bwd" else "cloth_cluster_fwd_kernel", k_ms[dom], B * -(-P // 512) * 8,
                                             min(256, B * -(-P // 512)), MACRO * SUBSTEPS) if cluster else None,
                         "note": (f"{-(-P // 512)} workgroups of 512 lanes per env (one particle per lane), halo positions / force cotangents / "
                                  "block sums exchanged through HBM every substep; 2000 sequential substeps per launch") if cluster else
                                 "one workgroup of 1024 lanes per env, 4 particles per lane, 2000 sequential substeps per launch"},
            **({"cpu_baseline": cpu_baseline_tshirt(env, st, min(B, 4))} if not (args.no_cpu_baseline or world > 1) else {})}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def bench_shape_rope(args, rank, world, device):
    """shape_rope: 582 plastic particles, 64x6x64 grid, box pusher in soft-contact mode
    (collide_batch).  One "step" = one env.step_diff -- 30 scanned simulator.steps of 133 substeps -- plus the backward
    of the reward to the push action, for `--envs` envs per GPU (the reference's shape_rope has no training script:
    this is the env-level loss + gradient that APG would drive)."""
    import torch.distributed as dist
    from unidom_amd.envs.registration import env_functions
    B = args.envs
    env = env_functions["shape_rope"](batch_size=B, seed=rank, device=device)
    env.build_reset_state()
    st = env.state
    sim = env.simulator
    N, S, T = sim.n_particles, env.conf.steps, env.conf.primitive_action_steps
    g = torch.Generator(device=device).manual_seed(rank)
    mid = st.x[:, N // 2]
    ang = torch.rand((B,), device=device, generator=g) * 6.2831853
    off = torch.stack([torch.cos(ang), torch.zeros_like(ang), torch.sin(ang)], -1)
    act = torch.cat([mid - 0.02 * off, mid + 0.08 * off], -1).contiguous().requires_grad_(True)   # start 5 mm from the rope

    def one():
        act.grad = None
        obs, reward, done, info = env.step_diff(act, st)
        reward.sum().backward()

    def sync():
        torch.cuda.synchronize(device)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(device)

    for _ in range(args.warmup):
        one()
    sim.check_status()
    sim.profile = {"fwd": [], "bwd": []}
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one()
    sync()
    dt = time.perf_counter() - t0
    prof, sim.profile = sim.profile, None
    assert torch.isfinite(act.grad).all()
    tm = torch.tensor([dt], device=device, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(tm, op=dist.ReduceOp.MAX)
    dt = float(tm[0])
    if rank == 0:
        units = world * B * T * S * args.steps
        cpu = None if (args.no_cpu_baseline or world > 1) else cpu_baseline_shape_rope(env, st, act)
        g_host = touched_cells(st.x[0].detach().cpu().numpy() + 0.0, env.conf.n_grid)
        g_act = device_active_cells(sim, one, device) or g_host
        k_ms = {k: float(np.mean([a.elapsed_time(b) for a, b in vv])) for k, vv in prof.items() if vv}
        dom = max(k_ms, key=k_ms.get)
        per_launch = B * S * ((192 * N + 56 * g_act) if dom == "fwd" else (288 * N + 112 * g_act))
        achieved = per_launch / (k_ms[dom] * 1e-3) / 1e9
        print(json.dumps({
            "metric": "mpm_substeps_per_sec_fwd_bwd", "value": units / dt, "unit": "substeps/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic", **dist_info(world),
            "config": {"workload": f"shape_rope (MLS-MPM plastic rope N={N}, res 64x6x64, soft contact, {T} x {S} substeps/env.step) "
                                   f"step_diff + backward to the push action, {B} envs per GPU", "touched_cells": g_act,
                       "touched_cells_host_count_of_one_input_state": g_host},
            "roofline": {"bound": "hbm", "kernel": lg_label(dom, env.simulator, B),
                         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": pmc_traffic(f"large_path:shape_rope:{dom}") if B == 32 else None,
                         "issue": lg_issue(f"large_path:shape_rope:{dom}", k_ms[dom]) if B == 32 else None,
                         "kernel_ms": k_ms, "algorithmic_bytes_per_launch": per_launch,
                         "note": f"latency / issue bound: {B} x {N} particles do not fill the chip (four lanes per particle)"},
            **({"cpu_baseline": cpu} if cpu else {})}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-saturation", action="store_true", help="skip the many-env probe of the same kernels")
    ap.add_argument("--no-graph", action="store_true", help="whip_rope: eager update instead of the captured HIP graph")
    ap.add_argument("--graph", action="store_true", help="cloth workloads: also time the update replayed as one HIP graph (reported as `hip_graph`, beside the eager `value`)")
    ap.add_argument("--workload", default="fold_cloth1", choices=["fold_cloth1", "fold_cloth1_para", "fold_tshirt", "whip_rope", "torus", "shape_rope", "pour_water", "pour_soup", "selftest"],
                    help="fold_cloth1 = the headline metric (default); fold_cloth1_para = BASELINE config 3 (parameter-aware obs, "
                         "32 envs/GPU); whip_rope = the MPM path (BASELINE config 4 shape: 32 envs/GPU)")
    ap.add_argument("--cloth-envs", type=int, default=None, help="cloth workloads: envs per GPU (default 4; 32 for fold_cloth1_para)")
    ap.add_argument("--n-grid", type=int, default=64, help="whip_rope only: 64 (default env, N=67), 128 (N=798) or 256 (N=6675): "
                    "the scaled configurations of SURVEY.md 8(d), simulator-level (the env's goal/obs sizes are tied to N=67)")
    ap.add_argument("--envs", type=int, default=32, help="whip_rope only: envs per GPU")
    ap.add_argument("--grid-ckpt", type=int, default=2, help="scaled whip_rope only: ud_mpm_conf.grid_ckpt_cells (0 = the backward "
                    "recomputes p2g + grid op instead of restoring the checkpointed grid)")
    ap.add_argument("--plb-grad", action="store_true", help="torus only: forward with checkpoints + loss + adjoint instead of the forward rollout")
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=INT",
                    help="MPM workloads, diagnostics only: ud_mpm_conf.tune_* of every simulator this run builds (lanes, cluster, cluster_part_lanes, "
                         "cluster_envs, env_groups, bwd_two_launch, collide_records), e.g. --tune env_groups=1 for counter passes that attribute per kernel")
    ap.add_argument("--kernel-mode", type=int, default=0,
                    help="cloth kernel family (include/unidom_hip.h): 0 default (v2-order forward, bit-exact vs the restatement of that order), "
                         "1 reference-order forward + literal adjoint, 2 fast-math, 3 reference-order forward + restructured adjoint")
    ap.add_argument("--full", action="store_true",
                    help="fold_cloth1 / fold_cloth1_para: also run what the headline figure does not need -- the forward-only rate, the same update "
                         "in the reference's operation order, the many-env saturation probe and the CPU baselines (each still subject to its "
                         "--no-* switch).  Off: set up, warm up, time --steps updates, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="fold_cloth1 / fold_cloth1_para: after the timed steps, write what the last timed update returned (loss, per-step "
                         "reward, gradient norm) and left behind (the clipped flat policy gradient, the updated flat policy parameters) "
                         "as DIR/<name>.npy, float32")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1 (ms_per_step is the time of one timed step)")
    if args.dump_outputs and args.workload not in ("fold_cloth1", "fold_cloth1_para"):
        ap.error("--dump-outputs is implemented for the fold_cloth1 / fold_cloth1_para line only")
    if args.gpus > 1 and "RANK" not in os.environ:
        self_launch(sys.argv[1:])              # never returns; nothing above has touched a GPU

    from unidom_amd.algorithms.apg.core import APG, init_distributed
    from unidom_amd.envs.registration import env_functions
    from unidom_amd.utils import prng

    rank, world, device = init_distributed(args.gpus)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    if args.tune:
        from unidom_amd.engine.mpm_simulator import SimpleMPMSimulator
        SimpleMPMSimulator.default_tuning = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in args.tune}
    if args.workload == "selftest":
        return bench_selftest(args, rank, world, device)
    if args.workload == "torus":
        return bench_torus(args, rank, world, device)
    if args.workload == "shape_rope":
        return bench_shape_rope(args, rank, world, device)
    if args.workload == "fold_tshirt":
        return bench_fold_tshirt(args, rank, world, device)
    if args.workload == "whip_rope" and args.n_grid != 64:
        return bench_mpm_scaled(args, rank, world, device)
    if args.workload == "whip_rope":
        return bench_whip_rope(args, rank, world, device)
    if args.workload in ("pour_water", "pour_soup"):
        return bench_whip_rope(args, rank, world, device, name=args.workload)

    global NUM_ENVS_PER_GPU
    para = args.workload == "fold_cloth1_para"
    NUM_ENVS_PER_GPU = args.cloth_envs if args.cloth_envs else (32 if para else 4)
    from unidom_amd.envs.fold_cloth1_env import DefaultConf
    conf = DefaultConf()
    conf.kernel_mode = args.kernel_mode
    if para:   # apg_para.py: stiffness drawn from [train_min_stiff, train_max_stiff] = [1000, 1600], obs normalised with [10, 1800]
        env = env_functions["fold_cloth1_para"](batch_size=NUM_ENVS_PER_GPU, conf=conf, aux_reward=True, stiffness=1300,
                                                eval_min_max_stiff=[10, 1800], device=device)
    else:
        env = env_functions["fold_cloth1"](batch_size=NUM_ENVS_PER_GPU, conf=conf, seed=0, aux_reward=True, device=device)
    want_graph = args.graph and world == 1      # opt-in: the headline `value` below stays the eager update; the graph replay is reported beside it
    if want_graph:                               # APG.capture: the learner's whole life on one non-default stream
        work = torch.cuda.Stream(device)
        work.wait_stream(torch.cuda.current_stream(device))
        torch.cuda.set_stream(work)
    learner = APG(env, EP_LEN, learning_rate=1e-4, max_gradient_norm=0.3, seed=0)
    key_env = prng.split(prng.PRNGKey(0), world)[rank]
    _, state = env.reset(key_env)
    env.simulator.profile = None

    def sync():
        torch.cuda.synchronize(device)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(device)

    for _ in range(args.warmup):
        learner.minimize(state)
    env.simulator.profile = {"fwd": [], "bwd": []}   # HIP events around every kernel launch, on its stream
    learner.sync.profile = []                        # ... and around the gradient all-reduce (N > 1)
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = learner.minimize(state)
    sync()
    dt = time.perf_counter() - t0
    prof = env.simulator.profile
    env.simulator.profile = None
    ranks = rank_report(world, device, dt, {k: float(np.mean([a.elapsed_time(b) for a, b in v])) for k, v in prof.items() if v}, learner.sync)
    learner.sync.profile = None
    if args.dump_outputs and rank == 0:   # before anything below touches the learner again
        dump_outputs(args.dump_outputs, {"loss": last["loss"], "reward": last["reward"], "grad_norm": last["grad_norm"],
                                         "policy_grad": learner.flat_grad,
                                         "policy_params": torch.cat([p.detach().reshape(-1) for p in learner.params])})

    graph_line = None
    if want_graph:
        try:
            learner.capture(state)
            learner.minimize_captured()
            sync()
            tg0 = time.perf_counter()
            for _ in range(args.steps):
                learner.minimize_captured()
            sync()
            dtg = time.perf_counter() - tg0
            graph_line = {"value": NUM_ENVS_PER_GPU * EP_LEN * MACRO * SUBSTEPS * args.steps / dtg, "ms_per_step": dtg / args.steps * 1e3,
                          "note": "the same update replayed as one HIP graph (APG.capture); not the headline value"}
        except Exception as e:
            graph_line = {"error": f"{type(e).__name__}: {e}"}

    # forward-only rate (BASELINE config 2), untimed region of the main metric
    dt_fwd = float("nan")
    if args.full:
        with torch.no_grad():
            sync()
            tf0 = time.perf_counter()
            for _ in range(args.steps):
                learner.evaluate(state, EP_LEN)
            sync()
            dt_fwd = time.perf_counter() - tf0

    # the same update in the reference's LITERAL operation order (ud_cloth_conf.mode 3: cloth_simulator.py:257-337 as written, forward
    # bit-exact vs the restatement of that order + the restructured adjoint), timed exactly like the headline -- reported beside it
    ref_line, dt_ref, k_ms_ref = None, float("nan"), {}
    if args.full and args.kernel_mode == 0:
        conf3 = DefaultConf()
        conf3.kernel_mode = 3
        if para:
            env3 = env_functions["fold_cloth1_para"](batch_size=NUM_ENVS_PER_GPU, conf=conf3, aux_reward=True, stiffness=1300,
                                                     eval_min_max_stiff=[10, 1800], device=device)
        else:
            env3 = env_functions["fold_cloth1"](batch_size=NUM_ENVS_PER_GPU, conf=conf3, seed=0, aux_reward=True, device=device)
        assert env3.simulator.mode == 3
        learner3 = APG(env3, EP_LEN, learning_rate=1e-4, max_gradient_norm=0.3, seed=0)
        _, state3 = env3.reset(key_env)
        for _ in range(args.warmup):
            learner3.minimize(state3)
        env3.simulator.profile = {"fwd": [], "bwd": []}
        sync()
        tr0 = time.perf_counter()
        for _ in range(args.steps):
            learner3.minimize(state3)
        sync()
        dt_ref = time.perf_counter() - tr0
        k_ms_ref = {k: float(np.mean([a.elapsed_time(b) for a, b in v])) for k, v in env3.simulator.profile.items() if v}
        env3.simulator.profile = None

    t_max = torch.tensor([dt, dt_fwd, dt_ref], device=device, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t_max, op=dist.ReduceOp.MAX)
    dt, dt_fwd, dt_ref = float(t_max[0]), float(t_max[1]), float(t_max[2])

    if rank == 0:
        units = world * NUM_ENVS_PER_GPU * EP_LEN * MACRO * SUBSTEPS * args.steps
        k_ms = {k: float(np.mean([a.elapsed_time(b) for a, b in v])) for k, v in prof.items() if v}
        dom = max(k_ms, key=k_ms.get)
        kname = {"fwd": {0: "cloth_rollout_fwd_v2_kernel", 1: "cloth_rollout_fwd_kernel", 2: "cloth_rollout_fwd_fast_kernel",
                         3: "cloth_rollout_fwd_ref_kernel"}[args.kernel_mode],
                 "bwd": "cloth_rollout_bwd_kernel" if args.kernel_mode == 1 else "cloth_rollout_bwd_fast_kernel"}[dom]
        per_launch = NUM_ENVS_PER_GPU * MACRO * SUBSTEPS * (BYTES_BWD if dom == "bwd" else BYTES_FWD)
        achieved = per_launch / (k_ms[dom] * 1e-3) / 1e9
        # the PMC passes were taken on the headline shape (4 envs per launch); null once the kernel sources have changed
        traffic = pmc_traffic(kname) if NUM_ENVS_PER_GPU == 4 else None
        out = {
            "metric": "substeps_per_sec_fwd_bwd", "value": units / dt, "unit": "substeps/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{args.workload} (mass-spring cloth, P=512) APG loss+grad+update: num_envs={NUM_ENVS_PER_GPU} per GPU, "
                                   "ep_len=3, 40 macro x 50 substeps per step_diff",
                       "kernel_mode": args.kernel_mode,
                       "order": {0: "v2 (the reference's formulas re-associated; bit-exact vs the CPU restatement of the same order)",
                                 1: "reference (literal operation order), literal six-reduction adjoint", 2: "v2 fast-math",
                                 3: "reference (literal operation order; bit-exact vs the CPU restatement of that order) + restructured adjoint"}[args.kernel_mode],
                       "num_envs_per_gpu": NUM_ENVS_PER_GPU, "ep_len": EP_LEN, "substeps_per_step": units // args.steps,
                       "parallelism": f"env-sharded dp{world}, 1 RCCL all-reduce of {learner.n_params} f32 per update"},
            "n_ranks_seen": dist.get_world_size() if dist.is_initialized() else 1,
            "allreduce_bytes_per_update": learner.n_params * 4 if world > 1 else 0,
            "roofline": {"bound": "hbm", "kernel": kname, "achieved": achieved,
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                         "kernel_ms": k_ms, "algorithmic_bytes_per_launch": per_launch,
                         "note": "latency/occupancy bound: 4 envs = 4 workgroups on 256 CUs, 2000 sequential substeps; the HBM fraction says nothing "
                                 "about this kernel -- see `issue` (instruction issue on the busy CUs) and `saturation`",
                         "issue": issue_roof(kname, k_ms[dom], 8 * NUM_ENVS_PER_GPU, NUM_ENVS_PER_GPU, MACRO * SUBSTEPS)},
        }
        if args.full:
            out["fwd_only_substeps_per_sec"] = units / dt_fwd
        if args.full and args.kernel_mode == 0:
            out["reference_order"] = {
                "value": units / dt_ref, "unit": "substeps/s", "ms_per_step": dt_ref / args.steps * 1e3, "kernel_ms": k_ms_ref, "kernel_mode": 3,
                "kernels": {"fwd": "cloth_rollout_fwd_ref_kernel", "bwd": "cloth_rollout_bwd_fast_kernel"},
                "roofline": (lambda dk, kn: {"bound": "hbm", "kernel": kn, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                             "achieved": NUM_ENVS_PER_GPU * MACRO * SUBSTEPS * (BYTES_BWD if dk == "bwd" else BYTES_FWD) / (k_ms_ref[dk] * 1e-3) / 1e9,
                                             "frac": NUM_ENVS_PER_GPU * MACRO * SUBSTEPS * (BYTES_BWD if dk == "bwd" else BYTES_FWD) / (k_ms_ref[dk] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                             "traffic": pmc_traffic(kn) if NUM_ENVS_PER_GPU == 4 else None,
                                             "issue": issue_roof(kn, k_ms_ref[dk], 8 * NUM_ENVS_PER_GPU, NUM_ENVS_PER_GPU, MACRO * SUBSTEPS)})(
                    max(k_ms_ref, key=k_ms_ref.get), {"fwd": "cloth_rollout_fwd_ref_kernel", "bwd": "cloth_rollout_bwd_fast_kernel"}[max(k_ms_ref, key=k_ms_ref.get)]) if k_ms_ref else None,
                "note": "the SAME update (same policy seed, same reset key, same steps / warm-up, same barrier-bracketed timing) with the cloth forward in the "
                        "reference's literal operation order (cloth_simulator.py:264-268 k*r/len*(len-L0)/L0 and the friction block :281-306 as written, "
                        "IEEE divide / sqrt, no FMA contraction): bit-exact against ClothOracle(order=1) over a whole step_diff incl. the grasp set of every "
                        "substep (tests/test_cloth_gpu.py::test_reference_order_*); the adjoint is the restructured one of the headline, reading this "
                        "forward's checkpoints.  The CPU figure in the same order: cpu_baseline.reference_order"}
        out.update(ranks)
        if graph_line is not None:
            out["hip_graph"] = graph_line
        if args.full and not args.no_saturation:
            out["saturation"] = saturation_probe(env, device)
        if args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(sample_envs=min(NUM_ENVS_PER_GPU, max(4, host_cores())),
                                               gpu_order=1 if args.kernel_mode in (1, 3) else 2)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
