#!/usr/bin/env python3
"""bench.py -- body-pair interactions/s of the brute-force N-body step (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run does what the headline figure needs and no more: set-up, W warm-up steps, K timed steps, the JSON line (metric, value,
unit, ms_per_step, the roofline of the kernel times taken inside the timed steps).  `--dump-outputs DIR` also writes the state the
last timed step left (what a caller of the step reads back) as DIR/<name>.npy.  `--full` adds everything that takes runs of its
own: the CPU baseline, the steady-state loop, the general-masses run, the rocprofv3 counter passes, the self-check of a multi-GPU
run, the per-kernel pass of a Barnes-Hut run and the companion configs.

One "step" = one nb_step_brute_force (rs-src/nbody.rs:106-162): all-pairs force + kick-drift over
the whole synthetic system.  Workload: N = 262 144-body Plummer sphere (3-D float4 kernel,
17 algorithmic flops / interaction), the configuration the metric is quoted on; it fits one GPU.
With N GPUs the SAME system is sharded as slabs of targets (strong scaling, the reference's own
thread split nbody.rs:426-428) with one all-gather of (x,y,z,m) per step.  Inputs are resident in
HBM before the timed region.  Prints ONE JSON line on rank 0.

Three hosts drive the same library (`--host`, default auto):
  single  one engine on one GPU (N = 1)
  group   ONE process, N GPUs: the library's own multi-GPU group (nbx_group_*: one engine per device,
          ncclCommInitAll + one in-place ncclAllGather per step issued by the library; no torch).
          This is what a plain `python bench.py --gpus N` runs for N > 1.
  torch   one process per GPU under `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`
          (WORLD_SIZE is set): torch.distributed (backend nccl = RCCL) does the all-gather on torch-owned memory.

`--workload bh`: one step = nb_step_barnes_hut(theta, dt) (nbody.rs:186-480) on N bodies (BASELINE config #4:
--n 1048576 --theta 0.5): ms/step split host build / flatten / upload / eval, CPU oracle step beside it.
"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from bench_support import (DT, GroupHost, SingleHost, TorchHost, measure_counters, measure_traffic,  # noqa: E402
                           steady_state, effective_cores, cpu_facts, CPU_LAW, GPU_LAW_2D, GPU_LAW_3D)

FLOPS_PER_INTERACTION = 17   # 3 sub, 3 mul + 2 add, 1 add eps, 1 mul, 1 div, 3 mul, 3 add

KERNEL_NAMES = {1: "k_force_tile_pk", 6: "k_force_smem_pkw<unit_mass=0>", 7: "k_force_smem_pkw<unit_mass=1>", 16: "k_force_tile_pk_h",
                17: "k_force_smem_pkw<unit_mass=0,self_image=1> on the widened fp16 copy", 18: "k_force_smem_pkw<unit_mass=1,self_image=1> on the widened fp16 copy",
                -1: "k_force_strict", -8: "k_force_strict_pc<8,8>", -16: "k_force_strict_pc<16,4>"}


def _use_built(module, so):
    """A benchmark run measures the library that build() left and compiles nothing: a compile at the first step would count against
    the run, and whoever benchmarks may only be allowed to read the tree. So the module's own build step, which takes a lock file
    beside the library, is left out when the library is there. Where it is missing that step runs, and fails, as before."""
    if os.path.exists(so):
        module.build = lambda force=False: so


def load_product():
    import rust_exp_amd as rx

    _use_built(rx.engine, rx.lib_path())
    return rx


def load_oracle():
    from oracle import binding as ob

    _use_built(ob, ob._SO)
    return ob


def cpu_baseline(st, seconds):
    """Oracle (CPU restatement of nbody.rs:132-144) on the host cores: a bounded i-slice of the same
    workload (work per target is uniform), threads = all cores with the reference's slab split."""
    ob = load_oracle()

    n = len(st["px"])
    cores = effective_cores()
    p = ob.particles(st["px"], st["py"], st["vx"], st["vy"], st["m"])   # the reference law is 2-D: z ignored
    # calibrate
    ni = min(n, 16 * cores)
    t0 = time.perf_counter(); ob.brute_forces(p, 0, ni, nthreads=cores); t1 = time.perf_counter()
    rate = ni * (n - 1) / max(t1 - t0, 1e-9)
    ni = int(min(n, max(ni, rate * seconds / (n - 1))))
    ni -= ni % cores or 0
    ni = max(ni, cores)
    t0 = time.perf_counter(); ob.brute_forces(p, 0, ni, nthreads=cores); t1 = time.perf_counter()
    mt = ni * (n - 1) / (t1 - t0)
    n1 = max(1, min(n, int(ni / cores)))
    t0 = time.perf_counter(); ob.brute_forces(p, 0, n1, nthreads=1); t2 = time.perf_counter()
    st1 = n1 * (n - 1) / (t2 - t0)
    return {
        "value": mt, "unit": "interactions/s", "cores": cores, "kind": "port", **cpu_facts(cores), "law": CPU_LAW,
        "sample": f"first {ni} targets x {n} sources (2-D reference law), {cores} threads, reference slab split",
        "single_thread_value": st1,
        "single_thread_sample": f"first {n1} targets x {n} sources, 1 thread (the reference's brute force is single-threaded)",
    }


def cpu_baseline_barnes_hut(st, theta, dt, threads, reps):
    """The CPU-baseline leg of the Barnes-Hut measurements: the oracle's nb_step_barnes_hut
    (nbody.rs:186-480: serial tree build + `threads` traversal workers) timed on the host cores. Median ms per step."""
    ob = load_oracle()

    p = ob.particles(st["px"], st["py"], st["vx"], st["vy"], st["m"])
    ts, rc = [], 0
    for _ in range(reps):
        t0 = time.perf_counter(); rc = ob.step_barnes_hut(p, theta, dt, threads); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, rc


def bh_accuracy(st, theta, engine, threads):
    """Checker leg (cpu_baseline only): the forces of the engine that was just timed, on the INITIAL state at full size, against
    the oracle's fp64 arbiter (orc_bh_forces_exact: the reference's tree and opening law, exact node sums, fp64 arithmetic) and
    against the oracle's own f32 traversal (orc_bh_forces, nbody.rs:333-377) -- errors relative to max|F|, over ALL bodies.
    DESIGN.md section 4 allows the exact-sum tree class (device tree above 65 536 bodies) 0.1 % of bodies on a flipped opening
    decision, bounded by 2e-3: here that allowance is a measured figure of this run."""
    ob = load_oracle()

    n = len(st["px"])
    p = ob.particles(st["px"], st["py"], st["vx"], st["vy"], st["m"])
    t0 = time.perf_counter()
    rc, ex, ey = ob.bh_forces_exact(p, theta, nthreads=threads)
    rc2, ofx, ofy = ob.bh_forces(p, theta, nthreads=threads)
    t1 = time.perf_counter()
    if rc != 0 or rc2 != 0:
        return {"error": f"oracle rc {rc} / {rc2}"}
    engine.set_particles(st["px"], st["py"], st["vx"], st["vy"], st["m"], st["pz"], st["vz"])
    gx, gy, _ = engine.forces(theta)
    scale = float(max(np.abs(ofx).max(), np.abs(ofy).max()))
    dev_arb = np.maximum(np.abs(gx - ex), np.abs(gy - ey)) / scale
    orc_arb = np.maximum(np.abs(ofx - ex), np.abs(ofy - ey)) / scale
    dev_orc = np.maximum(np.abs(gx - ofx), np.abs(gy - ofy)) / scale
    q = lambda a, f: float(np.percentile(a, f))   # noqa: E731
    return {"vs": "orc_bh_forces_exact (fp64 arbiter on the reference's tree), all bodies, relative to max|F|",
            "bodies": n, "p50": q(dev_arb, 50), "p99": q(dev_arb, 99), "p999": q(dev_arb, 99.9), "max": float(dev_arb.max()),
            "bodies_beyond_2e-5": int((dev_arb > 2e-5).sum()), "bodies_beyond_2e-4": int((dev_arb > 2e-4).sum()),
            "allowance": "p99.9 <= 2e-5, max <= 2e-3 (DESIGN.md section 4, exact-sum tree class; a body beyond 2e-5 sits on at least "
                         "one opening decision that the exactly rounded node records flip relative to the arbiter)",
            "within_allowance": bool(q(dev_arb, 99.9) <= 2e-5 and dev_arb.max() <= 2e-3),
            "oracle_f32_vs_arbiter": {"p999": q(orc_arb, 99.9), "max": float(orc_arb.max()),
                                      "note": "the reference's own f32 node folds against the same arbiter"},
            "vs_oracle_f32": {"p999": q(dev_orc, 99.9), "max": float(dev_orc.max())},
            "oracle_seconds": t1 - t0, "threads": threads}


REFERENCE_PUBLISHED_MS = 30.75   # screenshot.png, top-middle panel (2016 desktop, 1 thread)


def reference_scene_line(no_cpu_baseline=False, frames=90):
    """BASELINE.md section 1, the one number the reference publishes, measured the way its caller measures it
    (hs-src/RustNBodyExperiment.hs): withExperiment -> nb_stable_orbits 10000 0.5 30.0 (:42); every frame timeIt(nb_step_barnes_hut
    0.85 0.01 1) (:55-57) then nb_draw 512 512 (:58-60); the status line shows the MEDIAN of the last 30 step times (:44, :62,
    :65).  All through the SIX level-1 symbols -- the process-global engine, the drop-in's everyday path.  Beside it (cpu_baseline
    leg): BASELINE.md section 3 row CB -- the oracle's nb_step_barnes_hut on the same seeded scene, 1 thread, median of 30 -- and
    the force error of an engine in the level-1 configuration against the oracle's own traversal (orc_bh_forces, nbody.rs:333-377)."""
    os.environ.setdefault("NB_SEED", "1")
    rx = load_product()

    theta, dt, nthreads, n = 0.85, 0.01, 1, 10000
    rx.nb_stable_orbits(n, 0.5, 30.0)
    times, draws = [], []
    for _ in range(frames):
        t0 = time.perf_counter()
        rx.nb_step_barnes_hut(theta, dt, nthreads)
        t1 = time.perf_counter()
        rx.nb_draw(512, 512)
        t2 = time.perf_counter()
        times.append(t1 - t0); draws.append(t2 - t1)
    ms = float(np.median(times[-30:])) * 1e3
    # an engine in the same (default) configuration, same seed: which tree served the steps, and the checker's state
    e = rx.NBodyEngine()
    e.seed(1)
    e.stable_orbits(n, 0.5, 30.0)
    st = e.get_particles()
    for _ in range(5):
        e.step_barnes_hut(theta, dt, nthreads)
    e.synchronize()
    tree = {0: "host (reference-faithful insertion build)", 1: "device (bh_build.hip), exact sums"}[e.get_stat(rx.engine.NBX_STAT_BH_LAST_TREE)]
    out = {"metric": "ms per nb_step_barnes_hut call, reference default scene (10 000-body nb_stable_orbits, theta 0.85, dt 0.01, 1 thread), "
                     "median of the last 30 wall-clocked calls", "value": ms, "unit": "ms", "higher_is_better": False, "n_gpus": 1,
           "steps": frames, "warmup": frames - 30, "ms_per_step": ms, "draw_ms": float(np.median(draws[-30:])) * 1e3, "dtype": "f32",
           "data": "synthetic (seeded preset, NB_SEED=1)", "published_ms_per_step": REFERENCE_PUBLISHED_MS,
           "vs_baseline": REFERENCE_PUBLISHED_MS / ms,
           "vs_baseline_note": "published figure / this figure: other hardware (a 2016 desktop CPU), read off screenshot.png +-1 in the last digit",
           "config": {"workload": "reference_default_scene_nb_stable_orbits_N10000_theta0.85_dt0.01_level1_symbols", "bodies": n,
                      "tree": tree, "how": "RustNBodyExperiment.hs:42-65: timeIt around the FFI call, nb_draw 512x512 between calls, median of 30"},
           "bh_fallbacks": e.get_stat(rx.engine.NBX_STAT_BH_FALLBACKS)}
    if not no_cpu_baseline:
        ob = load_oracle()

        p = ob.particles(st["px"], st["py"], st["vx"], st["vy"], st["m"])
        q = p.copy()
        ts = []
        for _ in range(30):
            t0 = time.perf_counter(); rc = ob.step_barnes_hut(q, theta, dt, 1); ts.append(time.perf_counter() - t0)
        rc2, ofx, ofy = ob.bh_forces(p, theta, nthreads=effective_cores())
        e.set_particles(st["px"], st["py"], st["vx"], st["vy"], st["m"])
        gx, gy, _ = e.forces(theta)
        scale = float(max(np.abs(ofx).max(), np.abs(ofy).max()))
        err = np.maximum(np.abs(gx - ofx), np.abs(gy - ofy)) / scale
        out["cpu_baseline"] = {"value": float(np.median(ts)) * 1e3, "unit": "ms per step", "ms_per_step": float(np.median(ts)) * 1e3, "cores": 1,
                               "kind": "port", **cpu_facts(effective_cores()), "rc": rc,
                               "law": "nb_step_barnes_hut as written (nbody.rs:186-480), 1 thread like the published figure",
                               "sample": "BASELINE.md section 3 row CB: the oracle on the same seeded scene, 30 consecutive steps, median",
                               "accuracy": {"vs": "orc_bh_forces (the oracle's own f32 tree and traversal), initial state, all bodies, relative to max|F|",
                                            "p50": float(np.percentile(err, 50)), "p999": float(np.percentile(err, 99.9)), "max": float(err.max()),
                                            "rc": rc2}}
    e.close()
    return out


def _claim_stdout():
    """RCCL (and other C libraries) print banners to the C stdout ("RCCL version : ..." at communicator
    creation, flushed at exit). The contract is ONE JSON line on stdout, so keep a private handle to the real
    stdout for that line and point file descriptor 1 at stderr for everything else in this process."""
    sys.stdout.flush()
    real = os.dup(1)
    os.dup2(2, 1)
    return real


# ---- companions: the other BASELINE configs, timed by the same driver-run command ----------------------
COMPANIONS = (
    # key, BASELINE config, argv of the child run
    ("c0_reference_scene", "the reference's own default scene and the ONE number it publishes (BASELINE.md section 1): nb_stable_orbits(10000, 0.5, "
                           "30.0), nb_step_barnes_hut(0.85, 0.01, 1) through the six level-1 symbols, median of the last 30 wall-clocked calls",
     ["--workload", "reference_scene"]),
    ("c2_brute_65536", "65 536-body Plummer sphere, brute-force fp32 on 1 MI355X",
     ["--bodies", "65536", "--steps", "300", "--warmup", "60", "--steady-seconds", "0", "--no-general-masses", "--no-traffic",
      "--cpu-seconds", "2"]),
    ("c4_barnes_hut_1048576", "1 048 576 bodies Barnes-Hut theta=0.5 on 1 GPU",
     ["--workload", "bh", "--bodies", "1048576", "--theta", "0.5", "--steps", "40", "--warmup", "5", "--steady-seconds", "0"]),
    ("c5_fp16_sources_524288", "524 288-body two-galaxy collision, fp16 positions / fp32 accumulators (1 of its 8 GPUs' worth: whole system on 1 GPU)",
     ["--workload", "two_galaxies", "--bodies", "524288", "--source-bits", "16", "--dim", "2", "--steps", "10", "--warmup", "2",
      "--steady-seconds", "0", "--no-general-masses", "--no-traffic", "--cpu-seconds", "2"]),
    # not a BASELINE config (round 6): config #4's model at twice its size, 35 steps into its collapse -- where rounds 2-5
    # handed every few steps to a 50-85 ms host build (chains of bodies within EPS, nbody.rs:249-260); c6_fallbacks counts such steps
    ("c6_barnes_hut_2097152", "2 097 152 bodies Barnes-Hut theta=0.5 on 1 GPU (beyond BASELINE: config #4's model at twice the size, through its collapse)",
     ["--workload", "bh", "--bodies", "2097152", "--theta", "0.5", "--steps", "30", "--warmup", "5", "--steady-seconds", "0", "--no-traffic"]),
)


def companion_summary(key, line):
    """The few numbers of a child's JSON line that the parent's line carries (scalars only: flat and short)."""
    r, cb = line.get("roofline") or {}, line.get("cpu_baseline") or {}
    out = {"value": line.get("value"), "unit": line.get("unit"), "ms_per_step": line.get("ms_per_step"), "steps": line.get("steps"),
           "frac": r.get("frac"), "kernel_avg_ms": r.get("kernel_avg_ms"), "cpu_value": cb.get("value"), "cpu_cores": cb.get("cores")}
    if key.startswith("c0"):
        acc = cb.get("accuracy") or {}
        return {"ms_per_step": line.get("value"), "cpu_ms_per_step": cb.get("ms_per_step"), "cpu_cores": cb.get("cores"),
                "published_ms_per_step": line.get("published_ms_per_step"), "draw_ms": line.get("draw_ms"), "frames": line.get("steps"),
                "tree": (line.get("config") or {}).get("tree"), "host_hand_overs": line.get("bh_fallbacks"),
                "err_p999": acc.get("p999"), "err_max": acc.get("max"), "err_vs": acc.get("vs")}
    if key.startswith(("c4", "c6")):
        sp, acc = line.get("ms_split") or {}, cb.get("accuracy") or {}
        out.update({"build_ms": sp.get("tree_build"), "traversal_ms": sp.get("bh_eval_kernel"), "tree": (line.get("config") or {}).get("tree"),
                    "fallbacks": line.get("bh_fallbacks"),
                    "valu_busy": r.get("valu_busy_frac"), "traffic_bytes": r.get("traffic"),
                    "algorithmic_bytes": r.get("hbm_algorithmic_bytes_per_launch"), "flops_per_launch": r.get("flops_per_launch"),
                    "cpu_ms_per_step": cb.get("ms_per_step"),
                    "err_p999": acc.get("p999"), "err_max": acc.get("max"), "bodies_beyond_2e-5": acc.get("bodies_beyond_2e-5"),
                    "err_vs": acc.get("vs")})
    else:
        out.update({"flops_per_interaction": r.get("flops_per_interaction"), "kernel": r.get("kernel")})
    return out


def run_companions(base_argv=(), timeout=150):
    """BASELINE configs #2, #4 and #5 as short child runs of THIS script, after the official window (and after the parent's
    engine is closed): each child prints its own full JSON line; the parent keeps a summary. A child that fails is reported, it
    does not take the official line with it."""
    out = {}
    for key, what, argv in COMPANIONS:
        t0 = time.perf_counter()
        row = {"config": what, "argv": " ".join(argv)}
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--no-companions"] + list(base_argv) + argv,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=dict(os.environ))
            lines = [ln for ln in r.stdout.decode(errors="replace").splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not lines:
                row["error"] = "rc %d: %s" % (r.returncode, r.stderr.decode(errors="replace")[-300:])
            else:
                row.update(companion_summary(key, json.loads(lines[-1])))
        except (subprocess.TimeoutExpired, OSError, ValueError) as ex:
            row["error"] = repr(ex)
        row["wall_s"] = time.perf_counter() - t0
        out[key] = row
    return out


def flatten_companions(comp):
    """Scalar keys for the roofline object (the driver's parser keeps scalars one level deep)."""
    flat = {}
    for key, row in comp.items():
        short = key.split("_")[0]
        for k, v in row.items():
            if k in ("config", "argv", "wall_s", "unit", "steps", "kernel", "tree", "err_vs", "cpu_cores", "flops_per_interaction", "frames"):
                continue
            if isinstance(v, (int, float, str)) or v is None:
                flat[f"{short}_{k}"] = v
    return flat


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", "--bodies", dest="n", type=int, default=0,
                    help="bodies (default 262144; 1048576 for --workload bh). Under torch.distributed.run spell it --bodies: the "
                         "launcher's own parser treats --n as an ambiguous abbreviation of --nnodes / --nproc-per-node")
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--mode", default="fast")
    ap.add_argument("--jsplit", type=int, default=0)
    ap.add_argument("--bpt", type=int, default=0)
    ap.add_argument("--variant", type=int, default=-1)
    ap.add_argument("--strict-kernel", type=int, default=0, choices=[0, 1, 8, 16],
                    help="bit-exact mode: 0 = by size; 16 / 8 = waves per 64-target workgroup; 1 = one thread per body")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--workload", default="plummer", choices=["plummer", "two_galaxies", "stable_orbits", "bh", "reference_scene"],
                    help="stable_orbits = the reference's own preset (nb_stable_orbits n 0.5 30, seed 1; 2-D: unit planets + a 1000-mass sun); "
                         "reference_scene = the reference's default scene through the six nb_* symbols, timed as its caller times it")
    ap.add_argument("--theta", type=float, default=0.5, help="--workload bh: opening angle")
    ap.add_argument("--bh-tree", default="default", choices=["default", "host", "device"])
    ap.add_argument("--bh-walk", type=int, default=-1, choices=[-1, 0, 1, 2],
                    help="--workload bh, fast mode: 1 = walk over child groups, hand-scheduled (round 4, default), 2 = the same walk "
                         "compiled, 0 = node walk of rounds 1-3")
    ap.add_argument("--source-bits", type=int, default=32, choices=[16, 32],
                    help="16 = fp16 source copy / fp32 accumulators (BASELINE config #5)")
    ap.add_argument("--host", default="auto", choices=["auto", "single", "group", "torch"])
    ap.add_argument("--torch-path", action="store_true", help="same as --host torch (kept for round-1 command lines)")
    ap.add_argument("--shard-of", type=int, default=0,
                    help="single GPU: run only rank 0's slab of an N-way shard (per-GPU shape of an N-GPU run; not the metric)")
    ap.add_argument("--no-traffic", action="store_true", help="skip the in-run rocprofv3 PMC passes (roofline.traffic = null)")
    ap.add_argument("--verify", dest="verify", action="store_true", default=None,
                    help="after the timed loop: --verify-steps more steps on this host AND on one plain engine from the same state; "
                         "bit-exact mode must agree bit for bit, fast mode within the stated tolerance (default: on when --gpus > 1)")
    ap.add_argument("--no-verify", dest="verify", action="store_false")
    ap.add_argument("--verify-steps", type=int, default=2)
    ap.add_argument("--steady-seconds", type=float, default=3.0,
                    help="single GPU: after the official steps, a back-to-back loop of at least this many seconds for the "
                         "steady_state block (clock and socket power from rocm-smi); 0 = skip")
    ap.add_argument("--no-general-masses", action="store_true",
                    help="skip the general_masses block (the same run on random masses: the kernel with the m_j multiply)")
    ap.add_argument("--dry-run", action="store_true",
                    help="first contact with a multi-GPU node: create the communicator, run ONE exchange of the real payload and ONE "
                         "verified step, print what was found (rccl_ranks, exchange microseconds, per-rank kernel ms, verify) and exit")
    ap.add_argument("--no-companions", action="store_true",
                    help="skip the companions block (BASELINE configs #2, #4, #5 as short child runs after the official window)")
    ap.add_argument("--no-accuracy", action="store_true",
                    help="--workload bh: skip the full-size force-error check against the oracle's fp64 arbiter (cpu_baseline leg)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline figure: CPU baseline, steady-state loop, general-masses run, rocprofv3 counter "
                         "passes, the self-check of a multi-GPU run, the per-kernel pass of --workload bh, the companions block "
                         "(each still has its --no-... switch)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps: the state the last timed step left, as DIR/<name>.npy (float32)")
    ap.add_argument("--traffic-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


DUMP_LIMIT_BYTES = 60 * 1000 * 1000   # of array data: with the .npy headers the files stay under 64 MB in all


def dump_outputs(directory, host):
    """--dump-outputs: what the timed path computed in its last step, i.e. the arrays a caller reads back after it (positions,
    velocities, masses), one DIR/<name>.npy each. Beyond DUMP_LIMIT_BYTES in all: the same seeded sample of bodies from every array.
    Every rank calls this (the torch host's get_state is a collective); rank 0 writes."""
    host.sync(); host.barrier()
    st = host.get_state()
    if host.rank != 0:
        return
    arrays = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in st.items()}
    n = len(next(iter(arrays.values())))
    keep = DUMP_LIMIT_BYTES // (4 * len(arrays))
    if n > keep:
        idx = np.sort(np.random.default_rng(0x5EED).choice(n, keep, replace=False))
        arrays = {k: v[idx] for k, v in arrays.items()}
    os.makedirs(directory, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(directory, k + ".npy"), v)


def make_state(args, rx):
    """The workload from the library's own C-ABI generators (nbx_plummer_sphere / nbx_two_galaxies: what any host behind
    the boundary gets; bit-identical to rust-exp_amd/presets.py, tests/test_workload_generators.py)."""
    e = rx.NBodyEngine()
    if args.workload == "bh":
        e.plummer_sphere(args.n, dim=2)   # the reference (and its quadtree) is 2-D
    elif args.workload == "plummer":
        e.plummer_sphere(args.n, dim=args.dim)
    elif args.workload == "stable_orbits":
        e.seed(1)
        e.stable_orbits(args.n, 0.5, 30.0)
    else:
        e.two_galaxies(args.n)
    st = e.get_particles()
    e.close()
    return st


def verify_against_plain_engine(host, args, rx, step, is_bh, device):
    """Self-validation of whatever host ran the timed loop (a group over RCCL, one process per GPU, ...): from the state
    the timed loop left, `--verify-steps` more steps here AND on ONE plain engine holding all bodies. Bit-exact mode: every
    position and velocity bit-equal. Fast mode: within the stated tolerance (rust-exp_amd/tolerances.py), x2 because two
    fast results are compared (each is within the bound of the reference arithmetic). Every rank calls this; rank 0 judges."""
    kv = max(1, args.verify_steps)
    host.sync(); host.barrier()
    s0 = host.get_state()
    for _ in range(kv):
        step()
    host.sync(); host.barrier()
    s1 = host.get_state()
    if host.rank != 0:
        return None
    ref = rx.NBodyEngine(device=device, mode=args.mode)
    ref.set_source_precision(args.source_bits)
    ref.set_strict_kernel(args.strict_kernel)
    if args.bh_tree != "default":
        ref.set_bh_tree(args.bh_tree)
    ref.set_particles(s0["px"], s0["py"], s0["vx"], s0["vy"], s0["m"], s0["pz"], s0["vz"])
    n = len(s0["px"])
    fx, fy, fz = ref.forces(args.theta if is_bh else 0.0)
    a = np.sqrt(fx.astype(np.float64) ** 2 + fy.astype(np.float64) ** 2 + fz.astype(np.float64) ** 2) / np.maximum(s0["m"].astype(np.float64), 1e-30)
    amax = float(a.max()) if n else 0.0
    for _ in range(kv):
        if is_bh:
            ref.step_barnes_hut(args.theta, DT, 1)
        else:
            ref.step_brute_force(DT)
    r1 = ref.get_particles()
    ref.close()
    dp = max(float(np.abs(s1[k] - r1[k]).max()) if n else 0.0 for k in ("px", "py", "pz"))
    dv = max(float(np.abs(s1[k] - r1[k]).max()) if n else 0.0 for k in ("vx", "vy", "vz"))
    bit_equal = all(np.array_equal(s1[k].view(np.uint32), r1[k].view(np.uint32)) for k in ("px", "py", "pz", "vx", "vy", "vz"))
    moved = max(float(np.abs(s1[k] - s0[k]).max()) if n else 0.0 for k in ("px", "py", "pz"))
    from rust_exp_amd.tolerances import fast_step_tolerances

    ptol, vtol = fast_step_tolerances(amax, n, DT, kv)
    ptol, vtol = 2.0 * ptol, 2.0 * vtol
    finite = all(np.isfinite(s1[k]).all() for k in ("px", "py", "pz", "vx", "vy", "vz"))
    ok = finite and (bit_equal if args.mode == "strict" else (dp <= ptol and dv <= vtol))
    return {"ok": bool(ok), "steps": kv, "mode": args.mode, "bit_equal": bool(bit_equal), "max_dp": dp, "max_dv": dv,
            "tol_dp": None if args.mode == "strict" else ptol, "tol_dv": None if args.mode == "strict" else vtol,
            "max_displacement": moved, "max_accel": amax,
            "how": f"{kv} more steps on this host and on one plain engine (all {n} bodies, GPU {device}) from the state the timed loop "
                   "left; strict = bit-equal, fast = 2 x the stated tolerance (two fast results are compared)"}


# ---- first contact with a multi-GPU node must say WHERE it failed -------------------------------------
DIAG = {"stage": "start"}


def stage(name, **facts):
    """Where the run is; what is known so far. Printed (stderr, every rank; stdout line, rank 0) if the run dies."""
    DIAG["stage"] = name
    DIAG.update(facts)


def multi_gpu_fields(per, host_kind, world, is_bh, group_info=None, backend="nccl"):
    """The multi-GPU part of the JSON line from plain data (no GPU, no library): per = one dict per rank with its slab, the
    average ms of its dominant kernel inside the timed loop and -- single-process group -- the all-gather as its stream saw it."""
    kk = "bh_eval_ms" if is_bh else "force_ms"
    out = {"per_gpu": per,
           "rank_skew": {"kernel_ms_min": min(r[kk] for r in per), "kernel_ms_max": max(r[kk] for r in per),
                         "note": "per-rank average of the dominant kernel inside the timed loop (HIP events on each rank's stream)"}}
    if host_kind == "group":
        xs = [r["exchange_us"] for r in per]
        out["all_gather_us_per_step"] = float(np.mean(xs))
        out["rank_skew"].update({"exchange_us_min": min(xs), "exchange_us_max": max(xs),
                                 "exchange_note": "as seen from each rank's stream: includes the wait for the slowest peer"})
        gi = group_info or {}
        out["exchange"] = gi.get("exchange")
        out["rccl_ranks"] = gi.get("rccl_ranks")
        out["enqueue_threads"] = gi.get("enqueue_threads")
        if gi.get("note"):
            out["exchange_note"] = gi["note"]
    elif host_kind == "torch":
        out["exchange"] = "torch.distributed " + backend
        out["rccl_ranks"] = world if backend == "nccl" else 0
    return out


def per_gpu_rows(host, rx, host_kind, world):
    """Per-engine kernel times (HIP events on each engine's own stream) as plain rows; gathered over the ranks for the torch host."""
    per = []
    for e in host.engines:
        k_ms, k_cnt = e.profile_read(rx.NBX_K_FORCE)
        i_ms, i_cnt = e.profile_read(rx.NBX_K_INTEGRATE)
        b_ms, b_cnt = e.profile_read(rx.NBX_K_BH_EVAL)
        x_ms, x_cnt = e.profile_read(rx.NBX_K_EXCHANGE)
        t_ms, t_cnt = e.profile_read(rx.NBX_K_TREE_BUILD)
        lo, hi = e.slab()
        per.append({"slab": [lo, hi], "force_ms": k_ms / max(k_cnt, 1), "force_launches": k_cnt,
                    "integrate_ms": i_ms / max(i_cnt, 1), "bh_eval_ms": b_ms / max(b_cnt, 1), "bh_eval_launches": b_cnt,
                    "exchange_us": 1e3 * x_ms / max(x_cnt, 1), "exchanges": x_cnt,
                    "device_tree_build_ms": t_ms / max(t_cnt, 1), "device_tree_builds": t_cnt})
        e.profile(False)
    if host_kind == "torch" and world > 1:
        rows = host.gather_floats([per[0]["slab"][0], per[0]["slab"][1], per[0]["force_ms"], per[0]["force_launches"],
                                   per[0]["integrate_ms"], per[0]["bh_eval_ms"], per[0]["bh_eval_launches"]])
        per = [{"slab": [int(r[0]), int(r[1])], "force_ms": r[2], "force_launches": int(r[3]), "integrate_ms": r[4],
                "bh_eval_ms": r[5], "bh_eval_launches": int(r[6]), "exchange_us": None, "exchanges": 0} for r in rows]
        per[0]["exchange_us"] = None   # torch's collective runs on ProcessGroupNCCL's own stream: see ms_per_step minus kernels
    return per


def dry_run(host, args, rx, step, is_bh, host_kind, real_stdout):
    """--dry-run: the communicator exists (host construction), now ONE exchange of the real payload, ONE profiled step and ONE
    verified step; one JSON line saying what was found. Exit code 0 = the multi-GPU path works on this node."""
    stage("dry-run: first exchange (communicator already created)")
    host.sync(); host.barrier()
    t0 = time.perf_counter()
    host.prepare(args.theta if is_bh else 0.0)
    host.sync(); host.barrier()
    first_exchange_ms = (time.perf_counter() - t0) * 1e3
    stage("dry-run: one profiled step", first_exchange_ms=first_exchange_ms)
    for e in host.engines:
        e.profile(True); e.profile_reset()
    t0 = time.perf_counter()
    step()
    host.sync(); host.barrier()
    step_ms = host.reduce_max(time.perf_counter() - t0) * 1e3
    per = per_gpu_rows(host, rx, host_kind, host.world)
    stage("dry-run: one verified step", step_ms=step_ms)
    args.verify_steps = 1
    verify = verify_against_plain_engine(host, args, rx, step, is_bh, getattr(host, "local_rank", 0))
    stage("dry-run: done")
    if host.rank == 0:
        out = {"dry_run": True, "n_gpus": host.world, "host": host_kind, "bodies": args.n, "workload": args.workload,
               "first_exchange_ms_including_setup": first_exchange_ms, "one_step_ms": step_ms, "verify": verify}
        out.update(multi_gpu_fields(per, host_kind, host.world, is_bh,
                                    host.group.info() if host_kind == "group" else None, os.environ.get("NBX_DIST_BACKEND", "nccl")))
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    host.close()
    if verify is not None and not verify["ok"]:
        sys.exit(3)


def main():
    real_stdout = _claim_stdout()
    rank = int(os.environ.get("RANK", "0"))
    try:
        run(real_stdout)
    except SystemExit:
        raise
    except BaseException as ex:   # noqa: BLE001 -- whatever it is, say where
        import traceback

        diag = dict(DIAG, rank=rank, world_size=int(os.environ.get("WORLD_SIZE", "1")), error=repr(ex),
                    traceback=traceback.format_exc().splitlines()[-6:])
        sys.stderr.write("bench.py: FAILED at stage '%s' on rank %d: %s\n" % (DIAG["stage"], rank, json.dumps(diag)))
        if rank == 0:   # still one JSON line on stdout: no value, but where it died and what was known by then
            os.write(real_stdout, (json.dumps({"metric": None, "value": None, "error": repr(ex), "diagnostics": diag}) + "\n").encode())
        sys.exit(4)


def run(real_stdout):
    # multi-process GPU work on this stack needs dmabuf IPC (exported by the driver; harmless to restate)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    args = parse_args()
    if args.workload == "reference_scene":   # companion c0: its own line, nothing of the all-pairs machinery
        os.write(real_stdout, (json.dumps(reference_scene_line(args.no_cpu_baseline or not args.full)) + "\n").encode())
        return
    if args.n <= 0:
        args.n = 1048576 if args.workload == "bh" else 262144
    env_world = int(os.environ.get("WORLD_SIZE", "1"))
    host_kind = args.host
    if args.torch_path:
        host_kind = "torch"
    if host_kind == "auto":
        host_kind = "torch" if env_world > 1 else ("group" if args.gpus > 1 else "single")
    if host_kind == "torch" and env_world != args.gpus and not (env_world == 1 and args.gpus == 1):
        sys.exit(f"bench.py --host torch: WORLD_SIZE={env_world} but --gpus {args.gpus} (launch with torch.distributed.run, "
                 f"or drop --host torch to use the single-process group)")
    if host_kind == "single" and args.gpus != 1:
        sys.exit("--host single is one GPU")

    if host_kind == "torch":
        import torch  # noqa: F401  (before the HIP library: both then share torch's HIP runtime, see sharded.py)
    rx = load_product()

    n = args.n
    stage("initial conditions", host=host_kind, gpus=args.gpus, bodies=n, workload=args.workload)
    st = make_state(args, rx)
    stage("host construction: engines, communicator (ncclCommInitAll / init_process_group)")
    host = {"single": SingleHost, "group": GroupHost, "torch": TorchHost}[host_kind](args, rx, st)
    world, rank = host.world, host.rank
    is_bh = args.workload == "bh"
    if host_kind == "group":
        gi0 = host.group.info()
        stage("host constructed", world=world, exchange=gi0["exchange"], rccl_ranks=gi0["rccl_ranks"], exchange_note=gi0["note"])
    else:
        stage("host constructed", world=world, backend=os.environ.get("NBX_DIST_BACKEND", "nccl") if host_kind == "torch" else None)

    def step():
        if is_bh:
            host.step_bh(args.theta)
        else:
            host.step_brute()

    if args.dry_run:
        return dry_run(host, args, rx, step, is_bh, host_kind, real_stdout)
    # inputs resident in HBM, every buffer allocated and the communicator created before anything is timed, whatever
    # --warmup says; the W warm-up steps follow
    stage("first exchange (allocations, communicator warm-up)")
    host.prepare(args.theta if is_bh else 0.0)
    if host_kind == "group":
        gi0 = host.group.info()
        stage("warm-up steps", exchange=gi0["exchange"], rccl_ranks=gi0["rccl_ranks"], exchange_note=gi0["note"])
    else:
        stage("warm-up steps")
    if args.traffic_child:
        for _ in range(3):
            step()
        host.sync()
        host.close()
        return
    for _ in range(args.warmup):
        step()
    host.sync()
    # Per-kernel HIP events: inside the timed region for the all-pairs workloads (4 event records per 12 ms step).  A Barnes-Hut
    # step is a chain of 15-20 short kernels and every event record costs it ~7 us of pipeline bubble (0.24 -> 0.30 ms at
    # 10 000 bodies): its timed region runs WITHOUT events, and the per-kernel split comes from a second pass of the same steps.
    profile_in_region = not is_bh
    for e in host.engines:
        e.profile(profile_in_region)      # creates its events now, outside the timed region
        e.profile_reset()
        e.bh_host_timing()
    host.barrier(); host.sync()
    stage("timed steps")
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    host.sync(); host.barrier()
    t1 = time.perf_counter()
    elapsed = host.reduce_max(t1 - t0)
    if args.dump_outputs:
        stage("dump outputs", ms_per_step=elapsed / args.steps * 1e3)
        dump_outputs(args.dump_outputs, host)
    stage("per-rank kernel times", ms_per_step=elapsed / args.steps * 1e3)
    if not profile_in_region and args.full:
        for e in host.engines:
            e.profile(True)
            e.profile_reset()
            e.bh_host_timing()
        for _ in range(args.steps):
            step()
        host.sync(); host.barrier()

    # per-engine kernel times (HIP events on each engine's own stream, inside the timed region)
    per = per_gpu_rows(host, rx, host_kind, world)
    stage("verify / steady state / companions", per_gpu=per)

    engine = host.eng
    launch = engine.last_launch()   # of the timed loop (the blocks below launch other shapes)
    dev0 = getattr(host, "local_rank", 0)
    do_verify = args.verify if args.verify is not None else (args.full and world > 1)
    verify = None
    if do_verify and args.shard_of <= 1:
        verify = verify_against_plain_engine(host, args, rx, step, is_bh, dev0)
    steady = None
    if args.full and host_kind == "single" and args.steady_seconds > 0 and args.shard_of <= 1:
        steady = steady_state(host, step, args.steady_seconds)
    general = None
    if (args.full and host_kind == "single" and not is_bh and args.shard_of <= 1 and not args.no_general_masses and args.mode == "fast"
            and args.variant < 0 and args.source_bits == 32 and launch["variant"] == 7):
        # The same run on UNEQUAL masses (nb_random_disk's range, nbody.rs:62): positions unchanged, every body its own mass
        # -> no common mass -> the wave-split kernel WITH the per-interaction multiply by m_j (variant 6). What a caller
        # whose masses are all different gets; the headline workload (and nb_stable_orbits: one common mass + the sun) runs 7.
        g = SingleHost(args, rx, dict(st, m=np.random.default_rng(0x5EED).uniform(0.1, 1.5, n).astype(np.float32)))
        g.prepare()
        for _ in range(max(args.warmup, 2)):
            g.step_brute()
        g.sync()
        g.eng.profile(True); g.eng.profile_reset()
        tg0 = time.perf_counter()
        for _ in range(args.steps):
            g.step_brute()
        g.sync()
        tg1 = time.perf_counter()
        gk_ms, gk_cnt = g.eng.profile_read(rx.NBX_K_FORCE)
        g.eng.profile(False)
        gl = g.eng.last_launch()
        g_flops = FLOPS_PER_INTERACTION if gl["dim"] == 3 else 12
        g_peak = rx.device_info(dev0)["peak_fp32_flops"] / 1e12
        g_ach = float(n) * float(n - 1) * g_flops / (gk_ms / max(gk_cnt, 1) * 1e-3) / 1e12
        general = {"value": float(n) * float(n - 1) * args.steps / (tg1 - tg0), "unit": "interactions/s",
                   "ms_per_step": (tg1 - tg0) / args.steps * 1e3, "kernel": KERNEL_NAMES.get(gl["variant"], "k_force"),
                   "launch": gl, "kernel_avg_ms": gk_ms / max(gk_cnt, 1), "achieved": g_ach, "frac": g_ach / g_peak,
                   "flops_per_interaction": g_flops, "flops_executed_per_interaction": g_flops,
                   "masses": "uniform [0.1, 1.5) (nb_random_disk's range, nbody.rs:62), same positions, same steps/warmup, timed in this run"}
        g.eng.close()

    if rank == 0:
        info = rx.device_info(dev0)
        peak = info["peak_fp32_flops"] / 1e12
        ms_per_step = elapsed / args.steps * 1e3
        out = {"n_gpus": world if host_kind != "single" else 1, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
               "data": "synthetic"}
        sharding = ("single GPU" if world == 1 else
                    f"slab x{world} (reference split nbody.rs:426-428), one all-gather of "
                    f"{'half4' if args.source_bits == 16 and not is_bh else 'float4'} (x,y,z,m) per step; host = "
                    + ("one process, library-issued RCCL (nbx_group_*)" if host_kind == "group" else "one process per GPU, torch.distributed " + os.environ.get("NBX_DIST_BACKEND", "nccl")))
        if not is_bh:
            interactions_per_step = float(n) * float(n - 1)
            if args.shard_of > 1:
                lo, hi = engine.slab()
                interactions_per_step = float(hi - lo) * float(n - 1)
            value = interactions_per_step * args.steps / elapsed
            flops_per_inter = FLOPS_PER_INTERACTION if launch["dim"] == 3 else 12
            # variant 7 (one common mass): the multiply by m_j leaves the loop -> one flop fewer EXECUTED per interaction
            flops_executed = flops_per_inter - (1 if launch["variant"] in (7, 18) else 0)
            # dominant kernel: K1. Roofline from the SLOWEST rank's launches (the step waits for it).
            worst = max(per, key=lambda r: r["force_ms"])
            inter_per_launch = float(worst["slab"][1] - worst["slab"][0]) * float(n - 1)
            k_avg_s = worst["force_ms"] * 1e-3
            achieved = inter_per_launch * flops_per_inter / k_avg_s / 1e12
            slab_rows = worst["slab"][1] - worst["slab"][0]
            # algorithmic HBM bytes of one K1 launch (~16 B x N sources read once + 16 B per target read);
            # the per-split partial-acceleration slabs K1 writes for K2 are NOT algorithmic: they show up in `traffic`
            algorithmic = 16.0 * n + 16.0 * slab_rows
            traffic, traffic_info = None, None
            if args.full and world == 1 and not args.no_traffic:
                tail = [a for a in sys.argv[1:] if a not in ("--no-cpu-baseline",)]
                traffic_info = measure_traffic(tail + ["--no-cpu-baseline", "--no-traffic"], "k_force")
                if traffic_info:
                    traffic = traffic_info["bytes_per_launch"]
            # Instruction-mix ceiling of the packed sweep ("Why K1 stops"): per wave and source -- 128 interactions, two
            # targets per lane -- 3 (2-D: 2) v_pk_add for d, 3 (2) v_pk_fma for r^2 + eps, 2 v_rcp_f32, [1 v_pk_mul by m_j unless every
            # body has the same mass], 3 (2) v_pk_fma for the sums; issue cost per wave64 instruction and SIMD, measured
            # (tools/ubench_valu.hip; PMC of the kernel: 4.87 cycles per VALU instruction against this mix's 4.73): packed 3.85
            # cycles, v_rcp_f32 8.7 (quarter rate, nothing overlaps it).  A SIMD's peak is 64 flop per cycle.
            def mix_ceiling(dim, unit_mass):
                pk = 3 * dim + (0 if unit_mass else 1)
                return (17.0 if dim == 3 else 12.0) * 128.0 / (pk * 3.85 + 2 * 8.7) / 64.0
            packed = launch["variant"] in (1, 6, 7, 17, 18)
            ceiling = mix_ceiling(launch["dim"], launch["variant"] in (7, 18)) if packed else None
            if general:
                general["ceiling_frac"] = mix_ceiling(general["launch"]["dim"], False)
                general["frac_of_ceiling"] = general["frac"] / general["ceiling_frac"]
            out.update({
                "metric": f"body-pair interactions/s at N={n} (brute-force O(N^2) step)",
                "value": value, "unit": "interactions/s",
                "dtype": "f32" if args.source_bits == 32 else "f32 (fp16 source copy)",
                "config": {"workload": f"{ {'plummer': 'plummer_sphere'}.get(args.workload, args.workload) }_N{n}_brute_force_dim{launch['dim']}_dt{DT}"
                                       + ("_fp16sources" if args.source_bits == 16 else "")
                                       + (f"_rank0_of_{args.shard_of}_slab_only" if args.shard_of > 1 else ""),
                           "bodies": n, "seed": "0x5EED0001", "force_mode": args.mode, "host": host_kind,
                           "sharding": sharding, "launch": launch,
                           "kernel_note": (("roofline fraction: %.3f general masses (conservative: what a caller whose masses all differ, e.g. "
                                            "nb_random_disk, gets -- variant 6, timed in this run under general_masses) / %.3f equal masses "
                                            "(this workload). " % (general["frac"], achieved / peak) if general else "")
                                           + "Every body of this workload has the same mass, so the unit-mass sweep runs (variant 7: the "
                                           "per-interaction multiply by m_j is hoisted out of the loop: 16 flops executed of the 17 "
                                           "counted, see roofline.frac_executed). It also serves 'one common mass + a handful of "
                                           "exceptions' (nb_stable_orbits: unit planets + the sun)")
                                          if launch["variant"] == 7 else None},
                "roofline": {"bound": "valu_fp32",
                             "peak_definition": "fp32 vector FMA peak = CUs x clock x 256 flop/clk (157.3 TFLOP/s at 256 CUs, 2.4 GHz); "
                                                "the contract's hbm|mfma classes do not fit: no MFMA is used and HBM is not the bound",
                             "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                             "ceiling_frac": ceiling, "frac_of_ceiling": (achieved / peak / ceiling) if ceiling else None,
                             "ceiling_note": ("what this kernel's own instruction mix allows at the nominal 2.4 GHz: 17 (12) flop x 128 "
                                              "interactions / (packed ops x 3.85 + 2 v_rcp_f32 x 8.7 issue cycles) / 64 flop per cycle and "
                                              "SIMD; the sweep runs with the VALU 97 % busy at the board's power cap -- valu_busy_frac 0.971 (equal masses) / 0.974 "
                                              "(general masses), effective clock 2.23 of 2.4 GHz under the profiler: this round's counters, "
                                              "profiles/r06_pmc_summary.json (tools/gpu_session.sh k1pmc) -- so what is left between frac and "
                                              "ceiling_frac is that clock, not idle issue slots") if ceiling else
                                             ("no mix ceiling is quoted for the bit-exact kernels: frac counts the reference's 17 (12) flops "
                                              "per interaction against the plain fp32 peak, while the kernel executes the reference's "
                                              "arithmetic as written -- unfused multiplies and adds, an IEEE-correct sqrt and divide "
                                              "(expanded into ~10 instructions each) and the per-target sum in ascending j, one rounding "
                                              "at a time; those are what bit-exactness costs, not idle issue slots (DESIGN.md 5 K1s)"),
                             "general_masses_frac": general["frac"] if general else None,
                             "frac_conservative": general["frac"] if general else achieved / peak,
                             "traffic": traffic, "traffic_measurement": traffic_info,
                             "kernel": KERNEL_NAMES.get(launch["variant"], "k_force"),
                             "kernel_avg_ms": k_avg_s * 1e3, "kernel_launches": worst["force_launches"],
                             "flops_per_interaction": flops_per_inter, "flops_executed_per_interaction": flops_executed,
                             "frac_executed": achieved / peak * flops_executed / flops_per_inter,
                             "interactions_per_launch": inter_per_launch,
                             "hbm_algorithmic_bytes_per_launch": algorithmic,
                             "partial_slab_bytes_written_per_launch": 16.0 * slab_rows * launch.get("acc_slabs", launch["jsplit"]),
                             "note": "VALU-bound path (arithmetic intensity ~1e5 flop/B): peak = CUs*clock*256 flop/clk "
                                     "(fp32 vector FMA roofline, = the f32 MFMA rate); HBM is not the bound. With several GPUs: the "
                                     "slowest rank's kernel (its slab x all sources per launch)"},
                "integrate_kernel_avg_ms": per[0]["integrate_ms"],
            })
            if general:
                out["general_masses"] = general
        else:
            value = float(n) * args.steps / elapsed
            walk_kind = engine.get_option(rx.engine.NBX_OPT_BH_WALK) if args.mode == "fast" else 0
            out.update({
                "metric": f"bodies/s through nb_step_barnes_hut (theta={args.theta}) at N={n}",
                "value": value, "unit": "body-steps/s", "dtype": "f32",
                "config": {"workload": f"plummer_disk_projection_N{n}_barnes_hut_theta{args.theta}_dt{DT}", "bodies": n,
                           "seed": "0x5EED0001", "force_mode": args.mode, "host": host_kind, "sharding": sharding,
                           "tree": {0: "host (reference-faithful insertion build)", 1: "device (bh_build.hip)"}[engine.get_stat(rx.engine.NBX_STAT_BH_LAST_TREE)],
                           "walk": {0: "node by node (bh_eval.hip, rounds 1-3)", 1: "child groups, hand-scheduled loop (bh_walk.hip)",
                                    2: "child groups, compiled loop (bh_walk.hip)"}[walk_kind]},
                # steps of this run that the device tree was selected for but the host tree served (a refused build: EPS crowds,
                # an exhausted pool, a warm sort whose buckets overflowed) -- each costs ~20 ms at a million bodies
                "bh_fallbacks": engine.get_stat(rx.engine.NBX_STAT_BH_FALLBACKS),
                "bh_last_refusal": "0x%x" % engine.get_stat(rx.engine.NBX_STAT_BH_REFUSAL),
            })
        if is_bh and args.full:   # the per-kernel split and the roofline come from the second pass of the steps and from counting passes
            ht = engine.bh_host_timing()
            wk = engine.bh_work_detail(args.theta)
            ev_s = max(per[0]["bh_eval_ms"], 1e-9) * 1e-3     # HIP events around the traversal: (tree -> child groups) + walk
            # the kernels of one traversal, by name: the walk, and (child-group walks) the conversion of the tree before it
            # (the wave form by its template brackets: "k_bh_walk_groups" alone also names k_bh_walk_groups_lane, the per-lane form --
            #  round 4's host-tree line averaged one such launch, 6 GB, into the traffic of the wave walk)
            walk_kernel = "k_bh_walk_groups<" if walk_kind else "k_bh_eval"
            trav_kernels = (walk_kernel, "k_bh_groups(") if walk_kind else (walk_kernel,)
            # ALGORITHMIC flops of one evaluation, counted from the reference as written (2-D, div and sqrt = 1 flop each):
            #   pair law  nbody.rs:164-184 + :358    2 sub, 2 mul + 1 add, 1 add eps, 1 mul, 1 div, 2 mul, 2 add          = 12
            #   opening test nbody.rs:341-345        2 sub, 2 mul + 1 add, 1 sqrt, 1 div (the compare is not counted)      =  7
            # pair laws and opening tests (= visits of interior nodes) are counted by a counting traversal of this state
            flops = 12.0 * wk["pair_evals"] + 7.0 * wk["opening_tests"]
            achieved = flops / ev_s / 1e12
            bh_traffic, bh_traffic_info, issue = None, None, None
            if world == 1 and not args.no_traffic:   # HBM bytes of the traversal kernels, measured now (see measure_traffic)
                tail = [a for a in sys.argv[1:] if a not in ("--no-cpu-baseline",)]
                bh_traffic_info = measure_traffic(tail + ["--no-cpu-baseline", "--no-traffic"], trav_kernels)
                if bh_traffic_info:
                    bh_traffic = bh_traffic_info["bytes_per_launch"]
                # ... and the walk kernel's instruction issue, from counters of this run
                pm = measure_counters(tail + ["--no-cpu-baseline", "--no-traffic"], walk_kernel,
                                      ["SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_ACTIVE_INST_VALU SQ_WAVES SQ_WAVE_CYCLES SQ_INSTS_BRANCH SQ_ACTIVE_INST_SCA",
                                       "GRBM_GUI_ACTIVE"])
                if pm and pm.get("GRBM_GUI_ACTIVE") and pm.get("SQ_ACTIVE_INST_VALU") and pm.get("SQ_INSTS_SMEM"):
                    n_simd = info["compute_units"] * 4
                    cyc = pm["GRBM_GUI_ACTIVE"] / 8.0                # the counter is summed over the 8 XCDs
                    loads = pm["SQ_INSTS_SMEM"] / (2.0 if walk_kind else 1.0)   # a group turn issues two scalar loads, a node visit one
                    issue = {"valu_busy_frac": 4.0 * pm["SQ_ACTIVE_INST_VALU"] / n_simd / cyc,   # SQ_ACTIVE_INST_* count quad-cycles
                             "scalar_busy_frac": 4.0 * pm.get("SQ_ACTIVE_INST_SCA", 0.0) / n_simd / cyc,
                             "wave_slots_occupied_frac": 4.0 * pm.get("SQ_WAVE_CYCLES", 0.0) / (8.0 * n_simd) / cyc,
                             "valu_insts_per_wave_turn": pm["SQ_INSTS_VALU"] / loads,
                             "salu_insts_per_wave_turn": pm["SQ_INSTS_SALU"] / loads,
                             "branch_insts_per_wave_turn": pm.get("SQ_INSTS_BRANCH", 0.0) / loads,
                             "wave_turns_per_launch": loads, "waves": pm.get("SQ_WAVES"),
                             "turn": "one child group loaded (two scalar loads)" if walk_kind else "one node visited (one scalar load)",
                             "kernel_cycles": cyc, "launches_sampled": pm.get("SQ_INSTS_VALU_launches"),
                             "how": "rocprofv3 --kernel-trace --pmc, two passes (SQ_*; GRBM_GUI_ACTIVE) on a 3-step child run of this "
                                    "command; GRBM_GUI_ACTIVE / 8 = kernel cycles, 1024 SIMDs x 8 wave slots"}
            groups_bytes = 80.0 * ht["nodes"]   # upper bound: an 80-byte record per node (interior ones have one), written once, read once
            algorithmic = 32.0 * ht["nodes"] + 24.0 * n + (2.0 * groups_bytes if walk_kind else 0.0)
            out.update({
                "ms_split": {"bh_eval_kernel": per[0]["bh_eval_ms"], "integrate_kernel": per[0]["integrate_ms"],
                             "host_download": ht["download_ms"],
                             # device tree: GPU time of the build, first launch to last (HIP events); host tree: host wall time
                             "tree_build": per[0]["device_tree_build_ms"] if per[0].get("device_tree_builds") else ht["build_ms"],
                             "flatten": ht["flatten_ms"],
                             "upload_wait": ht["upload_ms"], "tree_nodes": ht["nodes"]},
                "roofline": {"bound": "valu_fp32",
                             "peak_definition": "fp32 vector FMA peak = CUs x clock x 256 flop/clk (157.3 TFLOP/s at 256 CUs, 2.4 GHz); "
                                                "the contract's hbm|mfma classes do not fit: a tree walk is bound by instruction issue",
                             "kernel": " + ".join(k.rstrip("(<") for k in trav_kernels),
                             "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                             "frac_definition": "algorithmic flops of one evaluation (12 per pair law + 7 per opening test, the reference's "
                                                "expressions as written, nbody.rs:164-184, :341-345) / traversal time (HIP events: tree -> "
                                                "child groups + walk; the child-group walk also applies the step's kick-drift, whose "
                                                "flops are not counted) / fp32 vector peak",
                             "flops_per_launch": flops, "pair_evals_per_body": wk["pair_evals"] / n,
                             "opening_tests_per_body": wk["opening_tests"] / n, "node_visits_per_body": wk["node_visits"] / n,
                             "group_loads_per_body": wk["group_loads"] / n,
                             "kernel_avg_ms": per[0]["bh_eval_ms"],
                             "valu_busy_frac": issue["valu_busy_frac"] if issue else None, "issue_counters": issue,
                             "hbm_algorithmic_bytes_per_launch": algorithmic,
                             "hbm_frac_of_8TBps": algorithmic / ev_s / 8e12, "traffic": bh_traffic,
                             "traffic_measurement": bh_traffic_info},
            })
        if world > 1 or host_kind != "single":
            out.update(multi_gpu_fields(per, host_kind, world, is_bh, host.group.info() if host_kind == "group" else None,
                                        os.environ.get("NBX_DIST_BACKEND", "nccl")))
        if verify is not None:
            out["verify"] = verify
        if steady is not None:
            out["steady_state"] = steady
        out.update({"device": info["name"], "arch": info["arch"], "compute_units": info["compute_units"],
                    "clock_khz": info["clock_khz"]})
        if args.full and not args.no_cpu_baseline and world == 1 and args.shard_of <= 1:
            if is_bh:
                cores = min(effective_cores(), 16)
                ms1, rc = cpu_baseline_barnes_hut(st, args.theta, DT, cores, 3 if n > 200000 else 15)
                acc = None
                if not args.no_accuracy and host_kind == "single" and args.mode == "fast":
                    acc = bh_accuracy(st, args.theta, engine, cores)
                out["cpu_baseline"] = {"value": n / (ms1 * 1e-3), "unit": "body-steps/s", "cores": cores, "kind": "port",
                                       **cpu_facts(effective_cores()),
                                       "law": "nb_step_barnes_hut as written (nbody.rs:186-480): serial f32 insertion build, recursive traversal "
                                              "with sqrt + divide per opening test, the 2-D pair law with an IEEE divide",
                                       "ms_per_step": ms1, "rc": rc, "accuracy": acc,
                                       "sample": f"oracle nb_step_barnes_hut on the same {n} bodies: serial tree build + {cores} traversal "
                                                 f"threads (the caller's maximum is 16, hs:94-97), median of {3 if n > 200000 else 15} steps"}
            else:
                out["cpu_baseline"] = cpu_baseline(st, args.cpu_seconds)
                # the two rates are NOT the same work per interaction: say what each side computes
                out["cpu_baseline"]["gpu_law"] = GPU_LAW_3D if out["config"]["launch"]["dim"] == 3 else GPU_LAW_2D
        comp_ok = (args.full and host_kind == "single" and world == 1 and not is_bh and args.workload == "plummer" and n == 262144
                   and args.mode == "fast" and args.variant < 0 and args.source_bits == 32 and args.shard_of <= 1
                   and args.jsplit == 0 and args.bpt == 0 and not args.no_companions)
        if comp_ok:
            # the other BASELINE configs (#2, #4, #5), timed by this same command after the official window;
            # scalars flattened into `roofline` (c2_* / c4_* / c5_*), the block itself last on the line
            host.close()
            comp = run_companions((["--no-cpu-baseline"] if args.no_cpu_baseline else []) + (["--no-traffic"] if args.no_traffic else []))
            out["roofline"].update(flatten_companions(comp))
            out["companions"] = comp
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    host.close()
    if verify is not None and not verify["ok"]:
        sys.stderr.write("bench.py: VERIFY FAILED: %s\n" % json.dumps(verify))
        sys.exit(3)   # a sharded result that differs from the plain engine's is not a measurement


if __name__ == "__main__":
    main()
