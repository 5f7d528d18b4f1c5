"""GPU: the single-process multi-GPU group (nbx_group_*), the host a plain `python bench.py --gpus N` uses.

* several engines sharing the ONE test GPU through the copy exchange (NBX_GROUP_EXCHANGE=copy): the fp16-source
  exchange (round-1 bug: only the fp32 array travelled, so every engine swept stale half4 copies of the other slabs),
  the lazy fp32 re-gather, mode switches in the middle of a run;
* the same checks through real RCCL (ncclCommInitAll + in-place ncclAllGather) when the box has >= 2 GPUs -- skipped
  on the single-GPU test box, there for the first multi-GPU machine this suite meets;
* bench.py's `--gpus N` flow without torch.distributed.run.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_bit_equal, fast_tolerances

pytestmark = pytest.mark.gpu

KEYS = ("px", "py", "vx", "vy")


def _plain(rx, p, mode, bits):
    e = rx.NBodyEngine(mode=mode)
    e.set_source_precision(bits)
    e.set_particles(p["px"], p["py"], p["vx"], p["vy"], p["m"])
    return e


def _check_group_against_plain_engine(rx, ob, devices, n, seed):
    G = len(devices)
    p = ob.stable_orbits(n, 0.5, 30.0, seed)
    dt = 0.01
    for bits in (32, 16):
        g = rx.NBodyGroup(devices, mode="fast")
        g.set_source_precision(bits)
        g.set_particles(p["px"], p["py"], p["vx"], p["vy"], p["m"])
        e = _plain(rx, p, "fast", bits)
        steps = 4
        for _ in range(steps):
            g.step_brute_force(dt); e.step_brute_force(dt)
        g.synchronize()
        a, b = g.get_particles(), e.get_particles()
        # bodies move ~0.3 per step here (v ~ sqrt(1000), nbody.rs:88): sources one step stale are off by 1e4 tolerances
        ptol, vtol = fast_tolerances(ob, p, dt, steps)
        for k in KEYS:
            err = float(np.abs(a[k] - b[k]).max())
            assert err <= (ptol if k[0] == "p" else vtol), (G, bits, k, err, ptol, vtol)
        assert float(np.abs(b["px"] - p["px"]).max()) > 0.1          # the bodies really moved
        # the exchange carried the half4 copy (fp16 run) / the float4 array (fp32 run): one per step either way
        assert g.exchanges() == steps + (1 if (bits == 16 and G > 1) else 0)   # + the lazy fp32 re-gather get_particles() triggered
        # a Barnes-Hut step needs current fp32 positions everywhere (tree build + walk): from the same state it equals the
        # plain engine's BIT FOR BIT (same tree, same per-body walk)
        g.step_brute_force(dt)               # leaves the fp32 copies of other slabs stale again in the fp16 run
        mid = g.get_particles()
        e3 = _plain(rx, mid, "fast", bits)
        g.step_barnes_hut(0.6, dt, 1); e3.step_barnes_hut(0.6, dt, 1)
        g.synchronize()
        a, b = g.get_particles(), e3.get_particles()
        for k in KEYS:
            assert_bit_equal(a[k], b[k], f"G={G} bits={bits} BH after fp16 exchange {k}")
        g.close()
        # a bit-exact step right after fp16-source steps, WITHOUT a get in between: the strict kernel reads the fp32 array
        # of ALL bodies, so the group must re-gather it by itself. Two identical groups (deterministic kernels): one is
        # read back before the strict step (that state goes through the oracle), the other is not.
        from rust_exp_amd.engine import NBX_OPT_FORCE_MODE

        pair = []
        for _ in range(2):
            h = rx.NBodyGroup(devices, mode="fast")
            h.set_source_precision(bits)
            h.set_particles(p["px"], p["py"], p["vx"], p["vy"], p["m"])
            h.step_brute_force(dt); h.step_brute_force(dt)
            pair.append(h)
        pre = pair[0].get_particles()
        pair[1].set_option(NBX_OPT_FORCE_MODE, 1)
        pair[1].step_brute_force(dt)
        got = pair[1].get_particles()
        q = ob.particles(pre["px"], pre["py"], pre["vx"], pre["vy"], pre["m"])
        ob.step_brute_force(q, dt, nthreads=8)
        for k in KEYS:
            assert_bit_equal(got[k], q[k], f"G={G} bits={bits} strict step after fast steps {k}")
        for h in pair:
            h.close()


@pytest.mark.parametrize("G,n", [(2, 8192), (3, 4099), (4, 20000)])
def test_group_fp16_and_fp32_exchange_on_one_gpu(rx, ob, monkeypatch, G, n):
    """VERDICT r01 weak #3 / ADVICE medium: group x NBX_OPT_SOURCE_PRECISION in {32, 16}, >= 3 steps, several engines
    (even and ragged slabs) on the one test GPU via the copy exchange."""
    monkeypatch.setenv("NBX_GROUP_EXCHANGE", "copy")
    _check_group_against_plain_engine(rx, ob, [0] * G, n, 90 + G)


@pytest.mark.parametrize("hook", ["init", "gather"])
def test_group_falls_back_to_peer_copies_when_rccl_fails(rx, ob, monkeypatch, hook):
    """VERDICT r02 next #1b: a failing ncclCommInitAll (or a failing collective) must not kill the run -- the group switches
    to the event-ordered peer-copy exchange, redoes the exchange, and says so. The failure is simulated
    (NBX_GROUP_RCCL_FAIL=init|gather: the only way to meet it on a single-GPU box; 'gather' needs a real communicator, so on
    one GPU it runs with one rank); the state must equal the oracle's bit for bit either way."""
    monkeypatch.delenv("NBX_GROUP_EXCHANGE", raising=False)
    monkeypatch.setenv("NBX_GROUP_RCCL_FAIL", hook)
    have = rx.device_count()
    G = 3 if hook == "init" else min(have, 4)
    devices = [0] * G if hook == "init" else list(range(G))      # 'init': RCCL is never entered, engines may share the GPU
    n = G * 1500 + 1
    p = ob.stable_orbits(n, 0.5, 30.0, 31)
    g = rx.NBodyGroup(devices, mode="strict")
    assert g.info()["exchange"] == "rccl" and g.info()["rccl_ranks"] == 0     # nothing created yet
    g.set_particles(p["px"], p["py"], p["vx"], p["vy"], p["m"])
    q = p.copy()
    for _ in range(3):
        g.step_brute_force(0.01); ob.step_brute_force(q, 0.01, nthreads=8)
    got = g.get_particles()
    for k in KEYS:
        assert_bit_equal(got[k], q[k], f"fallback({hook}) G={G} {k}")
    info = g.info()
    assert info["exchange"] == "peer_copy_after_rccl_failure" and info["rccl_ranks"] == 0 and "simulated" in info["note"], info
    assert g.exchanges() == 3
    g.close()


@pytest.mark.parametrize("bits,mode", [(32, "strict"), (32, "fast"), (16, "fast")])
def test_group_with_one_enqueue_thread_per_device(rx, ob, monkeypatch, bits, mode):
    """VERDICT r02 next #1c: one persistent host thread per engine enqueues that engine's K1 + K2 + its share of the
    exchange (nbx_group_set_enqueue_threads / NBX_GROUP_ENQUEUE=threads). Same results as the single enqueue thread:
    bit for bit (the kernels and their order per stream are the same), ragged slabs included."""
    monkeypatch.setenv("NBX_GROUP_EXCHANGE", "copy")
    G, n = 4, 4 * 2000 + 3
    p = ob.stable_orbits(n, 0.5, 30.0, 41)
    outs = []
    for threads in (False, True):
        g = rx.NBodyGroup([0] * G, mode=mode)
        g.set_source_precision(bits)
        g.set_enqueue_threads(threads)
        assert g.info()["enqueue_threads"] == (G if threads else 0)
        g.set_particles(p["px"], p["py"], p["vx"], p["vy"], p["m"])
        for _ in range(4):
            g.step_brute_force(0.01)
        g.step_barnes_hut(0.6, 0.01, 1)
        g.step_brute_force(0.01)
        g.synchronize()
        outs.append(g.get_particles())
        assert g.info()["exchange"] == "peer_copy"
        g.close()
    for k in KEYS:
        assert_bit_equal(outs[0][k], outs[1][k], f"enqueue threads {mode} {bits} {k}")
    if mode == "strict":
        q = p.copy()
        for _ in range(4):
            ob.step_brute_force(q, 0.01, nthreads=8)
        assert ob.step_barnes_hut(q, 0.6, 0.01, 4) == 0
        ob.step_brute_force(q, 0.01, nthreads=8)
        for k in KEYS:
            assert_bit_equal(outs[1][k], q[k], f"threads strict vs oracle {k}")


def test_group_over_rccl_with_two_or_more_gpus(rx, ob):
    """Real RCCL, G > 1 (ncclCommInitAll, in-place ncclAllGather of float4 and of half4, per-owner broadcasts for the ragged
    split): strict group == plain engine == oracle bit for bit; fast and fp16 within their tolerance classes."""
    have = rx.device_count()
    if have < 2:
        pytest.skip(f"needs >= 2 GPUs for RCCL with more than one rank ({have} here)")
    G = min(have, 8)
    devices = list(range(G))
    for n in (G * 4096, G * 1000 + 3):       # even slabs (all-gather) and a ragged last slab (broadcasts)
        p = ob.stable_orbits(n, 0.5, 30.0, 7)
        g = rx.NBodyGroup(devices, mode="strict")
        g.set_particles(p["px"], p["py"], p["vx"], p["vy"], p["m"])
        q = p.copy()
        for _ in range(3):
            g.step_brute_force(0.01); ob.step_brute_force(q, 0.01, nthreads=8)
        g.step_barnes_hut(0.7, 0.01, 1)
        assert ob.step_barnes_hut(q, 0.7, 0.01, 4) == 0
        got = g.get_particles()
        for k in KEYS:
            assert_bit_equal(got[k], q[k], f"RCCL G={G} n={n} {k}")
        g.close()
        _check_group_against_plain_engine(rx, ob, devices, n, 11)


def _run_bench(args, env_extra, timeout=900):
    env = dict(os.environ, **env_extra)
    env.pop("WORLD_SIZE", None); env.pop("RANK", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                         timeout=timeout, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout          # the ONE-JSON-line contract (RCCL banners go to stderr)
    return json.loads(lines[0])


def test_bench_gpus_n_plain_invocation_uses_the_group_host(rx):
    """`python bench.py --gpus 2` (no torch.distributed.run): the single-process group drives the run and prints one JSON
    line. Real RCCL when the box has two GPUs; otherwise the two engines share the GPU through the copy exchange
    (control flow + accounting only)."""
    extra = {} if rx.device_count() >= 2 else {"NBX_GROUP_EXCHANGE": "copy"}
    res = _run_bench(["--gpus", "2", "--n", "32768", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"], extra)
    assert res["n_gpus"] == 2 and res["config"]["host"] == "group" and res["scaling"] == "strong"
    assert len(res["per_gpu"]) == 2 and [r["slab"] for r in res["per_gpu"]] == [[0, 16384], [16384, 32768]]
    assert all(r["force_launches"] == 3 and r["exchanges"] == 3 and r["exchange_us"] > 0 for r in res["per_gpu"])
    assert res["value"] > 0 and 0 < res["roofline"]["frac"] < 1
    assert res["roofline"]["interactions_per_launch"] == 16384.0 * 32767.0


@pytest.mark.parametrize("extra_env", [{}, {"NBX_GROUP_ENQUEUE": "threads"}, {"NBX_GROUP_RCCL_FAIL": "init"}])
def test_bench_gpus_8_verifies_itself(rx, extra_env):
    """VERDICT r02 next #1 'done' line: `NBX_GROUP_EXCHANGE=copy python bench.py --gpus 8 --verify` on the 1-GPU box -- eight
    engines (sharing the GPU unless the box has eight), the timed loop, then the self-check: the group's state after more
    steps against ONE plain engine from the same state, in the JSON line. Also with one enqueue thread per device, and with a
    simulated RCCL failure (the run must survive on peer copies and say so)."""
    env = dict(extra_env)
    if rx.device_count() < 8 and "NBX_GROUP_RCCL_FAIL" not in env:
        env["NBX_GROUP_EXCHANGE"] = "copy"
    res = _run_bench(["--gpus", "8", "--n", "65536", "--steps", "3", "--warmup", "1", "--verify", "--no-cpu-baseline"], env)
    assert res["n_gpus"] == 8 and len(res["per_gpu"]) == 8
    v = res["verify"]
    assert v["ok"] and v["steps"] == 2 and v["max_dp"] <= v["tol_dp"] and v["max_dv"] <= v["tol_dv"] and v["max_displacement"] > 0, v
    if "NBX_GROUP_RCCL_FAIL" in env:
        assert res["exchange"] == "peer_copy_after_rccl_failure" and res["rccl_ranks"] == 0 and "simulated" in res["exchange_note"]
    elif rx.device_count() >= 8:
        assert res["exchange"] == "rccl" and res["rccl_ranks"] == 8
    else:
        assert res["exchange"] == "peer_copy" and res["rccl_ranks"] == 0
    assert res["enqueue_threads"] == (8 if env.get("NBX_GROUP_ENQUEUE") == "threads" else 0)
    assert res["rank_skew"]["kernel_ms_max"] >= res["rank_skew"]["kernel_ms_min"] > 0


def test_bench_verify_strict_and_barnes_hut_through_the_group(rx):
    """The same self-check in the bit-exact mode (must be bit-equal) and for the Barnes-Hut workload."""
    env = {} if rx.device_count() >= 3 else {"NBX_GROUP_EXCHANGE": "copy"}
    res = _run_bench(["--gpus", "3", "--n", "10001", "--steps", "2", "--warmup", "1", "--mode", "strict", "--verify", "--no-cpu-baseline"], env)
    assert res["verify"]["ok"] and res["verify"]["bit_equal"] and res["verify"]["max_dp"] == 0.0, res["verify"]
    res = _run_bench(["--gpus", "2", "--workload", "bh", "--n", "50000", "--theta", "0.6", "--steps", "2", "--warmup", "1", "--verify",
                      "--no-cpu-baseline", "--no-traffic"], env)
    assert res["verify"]["ok"], res["verify"]


def test_bench_under_torch_distributed_run_two_ranks(rx):
    """The driver's multi-GPU launch line: `python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr
    127.0.0.1 --master-port P bench.py --gpus 2 ...` (one rank per GPU, torch.distributed moves the slabs).  RCCL when the
    box has two GPUs; on the single-GPU test box the two ranks share the device and exchange over gloo
    (NBX_DIST_BACKEND=gloo: control flow, slab kernels side by side, the one-JSON-line contract -- not a measurement)."""
    import socket

    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    if rx.device_count() < 2:
        env["NBX_DIST_BACKEND"] = "gloo"
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--bodies", "32768", "--steps", "3", "--warmup", "1",
           "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["config"]["host"] == "torch" and res["scaling"] == "strong"
    assert [r["slab"] for r in res["per_gpu"]] == [[0, 16384], [16384, 32768]] and all(r["force_launches"] == 3 for r in res["per_gpu"])
    assert res["value"] > 0 and 0 < res["roofline"]["frac"] < 1 and "cpu_baseline" not in res
    assert res["verify"]["ok"] and res["verify"]["steps"] == 2, res["verify"]     # --full: on by default with more than one GPU


def test_bench_default_line_has_roofline_and_measured_traffic(rx):
    """N = 1 (the driver's `--full` line, at a small size): roofline + traffic measured by the in-run rocprofv3 passes when the
    profiler is installed."""
    import shutil

    res = _run_bench(["--full", "--n", "32768", "--steps", "3", "--warmup", "1", "--cpu-seconds", "0.5"], {})
    assert res["n_gpus"] == 1 and res["config"]["host"] == "single"
    rl = res["roofline"]
    assert rl["hbm_algorithmic_bytes_per_launch"] == 16.0 * 32768 * 2
    if shutil.which("rocprofv3"):
        assert rl["traffic"] is not None and rl["traffic"] >= 0.5 * rl["hbm_algorithmic_bytes_per_launch"], rl
    assert res["cpu_baseline"]["kind"] == "port"
    assert rl["flops_executed_per_interaction"] == 16 and abs(rl["frac_executed"] - rl["frac"] * 16 / 17) < 1e-12
    gm = res["general_masses"]
    assert gm["launch"]["variant"] == 6 and 0 < gm["frac"] < 1 and gm["value"] > 0
    ss = res["steady_state"]
    assert ss["window_s"] >= 3.0 and ss["ms_per_step"] > 0


def test_bench_barnes_hut_workload(rx):
    res = _run_bench(["--full", "--workload", "bh", "--n", "100000", "--steps", "3", "--warmup", "1"], {})
    assert res["unit"] == "body-steps/s" and res["value"] > 0
    assert res["ms_split"]["tree_nodes"] > 100000 and res["ms_split"]["bh_eval_kernel"] > 0
    assert res["cpu_baseline"]["rc"] == 0
    # the traversal kernel's HBM bytes are measured in the same run (rocprofv3 PMC child passes) when rocprofv3 is there:
    # at most one copy of the node array per XCD plus the bodies and the scattered result lines
    t = res["roofline"]["traffic"]
    if t is not None:
        alg = res["roofline"]["hbm_algorithmic_bytes_per_launch"]
        assert 0.0 < t <= 12.0 * alg, (t, alg)
        # ... and so is its VALU issue (round 3: counters of this run instead of a modelled constant); round 4: `frac` is work
        # over time over peak -- 12 flops per pair law + 7 per opening test, counted by a counting traversal -- and the VALU-busy
        # share is a field of its own
        rl = res["roofline"]
        ic = rl["issue_counters"]
        assert ic is not None and 0.0 < ic["valu_busy_frac"] < 1.0 and rl["valu_busy_frac"] == ic["valu_busy_frac"]
        assert 5.0 < ic["valu_insts_per_wave_turn"] < 60.0 and 5.0 < ic["salu_insts_per_wave_turn"] < 60.0, ic
    rl = res["roofline"]
    flops = 12.0 * rl["pair_evals_per_body"] * 100000 + 7.0 * rl["opening_tests_per_body"] * 100000
    assert abs(rl["flops_per_launch"] - flops) <= 1e-6 * flops
    assert rl["unit"] == "TFLOP/s" and abs(rl["achieved"] - flops / (rl["kernel_avg_ms"] * 1e-3) / 1e12) <= 1e-9 * rl["achieved"]
    assert abs(rl["frac"] - rl["achieved"] / rl["peak"]) < 1e-12 and 0.0 < rl["frac"] < 0.5
    assert res["config"]["walk"].startswith("child groups")


def test_bench_plain_run_is_lean_and_dumps_the_state_of_its_last_timed_step(rx, tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` does what its headline figure needs and nothing that takes a run of its
    own (those sit behind --full); `--dump-outputs DIR` writes the state the last timed step left, one float32 .npy per array.
    The kernels of the fast all-pairs step use no atomics, so a plain engine stepped W + K times from the same seeded state
    must give the same bits."""
    n, k, w = 4099, 3, 2                                                     # odd size: not a multiple of any tile
    res = _run_bench(["--gpus", "1", "--n", str(n), "--steps", str(k), "--warmup", str(w), "--dump-outputs", str(tmp_path / "out")], {})
    for key in ("cpu_baseline", "steady_state", "general_masses", "companions", "verify"):
        assert key not in res, key
    assert res["roofline"]["traffic"] is None and res["roofline"]["kernel_launches"] == k
    assert res["steps"] == k and res["warmup"] == w and res["unit"] == "interactions/s" and res["higher_is_better"] is True
    assert res["ms_per_step"] > 0 and abs(res["value"] - n * (n - 1.0) / (res["ms_per_step"] * 1e-3)) <= 1e-9 * res["value"]
    g = rx.NBodyEngine()
    g.plummer_sphere(n, dim=3)
    st = g.get_particles()
    g.close()
    e = rx.NBodyEngine(mode="fast")
    e.set_particles(st["px"], st["py"], st["vx"], st["vy"], st["m"], st["pz"], st["vz"])
    for _ in range(w + k):
        e.step_brute_force(0.01)
    want = e.get_particles()
    e.close()
    assert sorted(os.listdir(tmp_path / "out")) == sorted(key + ".npy" for key in want)
    for key in want:
        got = np.load(tmp_path / "out" / (key + ".npy"))
        assert got.dtype == np.float32 and got.shape == (n,)
        assert_bit_equal(got, want[key], key)
    assert np.abs(want["vx"]).max() > 0


LEVEL1 = r"""
import os, sys, json, zlib
sys.path.insert(0, os.environ["NBX_ROOT"])
import numpy as np
import rust_exp_amd as rx
rx.nb_stable_orbits(6000, 0.5, 30.0)
frames = []
for k in range(4):
    rx.nb_step_barnes_hut(0.85, 0.01, 1)
    frames.append(zlib.crc32(rx.nb_draw(256, 256).tobytes()))
rx.nb_step_barnes_hut(0.0, 0.01, 1)            # theta == 0 delegates to brute force (nbody.rs:197-200)
rx.nb_step_brute_force(0.01)
frames.append(zlib.crc32(rx.nb_draw(256, 256).tobytes()))
rx.nb_random_disk(3001)                        # ragged slabs
rx.nb_step_barnes_hut(0.5, 0.01, 4)
frames.append(zlib.crc32(rx.nb_draw(128, 96).tobytes()))
print("RESULT " + json.dumps({"n": rx.nb_num_particles(), "frames": frames}))
"""


def test_six_level1_symbols_through_the_group(rx):
    """NB_GPUS: the unmodified caller's six nb_* symbols served by the single-process group.  Bit-exact mode, same seed: every
    frame nb_draw produces must equal the single-engine run's, pixel for pixel (CRC of the framebuffer), through Barnes-Hut steps,
    the theta == 0 delegation, brute-force steps, a preset change to a ragged body count.  Two / three engines share the one test
    GPU through the copy exchange (real RCCL when the box has that many GPUs)."""
    outs = {}
    for gpus in ("1", "2", "3"):
        env = dict(os.environ, NBX_ROOT=ROOT, NB_SEED="77", NB_FORCE_MODE="strict", NB_GPUS=gpus)
        if rx.device_count() < int(gpus):
            env["NBX_GROUP_EXCHANGE"] = "copy"
        r = subprocess.run([sys.executable, "-c", LEVEL1], env=env, capture_output=True, text=True, timeout=600)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        assert r.returncode == 0 and lines, r.stdout[-1000:] + r.stderr[-3000:]
        outs[gpus] = json.loads(lines[-1][7:])
    assert outs["1"]["n"] == 3001 and len(set(outs["1"]["frames"])) == len(outs["1"]["frames"])   # the scene really changes
    assert outs["2"] == outs["1"] and outs["3"] == outs["1"]


LEVEL1_FP16 = r"""
import os, sys, json
sys.path.insert(0, os.environ["NBX_ROOT"])
import numpy as np
import rust_exp_amd as rx
rx.nb_stable_orbits(8192, 0.5, 30.0)
for k in range(5):
    rx.nb_step_brute_force(0.01)
fb = rx.nb_draw(256, 256)
np.save(os.environ["NBX_OUT"], fb)
print("RESULT ok")
"""


def test_level1_fp16_sources_through_the_group(rx, tmp_path):
    """BASELINE config #5 as the unmodified caller would run it: NB_GPUS=<n> NB_SOURCE_BITS=16 (fast mode). Five brute-force steps
    with bodies moving 0.3 per step: with the round-1 bug (stale half4 copies of the other slabs) the frames of 1 and 2 engines
    would have nothing in common; with the half4 all-gather they differ by a few boundary pixels at most (different launch
    shapes round differently)."""
    fbs = {}
    for gpus in ("1", "2"):
        out = str(tmp_path / f"fb{gpus}.npy")
        env = dict(os.environ, NBX_ROOT=ROOT, NB_SEED="78", NB_GPUS=gpus, NB_SOURCE_BITS="16", NBX_OUT=out)
        if rx.device_count() < int(gpus):
            env["NBX_GROUP_EXCHANGE"] = "copy"
        r = subprocess.run([sys.executable, "-c", LEVEL1_FP16], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "RESULT ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
        fbs[gpus] = np.load(out)
    lit = int((fbs["1"] != 0).sum())
    assert lit > 3000 and int((fbs["1"] != fbs["2"]).sum()) <= max(20, lit // 200), (lit, int((fbs["1"] != fbs["2"]).sum()))
