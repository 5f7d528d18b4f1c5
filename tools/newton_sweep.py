"""The measurements of docs/rounds/r12.md (K11, k_newton64), one JSON line per figure.
  python tools/newton_sweep.py sweep   262 144-body sphere, unequal then equal masses: law 0 and law 1 alternating on one engine,
                                       two passes, kernel time per sweep from NBX_OPT_PROFILE
  python tools/newton_sweep.py fp64    forces_f64 without / with the potential at 1 048 576 bodies under both laws (host clock)
NBX_SO=path loads another build of the library (the UNROLL A/B: make ... HIPCC="hipcc -DNBX_NEWTON_UNROLL=4" into a directory of its
own, then this script once per library)."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rust_exp_amd as rx
import rust_exp_amd.engine as eng
if os.environ.get("NBX_SO"):
    eng._SO = os.environ["NBX_SO"]
    eng.build = lambda force=False: eng._SO

def state(n, equal):
    st = rx.plummer_sphere(n)
    if not equal:
        st["m"] = np.random.default_rng(11).uniform(0.5, 2.0, n).astype(np.float32)
    return st

def engine(st):
    e = rx.NBodyEngine()
    e.set_particles(st["px"], st["py"], st["vx"], st["vy"], st["m"], pz=st["pz"], vz=st["vz"])
    return e

def sweep():
    n, reps = 262144, 5
    for equal in (False, True):
        e = engine(state(n, equal))
        e.profile(True)
        for law in ("reference", "newton"):
            e.set_law(law); e.forces(0.0)          # warm
        for p in (1, 2):
            for law in ("reference", "newton"):
                e.set_law(law)
                e.profile_reset()
                for _ in range(reps):
                    e.forces(0.0)
                ms, cnt = e.profile_read(rx.NBX_K_FORCE)
                ll = e.last_launch()
                print(json.dumps({"what": "sweep", "so": os.environ.get("NBX_SO", "default"), "n": n, "equal_masses": equal, "pass": p, "law": law,
                                  "variant": ll["variant"], "jsplit": ll["jsplit"], "ms_per_sweep": ms / cnt, "launches": cnt,
                                  "interactions_per_s": n * n / (ms / cnt * 1e-3)}), flush=True)

def fp64():
    n = 1048576
    e = engine(state(n, False))
    e.set_law("newton"); e.forces_f64(potential=False)   # warm: allocations
    for law in ("reference", "newton"):
        e.set_law(law)
        for pot in (False, True):
            t0 = time.perf_counter(); e.forces_f64(potential=pot); dt = time.perf_counter() - t0
            print(json.dumps({"what": "fp64", "n": n, "law": law, "potential": pot, "seconds": dt, "variant": e.last_launch()["variant"]}), flush=True)

{"sweep": sweep, "fp64": fp64}[sys.argv[1]]()
