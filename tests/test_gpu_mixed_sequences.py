"""Mixed call sequences on ONE long-lived engine: the octree path, the Newtonian law, the fp64 diagnostics and the Hermite family next
to the planar Barnes-Hut and all-pairs steps.  Every other test file builds a fresh engine per call kind; the engine carries state
between calls (engine_internal.h: the kept (a0, j0) and the block levels, the order-sorted copy of the positions and the warm sort's
order, two speculative Barnes-Hut steps in flight, the common mass and its exceptions, any_z, thirty buffers that only grow), and
this file is about that state.

A sequence cannot be followed in float64 (it is chaotic and the bounds compound), so the file rests on three properties, the first
two BIT FOR BIT -- legitimate because every path involved is deterministic, which test_every_operation_is_deterministic checks first:

  replay        after any prefix, get_particles() plus the options in force define a fresh engine; every operation that starts from
                the state alone gives on the long-lived engine what it gives on the fresh one.  The Hermite family is the exception
                by design: after a Hermite step (or acc_jerk) it continues from the kept pair; after anything that moved or replaced
                bodies it restarts, and the restart equals the fresh engine's first step (which test_gpu_hermite.py pins to float64).
  transparency  between two steps of one integrator, calls that return data and change no particle, and refused calls, change
                nothing: the final state equals the uninterrupted run's.  PROBES below is the table: "transparent", or "restarts"
                (the Hermite family's continuation then equals the fresh engine's; every other step kind is still untouched).
  anchor        at the end of every sequence forces_f64() of the final state lies within test_gpu_diag64.py's bound
                (n + 16) 2^-53 sum|term| -- test_gpu_newton.py's (n + 20) 2^-53 sum|term| under the Newtonian law -- of the float64 pair
                terms over get_particles(), summed with math.fsum.

The device-built quadtree (set_bh_tree("device"), bh_flat_dump("device")) and the device draw are asked for from 321 bodies on only
(below that size those probes take the host forms)."""
import functools
import math

import numpy as np
import pytest

from test_gpu_bh_oct import _with, system
from test_gpu_hermite import _sphere

pytestmark = pytest.mark.gpu

KEYS = ("px", "py", "pz", "vx", "vy", "vz", "m")
EPS = float(np.float32(0.0001))
DT = 0.01
NBX_OPT_BH_ASYNC = 15
NBX_STAT_BH_LAST_TREE = 1
DEFAULTS = {"law": "reference", "bh_dim": 2, "quad": True, "tree": "auto", "bh_async": 1, "train": 0, "eta": 0.02}
SMALL_DEVICE = 321  # the device quadtree and the device draw are asked for from this many bodies on


# ---- engines, states, results -----------------------------------------------------------------------------------------------------
def _set(e, st):
    e.set_particles(st["px"], st["py"], st["vx"], st["vy"], st["m"], st["pz"], st["vz"])


def _fresh(rx, st, o):
    e = rx.NBodyEngine()
    e.set_bh_dim(o["bh_dim"])
    e.set_bh_tree(o["tree"])
    e.set_option(NBX_OPT_BH_ASYNC, o["bh_async"])
    e.set_hermite_block_train(o["train"])
    e.set_bh_quadrupole(o["quad"])
    _set(e, st)
    e.set_law(o["law"])
    return e


def _enc(x):
    if x is None:
        return b""
    if isinstance(x, np.ndarray):
        return x.tobytes()
    if isinstance(x, dict):
        return b"|".join(_enc(v) for v in x.values())
    if isinstance(x, (tuple, list)):
        return b"|".join(_enc(v) for v in x)
    return repr(x).encode()


def _call(rx, fn, e, o):
    """("ok", bytes of what the call returned) or ("err", status): a refused call is a result like any other"""
    try:
        return "ok", _enc(fn(e, o))
    except rx.NBodyError as err:
        return "err", err.code


def _bytes(e):
    return _enc(e.get_particles())


def _copy(st):
    return {k: np.array(st[k], np.float32) for k in KEYS}


def _flip(a, b, x):
    return b if x == a else a


# ---- the operations ----------------------------------------------------------------------------------------------------------------
# movers: fn(e, o); which tree, dimension and law serve "bh" is the options' business (an option the law refuses keeps the call in
# the sequence as a refused call)
MOVERS = {
    "step_brute_force": lambda e, o: e.step_brute_force(DT),
    "step_local": lambda e, o: e.step_local(DT),
    "step_barnes_hut(0.5)": lambda e, o: e.step_barnes_hut(0.5, DT),
    "step_barnes_hut(0.85)": lambda e, o: e.step_barnes_hut(0.85, DT),
    "step_hermite": lambda e, o: e.step_hermite(DT),
    "step_hermite_block": lambda e, o: e.step_hermite_block(DT, o["eta"]),
}
HERMITE_MOVERS = ("step_hermite", "step_hermite_block")


def _idx(e, count):
    n = e.num_particles()
    return np.random.default_rng(count).permutation(n)[:min(count, n)].astype(np.int32)


def _with_dim(dim, theta):
    def fn(e, o):
        e.set_bh_dim(dim)
        try:
            return e.forces(theta)
        finally:
            e.set_bh_dim(o["bh_dim"])
    return fn


def _draw_device(e, o):
    if e.num_particles() < SMALL_DEVICE:
        return e.draw(64, 48)
    e.set_draw_device(True)
    try:
        return e.draw(64, 48)
    finally:
        e.set_draw_device(None)


def _draw_host(e, o):
    e.set_draw_device(False)
    try:
        return e.draw(64, 48)
    finally:
        e.set_draw_device(None)


def _profile(e, o):
    e.profile(True)
    e.profile(False)


def _save(e, o, load=False):
    import os
    import tempfile

    fd, path = tempfile.mkstemp(suffix=".nbx")
    os.close(fd)
    try:
        e.save(path)
        if load:
            e.load(path)
    finally:
        os.unlink(path)


def _law_flip(call=None):
    """the other law and back, with `call` (refused there) in between"""
    def fn(e, o):
        e.set_law(_flip("reference", "newton", o["law"]))
        try:
            return call(e, o) if call else None
        finally:
            e.set_law(o["law"])
    return fn


def _under_newton(call):
    def fn(e, o):
        e.set_law("newton")
        try:
            return call(e, o)
        finally:
            e.set_law(o["law"])
    return fn


def _planar_bh_under_newton(e, o):
    e.set_law("newton")
    e.set_bh_dim(2)
    try:
        return e.step_barnes_hut(0.5, DT)
    finally:
        e.set_bh_dim(o["bh_dim"])
        e.set_law(o["law"])


def _octree_in(how):
    def fn(e, o):
        e.set_bh_dim(3)
        e.set_mode("strict") if how == "strict" else e.set_source_precision(16)
        try:
            return e.step_barnes_hut(0.5, DT) if how == "strict" else e.forces(0.5)
        finally:
            e.set_mode("fast") if how == "strict" else e.set_source_precision(32)
            e.set_bh_dim(o["bh_dim"])
    return fn


def _dim_flip(e, o):
    e.set_bh_dim(_flip(2, 3, o["bh_dim"]))
    e.set_bh_dim(o["bh_dim"])


def _quad_flip(e, o):
    e.set_bh_quadrupole(not o["quad"])
    e.set_bh_quadrupole(o["quad"])


def _flat_device(e, o):
    return e.bh_flat_dump("device" if e.num_particles() >= SMALL_DEVICE else False)


# The table.  name: (fn, what it does to a running Hermite integration, is its result a function of state + options alone,
#                    must the call be refused whatever the options).
# "transparent": the next Hermite step continues from the kept pair as if the call had not been made.  "restarts": the kept pair is
# gone or replaced by that of the current state: the next Hermite step equals a fresh engine's first step from get_particles().
# Taken from the documented behaviour: include/nbody_mi355x.h on nbx_step_hermite ("anything else that can change positions,
# velocities or masses ... a change of NBX_OPT_DIM"), nbx_acc_jerk ("leaves the evaluated pair as the kept"), NBX_OPT_LAW (c_api.cpp:
# a kept pair belongs to the other law); every call that returns data and changes no particle is transparent.  No step kind other
# than the Hermite family may notice either class.
T, R = "transparent", "restarts"
PROBES = {
    "forces(0.0)": (lambda e, o: e.forces(0.0), T, True, False),
    "forces(0.5) planar": (_with_dim(2, 0.5), T, True, False),
    "forces(0.5) octree": (_with_dim(3, 0.5), T, True, False),
    "forces_f64": (lambda e, o: e.forces_f64(), T, True, False),
    "conserved": (lambda e, o: e.conserved(), T, True, False),
    "acc_jerk_f64()": (lambda e, o: e.acc_jerk_f64(), T, True, False),
    "acc_jerk_f64(idx)": (lambda e, o: e.acc_jerk_f64(_idx(e, 5)), T, True, False),
    "acc_jerk_subset(1)": (lambda e, o: e.acc_jerk_subset(_idx(e, 1)), T, True, False),
    "acc_jerk_subset(64)": (lambda e, o: e.acc_jerk_subset(_idx(e, 64)), T, True, False),
    "acc_jerk_subset(65)": (lambda e, o: e.acc_jerk_subset(_idx(e, 65)), T, True, False),
    "bh_oct_dump": (lambda e, o: e.bh_oct_dump(), T, True, False),
    "bh_oct_moments": (lambda e, o: e.bh_oct_moments(), T, True, False),
    "bh_flat_dump host": (lambda e, o: e.bh_flat_dump(), T, True, False),
    "bh_flat_dump device": (_flat_device, T, True, False),
    "draw host": (_draw_host, T, True, False),
    "draw device": (_draw_device, T, True, False),
    "get_particles": (lambda e, o: e.get_particles(), T, True, False),
    "save": (_save, T, True, False),
    "hermite_kept": (lambda e, o: e.hermite_kept(), T, False, False),
    "hermite_block_levels": (lambda e, o: e.hermite_block_levels(), T, False, False),
    "hermite_timestep": (lambda e, o: e.hermite_timestep(0.02), T, False, False),
    "last_launch": (lambda e, o: e.last_launch(), T, False, False),
    "profile on/off": (_profile, T, False, False),
    "synchronize": (lambda e, o: e.synchronize(), T, True, False),
    "set_bh_dim there and back": (_dim_flip, T, True, False),
    "set_bh_quadrupole there and back": (_quad_flip, T, True, False),
    "refused: octree step, strict mode": (_octree_in("strict"), T, True, True),
    "refused: octree forces, fp16 sources": (_octree_in("fp16"), T, True, True),
    "acc_jerk": (lambda e, o: e.acc_jerk(), R, True, False),
    "set_law there and back": (_law_flip(), R, True, False),
    "set_launch(dim=0)": (lambda e, o: e.set_launch(dim=0), R, True, False),
    "save + load": (functools.partial(_save, load=True), R, True, False),
    "refused: step_hermite under law 1": (_under_newton(lambda e, o: e.step_hermite(DT)), R, True, True),
    "refused: step_hermite_block under law 1": (_under_newton(lambda e, o: e.step_hermite_block(DT, 0.02)), R, True, True),
    "refused: acc_jerk under law 1": (_under_newton(lambda e, o: e.acc_jerk()), R, True, True),
    "refused: planar step_barnes_hut(0.5) under law 1": (_planar_bh_under_newton, R, True, True),
}
HERMITE_PROBES = ("hermite_kept", "hermite_block_levels", "hermite_timestep")   # read the kept pair: state-only when there is none
MAKES_KEPT = ("acc_jerk", "hermite_timestep")                                   # leave a valid kept pair behind (law 0)


# ---- the float64 anchor ---------------------------------------------------------------------------------------------------------
def _anchor(e, o, what):
    st = e.get_particles()
    n = len(st["m"])
    P = np.stack([st[k] for k in KEYS[:3]], 1).astype(np.float64)
    m = st["m"].astype(np.float64)
    got = e.forces_f64(potential=False)[:3]
    K = 20 if o["law"] == "newton" else 16
    worst = 0.0
    for i in range(n):
        d = P - P[i]
        s = (d * d).sum(1) + EPS
        w = m[i] * m * (1.0 / np.sqrt(s)) ** 3 if o["law"] == "newton" else m[i] * (m / s)
        terms = w[:, None] * d
        for k in range(3):
            bound = (n + K) * 2.0 ** -53 * np.abs(terms[:, k]).sum()
            err = abs(got[k][i] - math.fsum(terms[:, k]))
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
    print(f"anchor {what}: n = {n}, law = {o['law']}, worst error / bound = {worst:.3f}")
    assert worst <= 1.0, (what, worst)


# ---- the sequence runner: replay after every operation -----------------------------------------------------------------------------
class Sequence:
    """One long-lived engine, the options in force, a model of "is there a kept pair a Hermite step would continue from" (the table
    above), and the replay check: before every operation a fresh engine is made from the last get_particles(); operation and
    resulting state must agree in bytes unless the operation is of the Hermite family and continues."""

    def __init__(self, rx, st, **opts):
        self.rx, self.o = rx, dict(DEFAULTS, **opts)
        self.e = _fresh(rx, st, self.o)
        self.snap, self.live, self.log = _bytes(self.e), False, []

    def option(self, key, value):
        self.log.append(f"option {key} = {value}")
        if key == "law" and self.o[key] != value:
            self.live = False            # (c_api.cpp: a kept pair belongs to the other law; the same law again changes nothing)
        self.o[key] = value
        e = self.e
        {"law": e.set_law, "bh_dim": e.set_bh_dim, "quad": e.set_bh_quadrupole, "tree": e.set_bh_tree,
         "bh_async": lambda v: e.set_option(NBX_OPT_BH_ASYNC, v), "train": e.set_hermite_block_train, "eta": lambda v: None}[key](value)

    def replace(self, st, how="set_particles"):
        self.log.append(f"{how} n = {len(st['m'])}")
        if how == "load":
            import os
            import tempfile

            other = _fresh(self.rx, st, self.o)
            fd, path = tempfile.mkstemp(suffix=".nbx")
            os.close(fd)
            try:
                other.save(path)
                self.e.load(path)
            finally:
                os.unlink(path)
        else:
            _set(self.e, st)
        self.live = False
        self.snap = _bytes(self.e)
        assert self.snap == _enc(_copy(st)), self._say("the replaced state reads back")

    def _say(self, what):
        return what + "\n  options: %r\n  sequence:\n    " % (self.o,) + "\n    ".join(self.log)

    def do(self, name):
        rx, o = self.rx, self.o
        self.log.append(name)
        fn, klass, state_only, refused = PROBES[name] if name in PROBES else (MOVERS[name], None, True, False)
        hermite = name in HERMITE_MOVERS or name in HERMITE_PROBES
        f = _fresh(rx, self.e.get_particles(), o)
        want, got = _call(rx, fn, f, o), _call(rx, fn, self.e, o)
        after, after_f = _bytes(self.e), _bytes(f)
        ok = got[0] == "ok"
        if refused:
            assert got[0] == "err" and got[1] == rx.NBX_ERR_STATE, self._say(f"{name} was not refused: {got[:1]}")
        if name in PROBES or not ok:
            assert after == self.snap, self._say(f"{name} ({got[0]}) changed the particles")
        if (state_only or name in HERMITE_PROBES) and not (hermite and self.live):
            assert got == want, self._say(f"{name}: the long-lived engine's result is not the fresh engine's")
            assert after == after_f, self._say(f"{name}: the state after it is not the fresh engine's")
        # the model of the kept pair
        if name in MOVERS and ok:
            self.live = name in HERMITE_MOVERS
        elif name in PROBES and klass == R:
            self.live = name == "acc_jerk" and ok
        elif name in MAKES_KEPT and ok:
            self.live = True
        self.snap = after
        return got

    def finish(self, what):
        _anchor(self.e, self.o, what)


# ---- 1. determinism ---------------------------------------------------------------------------------------------------------------
DET_CONFIGS = {   # every way a mover is served: (options, size)
    "planar host tree": (dict(tree="host"), 321),
    "planar device tree, async": (dict(tree="device"), 1100),
    "planar device tree, waited for": (dict(tree="device", bh_async=0), 1100),
    "octree law 0": (dict(bh_dim=3), 1100),
    "octree law 1 quadrupole": (dict(bh_dim=3, law="newton"), 1100),
    "octree law 1 monopole": (dict(bh_dim=3, law="newton", quad=False), 1100),
    "block train 4": (dict(train=4), 321),
}


def _twice(rx, st, o, fn, steps=1):
    out = []
    for _ in range(2):
        e = _fresh(rx, st, o)
        res = [_call(rx, fn, e, o) for _ in range(steps)]
        out.append((res, _bytes(e)))
    return out[0] == out[1], out[0][0][-1][0]


@pytest.mark.parametrize("name", list(MOVERS) + list(PROBES))
def test_every_operation_is_deterministic(rx, name):
    """Two fresh engines, the same input, the same bytes -- the licence for everything below.  Movers run three times in a row (the
    second and third Barnes-Hut step find steps in flight and a warm order) under every configuration that serves them."""
    st = _sphere(rx, 1100, 6)
    fn = PROBES[name][0] if name in PROBES else MOVERS[name]
    configs = {"defaults": ({}, 1100), "law 1": (dict(law="newton"), 1100)}
    if name.startswith("step_barnes_hut"):
        configs = {k: v for k, v in DET_CONFIGS.items() if k != "block train 4"}
    if name == "step_hermite_block":
        configs["block train 4"] = DET_CONFIGS["block train 4"]
    if name in PROBES:
        configs["octree law 1"] = (dict(bh_dim=3, law="newton"), 1100)
    bad = []
    for label, (opts, n) in configs.items():
        o = dict(DEFAULTS, **opts)
        same, status = _twice(rx, st if n == 1100 else _sphere(rx, n, 6), o, fn, steps=3 if name in MOVERS else 1)
        print(f"deterministic: {name} [{label}] -> {status}, same bytes: {same}")
        if not same:
            bad.append(label)
    assert not bad, (name, bad)


# ---- 2. transparency ----------------------------------------------------------------------------------------------------------------
KINDS = {   # step kind: (mover, options, bodies)
    "step_hermite": ("step_hermite", {}, 321),
    "step_hermite_block": ("step_hermite_block", {}, 321),
    "step_hermite_block train 4": ("step_hermite_block", dict(train=4), 321),
    "planar device tree": ("step_barnes_hut(0.5)", {}, 1100),
    "octree law 0": ("step_barnes_hut(0.5)", dict(bh_dim=3), 321),
    "octree law 1": ("step_barnes_hut(0.5)", dict(bh_dim=3, law="newton"), 321),
    "brute force law 0": ("step_brute_force", {}, 321),
    "brute force law 1": ("step_brute_force", dict(law="newton"), 321),
}


@pytest.mark.parametrize("kind", list(KINDS))
def test_probes_and_refused_calls_between_two_steps_change_nothing(rx, kind):
    """step, probe, step == step, step for every probe of the table -- or, for the Hermite family behind a probe that "restarts",
    == step, then a fresh engine's step from get_particles() (acc_jerk keeps the levels of a block run: the fresh engine is given
    them).  A probe must also leave the particles as they are and be refused where the table says so."""
    mover, opts, n = KINDS[kind]
    o, st, step = dict(DEFAULTS, **opts), _sphere(rx, n, 11), MOVERS[mover]
    hermite = mover in HERMITE_MOVERS

    def first():
        e = _fresh(rx, st, o)
        assert _call(rx, step, e, o)[0] == "ok"
        return e

    levels = first().hermite_block_levels() if mover == "step_hermite_block" else None
    e = first()
    mid = e.get_particles()
    assert _call(rx, step, e, o)[0] == "ok"
    uninterrupted = _bytes(e)
    restarted = {}
    if hermite:
        for keep in (False, True) if levels is not None else (False,):
            f = _fresh(rx, mid, o)
            if keep:
                f.set_hermite_block_levels(levels)
            assert _call(rx, step, f, o)[0] == "ok"
            restarted[keep] = _bytes(f)
        assert restarted[False] != uninterrupted, "a restart must be visible for this test to mean anything"
    bad = []
    for name, (fn, klass, _, refused) in PROBES.items():
        e = first()
        # (nothing reads the state before the probe: a planar step is still in flight under it)
        got = _call(rx, fn, e, o)
        if refused and got != ("err", rx.NBX_ERR_STATE):
            bad.append(f"{name}: not refused ({got[0]})")
        if _bytes(e) != _enc(mid):
            bad.append(f"{name}: changed the particles")
        assert _call(rx, step, e, o)[0] == "ok", name
        want = restarted[name == "acc_jerk" and levels is not None] if hermite and klass == R else uninterrupted
        if _bytes(e) != want:
            bad.append(f"{name}: table says {klass if hermite else T}; continued as uninterrupted: {_bytes(e) == uninterrupted}")
    print(f"{kind}: {len(PROBES)} probes, {len(bad)} off the table")
    assert not bad, "\n".join([kind] + bad)


@pytest.mark.parametrize("n,tree", [(321, "auto"), (1100, "auto"), (321, "device")])
def test_a_tree_probe_between_hermite_steps_does_not_depend_on_which_tree_served(rx, n, tree):
    """forces(0.5) / the device tree's dump between Hermite and block steps: the host tree serves 321 bodies, the device tree 1100
    (and 321 on request).  A build that moves nothing leaves the kept pair and the levels alone at every size."""
    o, st = dict(DEFAULTS, tree=tree), _sphere(rx, n, 12)

    def run(probe):
        e = _fresh(rx, st, o)
        out = []
        for step in (lambda: e.step_hermite(DT), lambda: e.step_hermite_block(DT, 0.02), lambda: e.step_hermite_block(DT, 0.02)):
            step()
            if probe:
                kept = _enc(e.hermite_kept())
                e.forces(0.5)
                e.bh_flat_dump("device")
                assert e.get_stat(NBX_STAT_BH_LAST_TREE) == (0 if (n, tree) == (321, "auto") else 1)
                assert _enc(e.hermite_kept()) == kept
            out.append(_bytes(e))
        return out + [_enc(e.hermite_block_levels())]

    assert run(True) == run(False)


# ---- 3. hand-written sequences, one per suspicion -------------------------------------------------------------------------------
def test_prescribed_levels_do_not_survive_new_particles_of_the_same_count(rx):
    """set_hermite_block_levels -> set_particles (same n) -> acc_jerk -> step_hermite_block: the levels belonged to the old bodies;
    the block step makes its own from eta, as on a fresh engine."""
    st, other = _sphere(rx, 321, 13), _sphere(rx, 321, 14)
    s = Sequence(rx, st)
    s.e.set_hermite_block_levels(np.arange(321) % 4)
    s.log.append("set_hermite_block_levels(0 .. 3)")
    s.replace(other)
    assert s.do("acc_jerk")[0] == "ok"
    s.live = False                       # (the pair acc_jerk left is the fresh engine's own first evaluation: replay holds)
    assert s.do("step_hermite_block")[0] == "ok"
    f = _fresh(rx, other, s.o)
    f.step_hermite_block(DT, 0.02)
    assert _enc(s.e.hermite_block_levels()) == _enc(f.hermite_block_levels())
    s.finish("levels")


@pytest.mark.parametrize("mover", ["step_brute_force", "step_hermite"])
def test_a_planar_step_after_many_other_steps_sorts_from_a_stale_order(rx, mover):
    """16 640 bodies (the smallest family that takes the warm sort): one planar device-tree step leaves its order, then 40 all-pairs
    or Hermite steps of dt = 0.02 move the bodies (printed: the rms displacement against the root box), then the planar step again:
    its warm sort starts from an order 40 steps old; the fresh engine sorts cold.  Same bytes."""
    n = 16640
    st = rx.plummer_sphere(n, dim=2)
    rng = np.random.default_rng(15)
    st["vx"], st["vy"] = (rng.normal(0, 3, n).astype(np.float32) for _ in range(2))
    o = dict(DEFAULTS)
    e = _fresh(rx, st, o)
    e.step_barnes_hut(0.5, DT)
    e.step_barnes_hut(0.5, DT)
    p0 = e.get_particles()
    for _ in range(40):
        e.step_brute_force(0.02) if mover == "step_brute_force" else e.step_hermite(0.02)
    p1 = e.get_particles()
    box = max(np.ptp(p0["px"]), np.ptp(p0["py"]))
    moved = float(np.sqrt(np.mean((p1["px"] - p0["px"]) ** 2 + (p1["py"] - p0["py"]) ** 2)))
    print(f"{mover}: rms displacement {moved:.3g} = {moved / box:.3g} of the root box ({box:.3g})")
    assert moved > 0.02 * box   # (leaf cells at this size are a thousandth of the box)
    f = _fresh(rx, p1, o)
    for eng in (e, f):
        eng.step_barnes_hut(0.5, DT)
        eng.step_barnes_hut(0.5, DT)
    assert e.get_stat(NBX_STAT_BH_LAST_TREE) == 1 and f.get_stat(NBX_STAT_BH_LAST_TREE) == 1
    assert _bytes(e) == _bytes(f)


@pytest.mark.parametrize("then", ["octree step", "octree step law 1", "step_hermite", "forces_f64", "acc_jerk_f64", "conserved"])
def test_two_planar_steps_in_flight_then_at_once_another_path(rx, then):
    """Each of these entry points has to settle the speculative steps on its own path (resolve_pending)."""
    st = system("s2051")
    o = dict(DEFAULTS)
    twin = _fresh(rx, st, o)
    twin.step_barnes_hut(0.5, DT)
    twin.step_barnes_hut(0.5, DT)
    settled = twin.get_particles()
    e = _fresh(rx, st, o)
    e.step_barnes_hut(0.5, DT)
    e.step_barnes_hut(0.5, DT)            # two steps in flight; nothing has read a verdict or the state
    if then.startswith("octree"):
        o = dict(o, bh_dim=3, law="newton" if then.endswith("1") else "reference")
        e.set_bh_dim(3)                   # (an option that shapes a step settles them itself: the law flip as well)
        e.set_law(o["law"])
        fn = MOVERS["step_barnes_hut(0.5)"]
    else:
        fn = {"step_hermite": MOVERS["step_hermite"], "forces_f64": PROBES["forces_f64"][0], "acc_jerk_f64": PROBES["acc_jerk_f64()"][0],
              "conserved": PROBES["conserved"][0]}[then]
    f = _fresh(rx, settled, o)
    assert _call(rx, fn, e, o) == _call(rx, fn, f, o)
    assert _bytes(e) == _bytes(f)
    _anchor(e, o, then)


SHRINK = [2051, 65, 1, 63, 2051]


def test_every_newer_entry_point_at_a_small_size_after_a_larger_one(rx):
    """2051 -> 65 -> 1 -> 63 -> 2051 bodies on one engine: the buffers keep the larger size's records behind [n, n_pad) and behind the
    octree's groups, quadrupole records and moments.  At each size every entry point of the octree path, the fp64 sweeps and the
    Hermite family gives the fresh engine's bytes."""
    s = Sequence(rx, _sphere(rx, SHRINK[0], 20), bh_dim=3)
    for k, n in enumerate(SHRINK):
        if k:
            s.replace(_sphere(rx, n, 20 + k))
        for law, quad in (("reference", True), ("newton", True), ("newton", False)):
            s.option("law", law)
            s.option("quad", quad)
            for name in ("forces(0.5) octree", "bh_oct_moments", "bh_oct_dump", "forces_f64", "conserved", "acc_jerk_f64()", "acc_jerk_f64(idx)"):
                assert s.do(name)[0] == "ok", s._say(name)
            assert s.do("step_barnes_hut(0.5)")[0] == "ok"
        s.option("law", "reference")
        for name in ("acc_jerk_subset(65)", "acc_jerk", "step_hermite", "step_brute_force", "step_hermite_block", "step_brute_force"):
            assert s.do(name)[0] == "ok", s._say(name)
        s.option("train", 4)
        for name in ("acc_jerk_subset(64)", "step_hermite_block"):
            assert s.do(name)[0] == "ok", s._say(name)
        s.option("train", 0)
    s.finish("shrink and grow")


def test_law_dimension_and_quadrupole_flips_between_steps_of_every_kind(rx):
    s = Sequence(rx, _sphere(rx, 321, 30))
    for mover in list(MOVERS) * 2:
        s.do(mover)
        s.option("law", _flip("reference", "newton", s.o["law"]))
        s.do(mover)
        s.option("bh_dim", _flip(2, 3, s.o["bh_dim"]))
        s.do(mover)
    s.option("law", "newton")
    s.option("bh_dim", 3)
    for quad in (False, True, False):
        assert s.do("step_barnes_hut(0.5)")[0] == "ok"
        s.option("quad", quad)
    assert s.do("step_barnes_hut(0.85)")[0] == "ok"
    s.finish("flips")


def test_a_planar_state_on_the_octree_path_then_z_then_planar_again(rx):
    gal, sph = _copy(rx.two_galaxies(321)), _sphere(rx, 321, 31)
    s = Sequence(rx, gal, bh_dim=3)
    for st in (gal, sph, gal):
        if st is not gal or s.log:
            s.replace(st)
        for name in ("step_barnes_hut(0.5)", "forces(0.5) octree", "step_hermite", "step_hermite", "acc_jerk_f64()", "step_brute_force",
                     "bh_oct_moments", "step_barnes_hut(0.85)"):
            assert s.do(name)[0] == "ok", s._say(name)
        assert bool(s.e.get_particles()["pz"].any()) == (st is sph)
    s.finish("z")


def test_a_root_box_too_large_for_21_levels_is_refused_and_the_next_step_works(rx):
    st = _copy(_with(system("s65"), [(0.1, 0.1, 0.1), (0.101, 0.101, 0.101), (-5e6, -5e6, -5e6), (5e6, 5e6, 5e6)]))
    s = Sequence(rx, system("s65"), bh_dim=3)
    s.do("step_hermite")
    s.replace(st)
    for name in ("step_barnes_hut(0.5)", "forces(0.5) octree"):
        assert s.do(name) == ("err", rx.NBX_ERR_TREE_DEPTH), s._say(name)
    for name in ("step_brute_force", "step_hermite", "forces_f64"):
        assert s.do(name)[0] == "ok", s._say(name)
    s.finish("tree depth")


# ---- 4. seeded random sequences ------------------------------------------------------------------------------------------------------
def _random_system(rx, rng):
    """(state, clean): clean = no coincident or EPS-close bodies (those keep the block levels at 0 and stay off the device quadtree,
    whose refusals start a back-off that a fresh engine does not have)"""
    pick = rng.choice(["sphere", "galaxies", "pair", "dup", "equal"])
    n = int(rng.choice([1, 2, 63, 64, 65, 321, 1100, 2051]))
    if pick == "pair" or pick == "dup":
        return _copy(system(pick)), False
    if pick == "galaxies":
        return _copy(rx.two_galaxies(n)), True
    if pick == "equal":
        return _copy(rx.plummer_sphere(n, dim=3)), True
    return _sphere(rx, n, int(rng.integers(1 << 30))), True


def _vary(st, rng):
    """set_particles variants of the same count: one exceptional mass, all different, all equal, z zeroed, z back"""
    st, n = _copy(st), len(st["m"])
    how = rng.choice(["same", "exceptional", "different", "equal", "planar", "z"])
    if how == "exceptional":
        st["m"][:] = 1.0
        st["m"][n // 2] = 1000.0
    elif how == "different":
        st["m"] = rng.uniform(0.5, 2.0, n).astype(np.float32)
    elif how == "equal":
        st["m"][:] = 1.5
    elif how == "planar":
        st["pz"][:] = 0
        st["vz"][:] = 0
    elif how == "z":
        st["pz"] = rng.normal(0, 1, n).astype(np.float32)
    return st, how


@pytest.mark.parametrize("seed", range(12))
def test_seeded_random_sequences_replay_on_a_fresh_engine(rx, seed):
    rng = np.random.default_rng(1000 + seed)
    st, clean = _random_system(rx, rng)
    s = Sequence(rx, st, eta=0.02 if clean else 0.0)
    s.log.append(f"seed {seed}: n = {len(st['m'])}, clean = {clean}")
    names = list(MOVERS) * 3 + list(PROBES)
    try:
        for _ in range(16):
            r = rng.random()
            n = s.e.num_particles()
            if r < 0.2:
                key = rng.choice(["law", "bh_dim", "quad", "tree", "bh_async", "train"])
                value = {"law": _flip("reference", "newton", s.o["law"]), "bh_dim": _flip(2, 3, s.o["bh_dim"]), "quad": not s.o["quad"],
                         "tree": rng.choice(["auto", "host"] + (["device"] if clean and n >= SMALL_DEVICE else [])),
                         "bh_async": 1 - s.o["bh_async"], "train": 4 - s.o["train"]}[key]
                s.option(str(key), value if key != "tree" else str(value))
            elif r < 0.3:
                if rng.random() < 0.5:
                    st, how = _vary(s.e.get_particles(), rng)
                    s.replace(st, "load" if rng.random() < 0.3 else "set_particles")
                    s.log[-1] += f" ({how})"
                else:
                    st, clean = _random_system(rx, rng)
                    if not (clean and len(st["m"]) >= SMALL_DEVICE) and s.o["tree"] == "device":
                        s.option("tree", "auto")
                    s.o["eta"] = 0.02 if clean else 0.0
                    s.replace(st)
            else:
                s.do(str(rng.choice(names)))
        s.finish(f"seed {seed}")
    except AssertionError:
        print(s._say(f"seed {seed} failed"))
        raise
