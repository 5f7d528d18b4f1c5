"""The 3-D Barnes-Hut path (NBX_OPT_BH_DIM = 3: bh_oct.hip builds the octree, bh_oct_walk.hip walks it) against a plain Python
restatement of its semantics: the reference's tree rules (nbody.rs:186-480) with z added."""
import functools

import numpy as np
import pytest

from conftest import fp64_forces_sample

pytestmark = pytest.mark.gpu
f32 = np.float32
EPS = f32(1e-4)
LEVELS = 21


# ---- the restatement: a recursive build over f32 boxes, a node-major walk over a GIVEN node array ------------------------------
def ref_build(P, m):
    """Pre-order rows (px, py, pz, m as float64; s as f32; skip; interior; bodies in the node) of the octree of P [n, 3] f32."""
    n = len(m)
    lo, hi = np.repeat(P.min(0)[None], n, 0), np.repeat(P.max(0)[None], n, 0)   # root box: per-axis AABB, not cubic
    digs = np.zeros((n, LEVELS), int)
    for lvl in range(LEVELS):                                  # every body's path: child = 4 (z < cz) + 2 (y < cy) + (x >= cx)
        c = (lo + hi) * f32(0.5)                               # unfused f32 midpoints
        lt = P < c
        digs[:, lvl] = 4 * lt[:, 2] + 2 * lt[:, 1] + ~lt[:, 0]
        lo, hi = np.where(lt, lo, c), np.where(lt, c, hi)
    order = np.lexsort(digs.T[::-1])
    x1, x2 = P[:, 0].min(), P[:, 0].max()
    rows = []

    def node(a, b, depth, x1, x2):
        assert depth <= LEVELS
        k, ids = len(rows), order[a:b]
        rows.append(None)
        split = bool((digs[ids] != digs[ids[0]]).any())         # two bodies that do not share a level-21 cell
        if b - a == 1:
            rec = [float(v) for v in P[ids[0]]] + [float(m[ids[0]])]
        else:
            w = m[ids].astype(np.float64)
            rec = list((P[ids].astype(np.float64) * w[:, None]).sum(0) / w.sum()) + [w.sum()]
            assert split or ((P[ids].max(0) - P[ids].min(0)) < EPS).all(), "multi-body leaf wider than EPS"
        if split:
            cx = (x1 + x2) * f32(0.5)
            d = digs[ids, depth]
            for q in range(8):                                 # empty children dropped
                sel = np.nonzero(d == q)[0]
                if len(sel):
                    node(a + sel[0], a + sel[-1] + 1, depth + 1, *((cx, x2) if q & 1 else (x1, cx)))
        rows[k] = rec + [x2 - x1, len(rows), int(split), b - a]

    node(0, n, 0, x1, x2)
    return np.array(rows, dtype=np.float64)


def ref_walk(nodes, P, m, theta):
    """F = m a [n, 3] float64 of the walk over `nodes` (structured: px py pz m s skip interior): a node is accepted iff it is a
    leaf or s / sqrt(d2) < theta, d2 = (dx*dx + dy*dy) + dz*dz in f32; terms summed in float64."""
    n = len(m)
    acc, nxt = np.zeros((n, 3)), np.zeros(n, int)
    for k, nd in enumerate(nodes):
        act = np.nonzero(nxt == k)[0]
        if not len(act):
            continue
        d = np.array([nd["px"], nd["py"], nd["pz"]], f32) - P[act]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            take = (f32(nd["s"]) / np.sqrt(d2) < f32(theta)) if nd["interior"] else np.ones(len(act), bool)
        t = act[take]
        acc[t] += float(nd["m"]) * d[take].astype(np.float64) / (d2[take].astype(np.float64) + float(EPS))[:, None]
        nxt[t], nxt[act[~take]] = nd["skip"], k + 1
    return acc * m.astype(np.float64)[:, None]


# ---- the systems (seeded), their device trees and restated trees: made once ---------------------------------------------------
def _with(st, extra):
    out = {k: np.concatenate([st[k], np.zeros(len(extra), f32)]) for k in st}
    for i, (x, y, z) in enumerate(extra):
        j = len(st["m"]) + i
        out["px"][j], out["py"][j], out["pz"][j], out["m"][j] = x, y, z, st["m"][0]
    return out


@functools.lru_cache(maxsize=None)
def system(name):
    import rust_exp_amd as rx

    sphere = lambda n: rx.plummer_sphere(n, dim=3)  # noqa: E731
    return {"n1": lambda: sphere(1), "n2": lambda: sphere(2), "s65": lambda: sphere(65), "s2051": lambda: sphere(2051),
            "pair": lambda: _with(sphere(65), [(1.0, 2.0, 3.0), (1.0003, 2.0003, 3.0003)]),       # a long single-child chain
            "dup": lambda: _with(sphere(200), [(0.5, -0.25, 0.125)] * 4),                        # a multi-body leaf
            "gal2051": lambda: rx.two_galaxies(2051)}[name]()                                      # z == 0 everywhere


SYSTEMS = ["n1", "n2", "s65", "s2051", "pair", "dup", "gal2051"]


def engine_of(st, dim=3, mode="fast"):
    import rust_exp_amd as rx

    e = rx.NBodyEngine(mode=mode)
    e.set_bh_dim(dim)
    e.set_particles(st["px"], st["py"], st["vx"], st["vy"], st["m"], st["pz"], st["vz"])
    return e


def pos(st):
    return np.stack([st["px"], st["py"], st["pz"]], 1).astype(f32)


@functools.lru_cache(maxsize=None)
def device_tree(name):
    return engine_of(system(name)).bh_oct_dump()


def within_one_ulp(got, want64):
    return np.abs(got.astype(np.float64) - want64) <= np.spacing(np.abs(want64).astype(f32)).astype(np.float64)


@pytest.mark.parametrize("name", SYSTEMS)
def test_tree_equals_the_restated_build(name):
    st, t = system(name), device_tree(name)
    ref = ref_build(pos(st), st["m"])
    assert len(t) == len(ref)
    assert np.array_equal(t["skip"], ref[:, 5].astype(int)) and np.array_equal(t["interior"], ref[:, 6].astype(int))
    assert np.array_equal(t["s"], ref[:, 4].astype(f32))
    single = ref[:, 7] == 1
    for j, f in enumerate(("px", "py", "pz", "m")):
        assert within_one_ulp(t[f], ref[:, j]).all(), f
        assert np.array_equal(t[f][single].astype(np.float64), ref[single, j]), f   # a single body's leaf is the body, bit for bit


def test_planar_system_reduces_to_the_quadtree():
    t = device_tree("gal2051")
    q = engine_of(system("gal2051"), dim=2).bh_flat_dump(threaded="device")
    assert len(t) == len(q)
    for f in ("skip", "interior", "s"):
        assert np.array_equal(t[f], q[f]), f
    for f in ("px", "py", "m"):
        assert (np.abs(t[f].astype(np.float64) - q[f]) <= np.spacing(np.abs(q[f]))).all(), f
    assert not t["pz"].any()


@pytest.mark.parametrize("theta", [0.5, 0.85])
@pytest.mark.parametrize("name", SYSTEMS)
def test_forces_match_the_restated_walk(name, theta):
    st = system(name)
    want = ref_walk(device_tree(name), pos(st), st["m"], theta)
    got = np.stack(engine_of(st).forces(theta), 1)
    print(name, theta, "max err / max|F|:", np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
    assert np.abs(got - want).max() <= 2e-5 * np.abs(want).max()


@pytest.mark.parametrize("name", ["s65", "s2051", "pair"])
def test_every_node_opened_gives_the_direct_sum(name):
    st = system(name)
    want = fp64_forces_sample(st, np.arange(len(st["m"])), dim=3)
    got = np.stack(engine_of(st).forces(1e-6), 1)
    print(name, "max err / max|F|:", np.abs(got - want).max() / np.abs(want).max())
    assert np.abs(got - want).max() <= 2e-5 * np.abs(want).max()


def test_step_kick_drift_and_kill_box():
    from rust_exp_amd.tolerances import fast_step_tolerances

    st = {k: v.copy() for k, v in system("s2051").items()}
    rng = np.random.default_rng(7)
    for k in ("vx", "vy", "vz"):
        st[k] = rng.normal(0.0, 2.0, len(st["m"])).astype(f32)
    last = len(st["m"]) - 1
    st["px"][last], st["py"][last], st["pz"][last] = 0.0, 0.0, 60.0      # outside the kill box on z alone
    dt, theta = 0.01, 0.5
    e = engine_of(st)
    a = ref_walk(e.bh_oct_dump(), pos(st), st["m"], theta) / st["m"].astype(np.float64)[:, None]
    v = np.stack([st["vx"], st["vy"], st["vz"]], 1).astype(np.float64) + dt * a
    p = pos(st).astype(np.float64) + dt * v
    v[(np.abs(p) > 100.0 * 0.55).any(1)] = 0.0
    e.step_barnes_hut(theta, dt)
    out = e.get_particles()
    ptol, vtol = fast_step_tolerances(float(np.linalg.norm(a, axis=1).max()), len(st["m"]), dt)
    assert np.abs(np.stack([out["px"], out["py"], out["pz"]], 1) - p).max() <= ptol
    assert np.abs(np.stack([out["vx"], out["vy"], out["vz"]], 1) - v).max() <= vtol
    assert out["vx"][last] == 0.0 and out["vy"][last] == 0.0 and out["vz"][last] == 0.0
    flat = engine_of(st, dim=2)                                          # the default: z and vz untouched, as before
    flat.step_barnes_hut(theta, dt)
    out = flat.get_particles()
    assert np.array_equal(out["pz"], st["pz"]) and np.array_equal(out["vz"], st["vz"])


@pytest.mark.parametrize("how", ["strict", "shard"])
def test_unserved_configurations_are_refused(how):
    import rust_exp_amd as rx

    st = system("s65")
    e = rx.NBodyEngine(mode="strict" if how == "strict" else "fast")
    e.set_bh_dim(3)
    if how == "shard":
        e.set_shard(0, 2)
    e.set_particles(st["px"], st["py"], st["vx"], st["vy"], st["m"], st["pz"], st["vz"])
    for call in (lambda: e.step_barnes_hut(0.5, 0.01), lambda: e.forces(0.5)):
        with pytest.raises(rx.NBodyError) as err:
            call()
        assert err.value.code == rx.NBX_ERR_STATE


def test_root_box_too_large_for_21_levels():
    import rust_exp_amd as rx

    st = _with(system("s65"), [(0.1, 0.1, 0.1), (0.101, 0.101, 0.101), (-5e6, -5e6, -5e6), (5e6, 5e6, 5e6)])
    e = engine_of(st)
    with pytest.raises(rx.NBodyError) as err:
        e.step_barnes_hut(0.5, 0.01)
    assert err.value.code == rx.NBX_ERR_TREE_DEPTH
    out = e.get_particles()
    assert all(np.array_equal(out[k], st[k]) for k in st)
