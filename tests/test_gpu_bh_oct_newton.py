"""K13: the octree path under the Newtonian law (NBX_OPT_BH_DIM = 3, NBX_OPT_LAW = 1; bh_oct_newton.hip) against float64 restatements
over the DUMPED nodes and the DUMPED moments.  With x = c' - p, u = |x|^2 + eps, r = u^(-1/2), a leaf adds M x r^3 and an accepted
interior node x (M r^3 - 1.5 tr(P) r^5 + 7.5 (x^T P x) r^7) - 3 r^5 (P x); the opening decision is the f32 one of test_gpu_bh_oct.

Walk bound per component: (terms + K) * 2^-24 * sum |term|, terms = the accepted nodes of the body, |term| = the node's contribution
with every product replaced by its absolute value (the pieces of the quadrupole term cancel in part: a rounding is relative to a
piece, not to their sum).  K by the rules of test_gpu_newton.py, relative to that majorant:
  x_k 1; x_k^2 3; d2 = (.. + ..) + .. 5; u = d2 + eps 6; r = v_rsq_f32: 6 / 2 + 2 = 5; r2 = r r 11; r3 = r2 r 17; M r3 18; the
  product with x_k inside the accumulating FMA 19; m_i in the readout 20                                              -> K = 20 (monopole)
  r5 = r3 r2 29; r7 = r5 r2 41; q = P x: product 2, two FMAs 4; x.q: 6, two FMAs 8; 7.5 (x.q) 9, times r7 inside an FMA 50;
  -1.5 tr 1, times r5 inside an FMA 30, that FMA's sum with M r3 31; s = the outer FMA 51; s x_k inside an FMA 52; w = -3 r5 30,
  w q_k 35; the FMA s x_k + w q_k 53 (its addition to the sum is one of the `terms`); m_i 54                          -> K = 54 (quadrupole)

Moments bound per entry: 2^-24 |want| (the one fp32 rounding) + R 2^-53 tr(want), R = 21 levels x 8 children x 12 fp64 roundings per
shifted child and entry (Delta_i, m Delta_i, two products D Delta and their sum, + P_c, the product m Delta_i Delta_j, its addition,
the addition into the parent = 9; D_c + m Delta and its addition into D, which the next level multiplies = 2; the fp64 mass's own
addition = 1) = 2016."""
import functools

import numpy as np
import pytest

from test_gpu_bh_oct import EPS, device_tree, engine_of, f32, pos, system

pytestmark = pytest.mark.gpu
U, R = 2.0 ** -24, 21 * 8 * 12
KQ = {True: 54, False: 20}
MOM = ("xx", "yy", "zz", "xy", "xz", "yz")


def newton(st, quad=True):
    e = engine_of(st)
    e.set_law("newton")
    e.set_bh_quadrupole(quad)
    return e


@functools.lru_cache(maxsize=None)
def device_moments(name):
    return engine_of(system(name)).bh_oct_moments()


def ref_walk(nodes, mom, P, m, theta, quad):
    """(F = m a [n, 3], accepted nodes [n], sum |term| of F [n, 3]) in float64, node-major over the dumped arrays"""
    n = len(m)
    acc, mag, cnt, nxt = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, int), np.zeros(n, int)
    for k, nd in enumerate(nodes):
        act = np.nonzero(nxt == k)[0]
        if not len(act):
            continue
        c = np.array([nd["px"], nd["py"], nd["pz"]], f32)
        d = c - P[act]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            take = (f32(nd["s"]) / np.sqrt(d2) < f32(theta)) if nd["interior"] else np.ones(len(act), bool)
        t = act[take]
        x = c.astype(np.float64) - P[t].astype(np.float64)
        r = ((x * x).sum(1) + float(EPS)) ** -0.5
        term = float(nd["m"]) * x * (r ** 3)[:, None]
        big = np.abs(term)
        if quad and nd["interior"]:
            q = mom[k]
            Q = np.array([[q["xx"], q["xy"], q["xz"]], [q["xy"], q["yy"], q["yz"]], [q["xz"], q["yz"], q["zz"]]], np.float64)
            Qx, aQx = x @ Q, np.abs(x) @ np.abs(Q)
            term = term + x * (-1.5 * float(q["tr"]) * r ** 5 + 7.5 * (x * Qx).sum(1) * r ** 7)[:, None] - 3.0 * (r ** 5)[:, None] * Qx
            big = big + np.abs(x) * (1.5 * float(q["tr"]) * r ** 5 + 7.5 * (np.abs(x) * aQx).sum(1) * r ** 7)[:, None] + 3.0 * (r ** 5)[:, None] * aQx
        acc[t] += term
        mag[t] += big
        cnt[t] += 1
        nxt[t], nxt[act[~take]] = nd["skip"], k + 1
    w = m.astype(np.float64)[:, None]
    return acc * w, cnt, mag * w


@functools.lru_cache(maxsize=None)
def restated(name, theta, quad):
    st = system(name)
    return ref_walk(device_tree(name), device_moments(name), pos(st), st["m"], theta, quad)


def check(got, want, bound, what):
    err = np.abs(np.asarray(got, np.float64) - want)
    print(f"{what}: worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound), what


@pytest.mark.parametrize("name", ["s65", "pair", "dup", "s2051"])
def test_moments_are_the_direct_sums_over_the_leaves(name):
    t, got = device_tree(name), device_moments(name)
    assert len(got) == len(t)
    C = np.stack([t["px"], t["py"], t["pz"]], 1).astype(np.float64)
    want = np.zeros((len(t), 7))
    for k in np.nonzero(t["interior"])[0]:
        leaves = np.arange(k + 1, t["skip"][k])[t["interior"][k + 1:t["skip"][k]] == 0]
        x, w = C[leaves] - C[k], t["m"][leaves].astype(np.float64)
        S = (x * w[:, None]).T @ x
        want[k] = [S[0, 0], S[1, 1], S[2, 2], S[0, 1], S[0, 2], S[1, 2], S[0, 0] + S[1, 1] + S[2, 2]]
    G = np.stack([got[f] for f in MOM + ("tr",)], 1)
    assert not G[t["interior"] == 0].any() and not got["pad"].any()
    check(G, want, U * np.abs(want) + R * 2.0 ** -53 * want[:, 6:7], name)


@pytest.mark.parametrize("quad", [True, False])
@pytest.mark.parametrize("theta", [0.5, 0.85])
@pytest.mark.parametrize("name", ["n1", "n2", "s65", "pair", "dup", "gal2051", "s2051"])
def test_forces_match_the_restated_walk(name, theta, quad):
    want, terms, mag = restated(name, theta, quad)
    got = np.stack(newton(system(name), quad).forces(theta), 1)
    check(got, want, (terms[:, None] + KQ[quad]) * U * mag, f"{name} theta={theta} quad={quad}")


@pytest.mark.parametrize("name", ["s65", "s2051", "pair"])
def test_every_node_opened_gives_the_direct_sum(name):
    st = system(name)
    e = newton(st)
    want = np.stack(e.forces_f64(potential=False)[:3], 1)
    got = np.stack(e.forces(1e-6), 1)
    check(got, want, (len(st["m"]) + KQ[False]) * U * restated(name, 1e-6, False)[2], name)
    mono = np.stack(newton(st, quad=False).forces(1e-6), 1)
    assert np.array_equal(got.view(np.uint32), mono.view(np.uint32))   # only leaves are evaluated


def test_the_moments_earn_their_keep():
    st = system("s2051")
    e = newton(st)
    want = np.stack(e.forces_f64(potential=False)[:3], 1)
    rms = lambda F: float(np.sqrt(((F - want) ** 2).sum(1).mean()))  # noqa: E731
    ref = {q: rms(restated("s2051", 0.5, q)[0]) for q in (True, False)}
    got = {q: rms(np.stack(newton(st, q).forces(0.5), 1).astype(np.float64)) for q in (True, False)}
    print("rms error of F at theta = 0.5: restated quadrupole / monopole", ref[True], ref[False], "device", got[True], got[False])
    assert ref[True] < ref[False] and got[True] < got[False]


def test_step_kick_drift_and_kill_box():
    from rust_exp_amd.tolerances import fast_step_tolerances

    st = {k: v.copy() for k, v in system("s2051").items()}
    rng = np.random.default_rng(7)
    for k in ("vx", "vy", "vz"):
        st[k] = rng.normal(0.0, 2.0, len(st["m"])).astype(f32)
    last = len(st["m"]) - 1
    st["px"][last], st["py"][last], st["pz"][last] = 0.0, 0.0, 60.0      # outside the kill box on z alone
    dt, theta = 0.01, 0.5
    e = newton(st)
    a = ref_walk(e.bh_oct_dump(), e.bh_oct_moments(), pos(st), st["m"], theta, True)[0] / st["m"].astype(np.float64)[:, None]
    v = np.stack([st["vx"], st["vy"], st["vz"]], 1).astype(np.float64) + dt * a
    p = pos(st).astype(np.float64) + dt * v
    v[(np.abs(p) > 100.0 * 0.55).any(1)] = 0.0
    e.step_barnes_hut(theta, dt)
    out = e.get_particles()
    ptol, vtol = fast_step_tolerances(float(np.linalg.norm(a, axis=1).max()), len(st["m"]), dt)
    assert np.abs(np.stack([out["px"], out["py"], out["pz"]], 1) - p).max() <= ptol
    assert np.abs(np.stack([out["vx"], out["vy"], out["vz"]], 1) - v).max() <= vtol
    assert out["vx"][last] == 0.0 and out["vy"][last] == 0.0 and out["vz"][last] == 0.0


def test_the_reference_law_is_untouched_and_unserved_configurations_refuse(rx):
    st = system("s65")
    bits = lambda F: np.stack(F).view(np.uint32)  # noqa: E731
    fresh = bits(engine_of(st).forces(0.5))
    e = newton(st)
    assert np.any(bits(e.forces(0.5)) != fresh)
    e.set_law("reference")
    assert np.array_equal(bits(e.forces(0.5)), fresh)
    e.set_bh_quadrupole(False)
    assert np.array_equal(bits(e.forces(0.5)), fresh)
    for how in (lambda e: e.set_mode("strict"), lambda e: e.set_source_precision(16), lambda e: e.set_shard(0, 2)):
        e = newton(st)
        before = e.get_particles()
        how(e)
        for call in (lambda: e.step_barnes_hut(0.5, 0.01), lambda: e.forces(0.5)):
            with pytest.raises(rx.NBodyError) as err:
                call()
            assert err.value.code == rx.NBX_ERR_STATE
        after = e.get_particles()
        assert all(np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)) for k in before)
