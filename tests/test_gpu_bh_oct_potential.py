"""K14: the potential of the Newtonian octree walk (nbx_bh_potential / nbx_bh_conserved; bh_oct_potential.hip) against a float64
restatement over the DUMPED nodes and moments: x = c' - p, u = |x|^2 + eps, r = u^(-1/2); a leaf adds -M r, an accepted interior node
-M r + 0.5 tr(P) r^3 - 1.5 (x^T P x) r^5; f32 opening decision of test_gpu_bh_oct; the readout adds the own share m_i / sqrt(eps).
Bound per body: (terms + K) * 2^-24 * sum |piece|, terms = the accepted nodes, |piece| = every product of a node's contribution by its
absolute value, plus m_i / sqrt(eps).  K by the rules of test_gpu_newton.py / test_gpu_bh_oct_newton.py:
  x_k 1; x_k^2 3; d2 5; u 6; r = v_rsq_f32: 6 / 2 + 2 = 5; -M r inside the accumulating FMA 5 (its addition is one of the `terms`); the
  own share m_i v_rsq_f32(eps) 2 inside an FMA, whose addition is one more term                                      -> K = 6 (monopole)
  r2 11; r3 17; r5 29; M r 6; low = fma(0.5 tr, r3, -M r): 17, rounded 18; Pxx x^2 4, two FMAs 6; xy 3, Pxy xy 4, two FMAs 6;
  x^T P x = fma(2, off, diag) 7; -1.5 (..) 8, times r5 inside an FMA 37, rounded 38; the own share's addition 39   -> K = 39 (quadrupole)"""
import functools
import math

import numpy as np
import pytest

from test_gpu_bh_oct import EPS, device_tree, f32, pos, system
from test_gpu_bh_oct_newton import MOM, check, device_moments, newton

pytestmark = pytest.mark.gpu
U, KQ, OWN = 2.0 ** -24, {True: 39, False: 6}, float(EPS) ** -0.5
bits = lambda p: np.stack([p[k] for k in sorted(p)]).view(np.uint32)  # noqa: E731


def ref_phi(nodes, mom, P, m, theta, quad):
    """(phi [n], accepted nodes [n], sum |piece| [n]) in float64, node-major over the dumped arrays, own share included"""
    phi = m.astype(np.float64) * OWN
    mag, cnt, nxt = phi.copy(), np.zeros(len(m), int), np.zeros(len(m), int)
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
        big = float(nd["m"]) * r
        term = -big
        if quad and nd["interior"]:
            tr, q = float(mom[k]["tr"]), np.array([mom[k][f] for f in MOM], np.float64)
            w = np.concatenate([x * x, 2.0 * x[:, [0, 0, 1]] * x[:, [1, 2, 2]]], 1) * q      # the six pieces of x^T P x
            term = term + 0.5 * tr * r ** 3 - 1.5 * w.sum(1) * r ** 5
            big = big + 0.5 * tr * r ** 3 + 1.5 * np.abs(w).sum(1) * r ** 5
        phi[t] += term
        mag[t] += big
        cnt[t] += 1
        nxt[t], nxt[act[~take]] = nd["skip"], k + 1
    return phi, cnt, mag


@functools.lru_cache(maxsize=None)
def restated(name, theta, quad):
    st = system(name)
    return ref_phi(device_tree(name), device_moments(name), pos(st), st["m"], theta, quad)


@pytest.mark.parametrize("quad", [True, False])
@pytest.mark.parametrize("theta", [0.5, 0.85])
@pytest.mark.parametrize("name", ["n1", "n2", "s65", "pair", "dup", "gal2051", "s2051"])
def test_potential_matches_the_restated_walk(name, theta, quad):
    want, terms, mag = restated(name, theta, quad)
    got = newton(system(name), quad).bh_potential(theta)
    check(got, want, (terms + KQ[quad]) * U * mag, f"{name} theta={theta} quad={quad}")


@pytest.mark.parametrize("name", ["s65", "s2051"])
def test_every_node_opened_gives_the_direct_sum(name):
    st = system(name)
    want, n = newton(st).forces_f64()[3], len(st["m"])
    assert int((device_tree(name)["interior"] == 0).sum()) == n          # one body per leaf: the own share is exact
    got = newton(st).bh_potential(1e-6)
    check(got, want, (n + KQ[False]) * U * (np.abs(want) + st["m"].astype(np.float64) * OWN), name)   # |want| = sum over j != i
    assert np.array_equal(got.view(np.uint32), newton(st, quad=False).bh_potential(1e-6).view(np.uint32))   # only leaves are evaluated


def test_the_moments_earn_their_keep():
    st = system("s2051")
    want = newton(st).forces_f64()[3]
    rms = lambda phi: float(np.sqrt(((np.asarray(phi, np.float64) - want) ** 2).mean()))  # noqa: E731
    ref = {q: rms(restated("s2051", 0.5, q)[0]) for q in (True, False)}
    got = {q: rms(newton(st, q).bh_potential(0.5)) for q in (True, False)}
    print("rms error of phi at theta = 0.5: restated quadrupole / monopole", ref[True], ref[False], "device", got[True], got[False])
    assert ref[True] < ref[False] and got[True] < got[False]


@pytest.mark.parametrize("name", ["s2051", "gal2051"])
def test_conserved_sums_take_the_walks_potential(name):
    st = system(name)
    e = newton(st)
    full, tree = e.conserved(), e.bh_conserved(0.5)
    assert all(np.array_equal(np.asarray(full[k]).view(np.uint64), np.asarray(tree[k]).view(np.uint64)) for k in full if k != "potential")
    terms = 0.5 * st["m"].astype(np.float64) * e.bh_potential(0.5).astype(np.float64)     # exact products of widened floats
    bound = (len(terms) + 16) * 2.0 ** -53 * np.abs(terms).sum()                          # test_gpu_diag64's sum over the slab
    print(name, "W tree / all-pairs:", tree["potential"], full["potential"], "error / bound:", abs(tree["potential"] - math.fsum(terms)) / bound)
    assert abs(tree["potential"] - math.fsum(terms)) <= bound


def test_probes_leave_the_state_and_the_next_step_alone():
    e, fresh = newton(system("s2051")), newton(system("s2051"))
    before = bits(e.get_particles())
    e.bh_potential(0.5)
    e.bh_conserved(0.5)
    assert np.array_equal(bits(e.get_particles()), before)
    for probe in (lambda: e.bh_conserved(0.85), lambda: e.bh_potential(0.5)):   # step, probe, step = step, step
        e.step_barnes_hut(0.5, 0.01)
        fresh.step_barnes_hut(0.5, 0.01)
        probe()
        assert np.array_equal(bits(e.get_particles()), bits(fresh.get_particles()))


REFUSED = {"NBX_OPT_LAW": lambda e: e.set_law("reference"), "NBX_OPT_BH_DIM": lambda e: e.set_bh_dim(2), "strict": lambda e: e.set_mode("strict"),
           "fp16 sources": lambda e: e.set_source_precision(16), "shard": lambda e: e.set_shard(0, 2), "theta 0": 0.0, "theta -1": -1.0,
           "theta nan": float("nan")}


@pytest.mark.parametrize("how", list(REFUSED))
def test_unserved_configurations_and_thetas_refuse(rx, how):
    e = newton(system("s65"))
    before = bits(e.get_particles())
    theta, want = (0.5, rx.NBX_ERR_STATE) if callable(REFUSED[how]) else (REFUSED[how], rx.NBX_ERR_INVALID)
    if callable(REFUSED[how]):
        REFUSED[how](e)
    for call in (lambda: e.bh_potential(theta), lambda: e.bh_conserved(theta)):
        with pytest.raises(rx.NBodyError) as err:
            call()
        assert err.value.code == want and (not how.startswith("NBX_OPT") or how in str(err.value))   # the option at fault, by name
    assert np.array_equal(bits(e.get_particles()), before)
