"""nbx_forces_f64 / nbx_conserved (K7, diag64.hip) against an exact-sum reference: every pair term in numpy float64, every sum
with math.fsum.

The bound is derived, not measured.  A sum of n terms, each computed to within 16 roundings, is off by at most
(n + 16) * 2^-53 * sum|term| in any summation order; so every force component and phi_i is held to that with the reference's own
sum|term_ij| over the sources, and eleven of the conserved sums to the same with sum|term_i| over the slab.  The twelfth,
POTENTIAL = sum_i 1/2 m_i phi_i, is a sum over pairs: phi_i is off by at most (n + 16) u sum_j|term_ij| and the outer sum of slab
terms adds (slab + 16) u sum_i|1/2 m_i phi_i|, together at most (n + slab + 32) u * sum over the slab's pairs of |pair term|."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EPS = float(np.float32(0.0001))
KEYS = ("px", "py", "pz", "vx", "vy", "vz", "m")


def _sphere(rx, n, seed):
    """Plummer sphere with masses in [0.5, 2) and velocities in [-1, 1)^3"""
    rng = np.random.default_rng(seed)
    st = rx.plummer_sphere(n)
    st["m"] = rng.uniform(0.5, 2.0, n).astype(np.float32)
    for k in ("vx", "vy", "vz"):
        st[k] = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    return st


def _coincident(rx):
    st = _sphere(rx, 204, 5)
    for k in ("px", "py", "pz"):
        st[k][[7, 99, 100, 203]] = st[k][7]
    return st


CASES = {
    "one": lambda rx: _sphere(rx, 1, 1),                      # no pair
    "two": lambda rx: _sphere(rx, 2, 2),                      # one pair
    "wave+1": lambda rx: _sphere(rx, 65, 3),                  # one body past a wave; unequal masses; real z
    "block+1": lambda rx: _sphere(rx, 769, 4),                # 64 * T * k + 1 for T = 1, 2 and 4: a last target block of one body
    "galaxies": lambda rx: rx.two_galaxies(2051),             # source split > 1 with a short last range; planar; mass ratio 1000
    "coincident": _coincident,                                # 200 bodies + 4 at one position
    "shard": lambda rx: _sphere(rx, 777, 6),
}


@functools.lru_cache(maxsize=None)
def _case(rx, name):
    st = CASES[name](rx)
    return st, _reference(st)


def _reference(st):
    """(value, sum|term|) of (Fx, Fy, Fz, phi) per body [n, 4] and of the twelve conserved terms per body [n, 12] (exact sums
    over the sources; the conserved sums over any slab are fsums of its rows)."""
    x, y, z, vx, vy, vz, m = (np.asarray(st[k], np.float64) for k in KEYS)
    P = np.stack([x, y, z], 1)
    n = len(m)
    val, mag = np.zeros((n, 4)), np.zeros((n, 4))
    for i in range(n):
        d = np.delete(P, i, 0) - P[i]
        mj = np.delete(m, i)
        r2 = (d * d).sum(1) + EPS
        terms = np.column_stack([m[i] * (mj / r2)[:, None] * d, mj * (0.5 * np.log(r2))])
        val[i] = [math.fsum(c) for c in terms.T]
        mag[i] = np.abs(terms).sum(0)
    cons = np.stack([0.5 * (m * (vx * vx + vy * vy + vz * vz)), 0.5 * (m * val[:, 3]), m, m * vx, m * vy, m * vz,
                     m * (y * vz - z * vy), m * (z * vx - x * vz), m * (x * vy - y * vx), m * x, m * y, m * z], 1)
    cmag = np.abs(cons)
    cmag[:, 1] = 0.5 * m * mag[:, 3]
    return val, mag, cons, cmag


def _flat(c):
    return np.concatenate([[c["kinetic"], c["potential"], c["mass"]], c["momentum"], c["angular_momentum"], c["mass_moment"]])


def _check(e, st, ref, what):
    """forces_f64 with and without the potential, and conserved(), of engine e's slab against the reference"""
    val, mag, cons, cmag = ref
    n = len(st["m"])
    lo, hi = e.slab()
    bound = (n + 16) * U * mag[lo:hi]
    for potential in (True, False):
        got = e.forces_f64(potential=potential)
        ll = e.last_launch()
        assert ll["variant"] == 64 and ll["block"] == 256 and ll["bodies_per_thread"] in (1, 2, 4), ll
        for k in range(4 if potential else 3):
            err = np.abs(got[k] - val[lo:hi, k])
            worst = float((err / np.maximum(bound[:, k], 1e-300)).max()) if hi > lo else 0.0
            print(f"{what} potential={potential} component {k}: worst error / bound = {worst:.3f}")
            assert np.all(err <= bound[:, k]), (what, potential, k, worst)
    got = _flat(e.conserved())
    want = np.array([math.fsum(c) for c in cons[lo:hi].T])
    cbound = (hi - lo + 16) * U * cmag[lo:hi].sum(0)
    cbound[1] = (n + hi - lo + 32) * U * cmag[lo:hi, 1].sum()
    print(f"{what} conserved: error / bound = {np.abs(got - want) / np.maximum(cbound, 1e-300)}")
    assert np.all(np.abs(got - want) <= cbound), (what, got, want, cbound)
    return got, cbound


def _engine(rx, st, rank=0, world=1):
    e = rx.NBodyEngine()
    e.set_shard(rank, world)
    e.set_particles(*(st[k] for k in ("px", "py", "vx", "vy", "m", "pz", "vz")))
    return e


@pytest.mark.parametrize("name", ["one", "two", "wave+1", "block+1", "galaxies", "coincident"])
def test_forces_potential_and_sums_within_the_summation_bound(rx, name):
    st, ref = _case(rx, name)
    e = _engine(rx, st)
    _check(e, st, ref, name)
    if name == "galaxies":
        assert e.last_launch()["jsplit"] >= 2     # (coincident bodies: a NaN anywhere fails every comparison of _check)


def test_every_slab_of_a_three_way_shard_and_the_ranks_add_up(rx):
    st, ref = _case(rx, "shard")
    whole, bound = _check(_engine(rx, st), st, ref, "unsharded")
    parts = []
    for rank in range(3):
        e = _engine(rx, st, rank, 3)
        assert e.slab() == (259 * rank, 777 if rank == 2 else 259 * (rank + 1))
        parts.append(_check(e, st, ref, f"rank {rank}")[0])
    assert np.all(np.abs(np.sum(parts, 0) - whole) <= bound), (parts, whole, bound)


def test_conserved_reads_the_live_device_state_and_leaves_it_alone(rx):
    """Three Barnes-Hut steps leave the state on the device with a step still in flight: conserved() resolves it, reads that
    state, changes nothing and repeats bit for bit."""
    st0 = rx.two_galaxies(777)
    e = _engine(rx, st0)
    for _ in range(3):
        e.step_barnes_hut(0.85, 0.01, 1)
    first = _flat(e.conserved())
    before = e.get_particles()
    assert any(np.any(before[k] != st0[k]) for k in ("px", "py"))
    ref = _reference(before)
    got, bound = _check(e, before, ref, "after three steps")
    assert np.array_equal(first.view(np.uint64), got.view(np.uint64))
    fx, fy, fz, phi = e.forces_f64()
    again = e.forces_f64()
    assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip((fx, fy, fz, phi), again))
    assert abs(math.fsum(0.5 * before["m"].astype(np.float64) * phi) - got[1]) <= bound[1]
    after = e.get_particles()
    assert all(np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)) for k in KEYS)
