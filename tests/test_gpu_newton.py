"""NBX_OPT_LAW = 1, the Plummer-softened Newtonian law, against its pair terms in numpy float64 summed with math.fsum:
    F_i = m_i sum_j m_j d s^(-3/2),   phi_i = -sum_{j != i} m_j s^(-1/2),   d = p_j - p_i, s = |d|^2 + eps
forces(0.0) (K11, force_newton.hip) is held per component to (n + K) * 2^-24 * sum_j |term|, forces_f64 / conserved (k_newton64) to the
same with 2^-53; POTENTIAL, a sum over pairs, to (n + slab + 2 K) u sum |pair term| as in test_gpu_diag64.py.  n: the summation of n
terms in any order.  K: the roundings that reach one term, counted from the sweep's instructions by the rules of test_gpu_hermite.py
(one per rounding, v_rsq_f32 = 2 like v_rcp_f32, a square root halves the relative error of its argument): every d_k is one
subtraction (1); s is three FMAs on squares of rounded d (3 + 2 = 5); u = rsq(s): 5 / 2 + 2 = 4.5; u u: 9 + 1 = 10; m_j u: 5.5;
w = (m_j u)(u u): 16.5; the term w d_k: 17.5 (the FMA's product is not rounded: its sum is the n); times m_i in the readout: 18.5.
With one common mass m_j leaves the loop (-1) and the common mass multiplies the finished sum (+1): the same.          -> K = 20
fp64: the same chain with u = v_rsq_f64 + two Newton steps, whose remaining roundings are the last step's product s y (by half) and
its closing FMA: 1.5, charged 2 like the fp32 instruction, so K = 20 there too; a potential term -m_j u carries 5.5 of them."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 20
EPS = float(np.float32(0.0001))
KEYS = ("px", "py", "pz", "vx", "vy", "vz", "m")


def _sphere(rx, n, seed, same=()):
    """Plummer sphere with masses in [0.5, 2) and velocities in [-1, 1)^3; the bodies `same` share one position"""
    rng = np.random.default_rng(seed)
    st = rx.plummer_sphere(n)
    st["m"] = rng.uniform(0.5, 2.0, n).astype(np.float32)
    for k in ("vx", "vy", "vz"):
        st[k] = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    for k in ("px", "py", "pz"):
        st[k][list(same)] = st[k][list(same)[:1]]
    return st


V = math.sqrt(0.5)
ORBIT = ([-0.5, 0.5], [0, 0], [0, 0], [0, 0], [-V, V], [0, 0], [1, 1])   # two bodies of mass 1, circular orbit of separation 1


CASES = {
    "one": lambda rx: _sphere(rx, 1, 1),                      # no pair, pads only; one mass: the unit-mass loop ends at n
    "two": lambda rx: _sphere(rx, 2, 2),                      # one pair
    "wave+1": lambda rx: _sphere(rx, 65, 3),                  # one body past a wave; unequal masses; real z
    "block+1": lambda rx: _sphere(rx, 257, 4),                # a last target block of one body, two source tiles
    "split3": lambda rx: _sphere(rx, 1100, 6),                # NBX_OPT_JSPLIT = 3: five tiles split unevenly
    "galaxies": lambda rx: rx.two_galaxies(515),              # planar: the DIM = 2 kernels; mass ratio 1000
    "equal": lambda rx: rx.plummer_sphere(300),               # variant 31, n no multiple of 64 inside a wave's quarter
    "coincident": lambda rx: _sphere(rx, 204, 5, (7, 99, 100, 203)),   # 200 bodies + 4 at one position: exact-zero force terms
    "block64+1": lambda rx: _sphere(rx, 769, 4),              # fp64: 64 * T * k + 1 targets for T = 1, 2, 4
    "galaxies64": lambda rx: rx.two_galaxies(2051),           # fp64: source split > 1 with a short last range
    "orbit": lambda rx: {k: np.asarray(c, np.float32) for k, c in zip(KEYS, ORBIT)},
}


def _pairs(st):
    P = np.stack([np.asarray(st[k], np.float64) for k in KEYS[:3]], 1)
    d = P[None, :, :] - P[:, None, :]                       # [i, j] = p_j - p_i
    return P, np.stack([np.asarray(st[k], np.float64) for k in KEYS[3:6]], 1), np.asarray(st["m"], np.float64), d, (d * d).sum(2) + EPS


@functools.lru_cache(maxsize=None)
def _case(rx, name):
    """the state; (value, sum|term|) of (Fx, Fy, Fz, phi) per body [n, 4]; the twelve conserved terms per body and their magnitudes"""
    st = CASES[name](rx)
    P, V, m, d, s = _pairs(st)
    n = len(m)
    u = 1.0 / np.sqrt(s)
    terms = np.concatenate([(m[:, None] * m[None, :] * u * u * u)[:, :, None] * d, (-m[None, :] * u)[:, :, None]], 2)
    terms[np.arange(n), np.arange(n), 3] = 0.0                # phi excludes j = i
    val = np.array([[math.fsum(terms[i, :, k]) for k in range(4)] for i in range(n)])
    mag = np.abs(terms).sum(1)
    x, y, z, (vx, vy, vz) = *P.T, V.T
    cons = np.stack([0.5 * (m * (V * V).sum(1)), 0.5 * (m * val[:, 3]), m, m * vx, m * vy, m * vz, m * (y * vz - z * vy),
                     m * (z * vx - x * vz), m * (x * vy - y * vx), m * x, m * y, m * z], 1)
    cmag = np.abs(cons)
    cmag[:, 1] = 0.5 * m * mag[:, 3]
    return st, val, mag, cons, cmag


def _engine(rx, st, law="newton"):
    e = rx.NBodyEngine()
    e.set_particles(*(st[k] for k in ("px", "py", "vx", "vy", "m", "pz", "vz")))   # (all z zero: the planar kernels)
    e.set_law(law)
    return e


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in KEYS)


def _within(got, val, bound, what):
    err = np.abs(np.asarray(got, np.float64) - val)
    print(f"{what}: worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound), what


@pytest.mark.parametrize("name", ["one", "two", "wave+1", "block+1", "split3", "galaxies", "equal", "coincident"])
def test_fp32_sweep_within_the_summation_bound(rx, name):
    st, val, mag, _, _ = _case(rx, name)
    e = _engine(rx, st)
    e.set_launch(jsplit=3 if name == "split3" else 0)
    got = e.forces(0.0)
    ll = e.last_launch()
    assert ll["variant"] == (31 if st["m"].min() == st["m"].max() else 30) and ll["dim"] == (2 if name == "galaxies" else 3), ll
    assert ll["bodies_per_thread"] == 4 and (name != "split3" or ll["jsplit"] == 3), ll
    for k in range(3):
        _within(got[k], val[:, k], (len(st["m"]) + K) * 2.0 ** -24 * mag[:, k], f"{name} component {k}")


def test_law_is_off_by_default_and_switches_back_bit_for_bit(rx):
    st = _case(rx, "wave+1")[0]
    fresh = _engine(rx, st, "reference").forces(0.0)
    e = _engine(rx, st, "newton")
    newton = e.forces(0.0)
    assert any(np.any(a != b) for a, b in zip(fresh, newton))
    e.set_law("reference")
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(fresh, e.forces(0.0)))


@pytest.mark.parametrize("name", ["one", "two", "wave+1", "block64+1", "coincident", "galaxies64"])
def test_fp64_forces_potential_and_conserved_sums(rx, name):
    st, val, mag, cons, cmag = _case(rx, name)
    n, u = len(st["m"]), 2.0 ** -53
    e = _engine(rx, st)
    for potential in (True, False):
        got = e.forces_f64(potential=potential)
        assert e.last_launch()["variant"] == 65
        for k in range(4 if potential else 3):
            _within(got[k], val[:, k], (n + K) * u * mag[:, k], f"{name} potential={potential} component {k}")
    c = e.conserved()
    got = np.hstack([c["kinetic"], c["potential"], c["mass"], c["momentum"], c["angular_momentum"], c["mass_moment"]])
    cbound = (n + K) * u * cmag.sum(0)
    cbound[1] = (2 * n + 2 * K) * u * cmag[:, 1].sum()
    _within(got, np.array([math.fsum(col) for col in cons.T]), cbound, f"{name} conserved")
    assert _same_bits(st, e.get_particles())


@pytest.mark.parametrize("name", ["wave+1", "orbit"])
def test_three_brute_force_steps_follow_the_kick_drift_in_float64(rx, name):
    st = _case(rx, name)[0]
    dt, e = 0.01, _engine(rx, st)
    P, V, m, d, s = _pairs(st)
    amax = None
    for _ in range(3):
        e.step_brute_force(dt)
        d = P[None, :, :] - P[:, None, :]
        a = ((m[None, :] * ((d * d).sum(2) + EPS) ** -1.5)[:, :, None] * d).sum(1)
        amax = np.sqrt((a * a).sum(1)).max() if amax is None else amax
        V = V + dt * a
        P = P + dt * V
    ptol, vtol = rx.fast_step_tolerances(amax, len(m), dt, 3)
    got = e.get_particles()
    dp = max(np.abs(got[k] - P[:, i]).max() for i, k in enumerate(KEYS[:3]))
    dv = max(np.abs(got[k] - V[:, i]).max() for i, k in enumerate(KEYS[3:6]))
    assert dp <= ptol and dv <= vtol and e.last_launch()["variant"] in (30, 31), (dp / ptol, dv / vtol)


REFUSED = {
    "bh_step": lambda e: e.step_barnes_hut(0.5, 0.01),
    "bh_forces": lambda e: e.forces(0.5),
    "step_hermite": lambda e: e.step_hermite(0.01),
    "acc_jerk": lambda e: e.acc_jerk(),
    "step_hermite_block": lambda e: e.step_hermite_block(0.01, 0.02),
    "strict": lambda e: (e.set_mode("strict"), e.step_brute_force(0.01)),
    "fp16_sources": lambda e: (e.set_source_precision(16), e.step_brute_force(0.01)),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_paths_without_a_newtonian_form_refuse_and_leave_the_state(rx, name):
    e = _engine(rx, _case(rx, "wave+1")[0])
    e.step_brute_force(0.01)
    before = e.get_particles()
    with pytest.raises(rx.NBodyError) as err:
        REFUSED[name](e)
    assert err.value.code == rx.NBX_ERR_STATE and "NBX_OPT_LAW" in str(err.value)
    assert _same_bits(before, e.get_particles())
