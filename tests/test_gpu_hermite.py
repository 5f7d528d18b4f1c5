"""nbx_acc_jerk / nbx_step_hermite / nbx_hermite_timestep (K8, hermite.hip) against the formulas restated in numpy float64:

    a_i = sum_j m_j d / s,   j_i = sum_j m_j (w / s - 2 (d.w) d / s^2),   d = p_j - p_i, w = v_j - v_i, s = |d|^2 + eps

acc_jerk is held to a derived bound per component, (n + K) * 2^-24 * sum_j |term|, against exact sums (math.fsum) of float64
terms.  n: the fp32 summation of n terms in any order.  K: the roundings that reach one term, counted from the sweep's
instructions (v_rcp_f32 = 2): every d_k and w_k is one subtraction (1 each); s is three FMAs on squares of rounded d (3 + 2 = 5);
inv = rcp(s) (5 + 2 = 7); mi = m_j inv (8).
  acceleration term mi d_k: 8 + 1 = 9                                                                         -> K = 10
  jerk term mi (w_k + beta d_k), beta = (d.w)(-2 inv): d.w is a multiply and two FMAs on products of rounded d, w -- (3 + 2) of
  sum_l |d_l w_l|, which is why the magnitude below carries that sum and not |d.w| --, -2 inv is exact, beta one multiply
  (5 + 7 + 1 = 13), beta d_k 14, the FMA that forms w_k + beta d_k one more on both parts (15; the w_k part: 1 + 1 = 2), times mi
  (8): 23 on the d part, 10 on the w part                                                                     -> K = 24
The accumulating FMAs round the running sums: that is the n."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = float(np.float32(0.0001))
KEYS = ("px", "py", "pz", "vx", "vy", "vz", "m")
K_ACC, K_JERK = 10, 24


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


def _lattice(n, seed, planar=False):
    """jittered lattice: spacing 2, jitter +-0.5 per axis (separations >= 1), masses in [0.5, 2), velocities in [-1, 1)"""
    rng = np.random.default_rng(seed)
    dim = 2 if planar else 3
    side = int(math.ceil(n ** (1.0 / dim)))
    cells = np.stack(np.unravel_index(np.arange(n), (side,) * dim), 1)
    P, V = np.zeros((n, 3)), np.zeros((n, 3))
    P[:, :dim] = 2.0 * cells + rng.uniform(-0.5, 0.5, (n, dim))
    V[:, :dim] = rng.uniform(-1.0, 1.0, (n, dim))
    return {k: np.asarray(c, np.float32) for k, c in zip(KEYS, (*P.T, *V.T, rng.uniform(0.5, 2.0, n)))}


def _engine(rx, st, planar=False, **kw):
    e = rx.NBodyEngine(**kw)
    e.set_particles(*(st[k] for k in ("px", "py", "vx", "vy", "m")), **({} if planar else {"pz": st["pz"], "vz": st["vz"]}))
    return e


def _state64(st):
    c = [np.asarray(st[k], np.float64) for k in KEYS]
    return np.stack(c[0:3], 1), np.stack(c[3:6], 1), c[6]


def _terms(P, V, m, i):
    """the pair terms of body i, [n, 6], and the magnitudes the bound charges them with"""
    d, w = P - P[i], V - V[i]
    s = ((d * d).sum(1) + EPS)[:, None]
    mj = m[:, None]
    dw, dw_abs = (d * w).sum(1)[:, None], np.abs(d * w).sum(1)[:, None]
    terms = np.hstack([mj * d / s, mj * (w / s - 2.0 * dw * d / s ** 2)])
    return terms, np.hstack([np.abs(mj * d / s), mj * (np.abs(w) / s + 2.0 * dw_abs * np.abs(d) / s ** 2)])


def _acc_jerk64(P, V, m):
    return np.stack([_terms(P, V, m, i)[0].sum(0) for i in range(len(m))]).reshape(-1, 2, 3).transpose(1, 0, 2)


def _hermite64(P, V, m, dt, steps, aj=None):
    a0, j0 = _acc_jerk64(P, V, m) if aj is None else aj
    for _ in range(steps):
        Pp = P + V * dt + a0 * (dt * dt / 2) + j0 * (dt ** 3 / 6)
        Vp = V + a0 * dt + j0 * (dt * dt / 2)
        a1, j1 = _acc_jerk64(Pp, Vp, m)
        V1 = V + (a0 + a1) * (dt / 2) + (j0 - j1) * (dt * dt / 12)
        P = P + (V + V1) * (dt / 2) + (a0 - a1) * (dt * dt / 12)
        V, a0, j0 = V1, a1, j1
    return P, V, (a0, j0)


CASES = {
    "one": lambda rx: _sphere(rx, 1, 1),                        # all zeros
    "two": lambda rx: _sphere(rx, 2, 2),
    "wave+1": lambda rx: _sphere(rx, 65, 3),
    "block+1": lambda rx: _sphere(rx, 257, 4),                  # one target past whole workgroups (64 T targets each, T = 1, 2 or 4)
    "split3": lambda rx: _sphere(rx, 1100, 6),                  # five source tiles in three ranges: a short first one
    "coincident": _coincident,                                  # 200 bodies + 4 at one position: jerk m w / eps, finite
    "galaxies": lambda rx: rx.two_galaxies(515),                # planar: the DIM = 2 sweep; mass ratio 1000
}


@functools.lru_cache(maxsize=None)
def _exact(rx, name):
    st = CASES[name](rx)
    P, V, m = _state64(st)
    val, mag = np.zeros((len(m), 6)), np.zeros((len(m), 6))
    for i in range(len(m)):
        t, a = _terms(P, V, m, i)
        val[i], mag[i] = [math.fsum(c) for c in t.T], a.sum(0)
    return st, val, mag


@pytest.mark.parametrize("name", list(CASES))
def test_acc_jerk_within_the_summation_bound(rx, name):
    st, val, mag = _exact(rx, name)
    n = len(st["m"])
    planar = name == "galaxies"
    e = _engine(rx, st, planar)
    if name == "split3":
        e.set_launch(jsplit=3)
    before = e.get_particles()
    got = np.stack(e.acc_jerk(), 1)
    ll = e.last_launch()
    assert ll["variant"] == 40 and ll["block"] == 256 and ll["dim"] == (2 if planar else 3), ll
    assert name != "split3" or ll["jsplit"] == 3, ll
    bound = (n + np.repeat([K_ACC, K_JERK], 3)) * U * mag
    err = np.abs(got - val)
    print(f"{name}: worst error / bound per component = {(err / np.maximum(bound, 1e-300)).max(0)}")
    assert np.all(err <= bound), name
    assert np.array_equal(got.view(np.uint32), np.stack(e.acc_jerk(), 1).view(np.uint32))
    after = e.get_particles()
    assert all(np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)) for k in KEYS)


def _run(rx, st, planar, dt, restart):
    e = _engine(rx, st, planar)
    for k in range(4):
        if restart and k == 2:
            e.step_brute_force(dt)
        e.step_hermite(dt)
    return e.get_particles()


@pytest.mark.parametrize("n,planar,restart", [(2, False, False), (65, False, False), (321, False, False), (321, True, False),
                                              (65, False, True)])
def test_step_hermite_follows_the_scheme_in_float64(rx, n, planar, restart):
    """restart: a kick-drift step between the Hermite steps invalidates the kept (a0, j0); the reference re-evaluates them"""
    dt = 1.0 / 16
    st = _lattice(n, 7 + n, planar)
    P, V, m = _state64(st)
    aj = _acc_jerk64(P, V, m)
    ptol, vtol = rx.fast_step_tolerances(float(np.sqrt((aj[0] ** 2).sum(1)).max()), n, dt, 4)
    if restart:
        P, V, _ = _hermite64(P, V, m, dt, 2, aj)
        V = V + dt * _acc_jerk64(P, V, m)[0]
        P = P + dt * V
        P, V, _ = _hermite64(P, V, m, dt, 2)
        p1, v1 = rx.fast_step_tolerances(float(np.sqrt((aj[0] ** 2).sum(1)).max()), n, dt, 1)
        ptol, vtol = ptol + p1, vtol + v1
    else:
        P, V, _ = _hermite64(P, V, m, dt, 4, aj)
    got = _run(rx, st, planar, dt, restart)
    dp = np.abs(np.stack([got[k] for k in KEYS[0:3]], 1) - P).max()
    dv = np.abs(np.stack([got[k] for k in KEYS[3:6]], 1) - V).max()
    print(f"n={n} planar={planar} restart={restart}: |dp| = {dp:.3g} (tol {ptol:.3g}), |dv| = {dv:.3g} (tol {vtol:.3g})")
    assert dp <= ptol and dv <= vtol
    again = _run(rx, st, planar, dt, restart)
    assert all(np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)) for k in KEYS)


@pytest.mark.parametrize("n", [65, 1100])
def test_timestep_is_eta_times_the_smallest_ratio(rx, n):
    """Roundings of the device's value: two sums of three squares (3 each), their quotient (1), its square root (halves what came
    before, adds 1: 4.5), the multiply by eta (1): 5.5 -- and the float64 minimum may fall on another body, whose ratio is then
    within the same distance.  Held to the 16 * 2^-24 the interface states."""
    e = _engine(rx, _sphere(rx, n, 8))
    eta = float(np.float32(0.02))
    aj = np.stack(e.acc_jerk(), 1).astype(np.float64)
    want = eta * (np.sqrt((aj[:, 0:3] ** 2).sum(1)) / np.sqrt((aj[:, 3:6] ** 2).sum(1))).min()
    got = e.hermite_timestep(eta)
    print(f"n={n}: relative difference {abs(got - want) / want / U:.2f} * 2^-24")
    assert abs(got - want) <= 16 * U * want


@pytest.mark.parametrize("what", ["shard", "group", "strict", "fp16"])
def test_refusals_leave_the_state_alone(rx, monkeypatch, what):
    from rust_exp_amd.engine import NBX_ERR_STATE

    st = _sphere(rx, 65, 9)
    args = [st[k] for k in ("px", "py", "vx", "vy", "m")]
    if what == "group":
        monkeypatch.setenv("NBX_GROUP_EXCHANGE", "copy")   # (two members on one device: peer copies, no communicator)
        g = rx.NBodyGroup([0, 0])
        g.set_particles(*args, pz=st["pz"], vz=st["vz"])
        e, state = g.engine(0), g.get_particles
    else:
        e = rx.NBodyEngine(mode="strict" if what == "strict" else "fast")
        if what == "shard":
            e.set_shard(0, 2)
        if what == "fp16":
            e.set_source_precision(16)
        e.set_particles(*args, pz=st["pz"], vz=st["vz"])
        state = e.get_particles
    for call in (lambda: e.step_hermite(0.01), e.acc_jerk, lambda: e.hermite_timestep(0.02)):
        with pytest.raises(rx.NBodyError) as err:
            call()
        assert err.value.code == NBX_ERR_STATE
    after = state()
    assert all(np.array_equal(st[k].view(np.uint32), after[k].view(np.uint32)) for k in KEYS)
