"""nbx_acc_jerk_f64 (K12, acc_jerk64.hip) against its pair terms in numpy longdouble, each converted to float and summed exactly
(math.fsum):
    law 0   a_i = sum_j m_j d / s,        j_i = sum_j m_j (w / s - 2 (d.w) d / s^2)
    law 1   a_i = sum_j m_j d s^(-3/2),   j_i = sum_j m_j (w s^(-3/2) - 3 (d.w) d s^(-5/2)),   d = p_j - p_i, w = v_j - v_i, s = |d|^2 + eps
Bound per component: (n + K + 1) * 2^-53 * sum_j |term|, the jerk's d-part charged with sum_l |d_l w_l| as in test_gpu_hermite._terms.
n: the summation of n terms in any order; + 1: the reference term's conversion to double.  K: the roundings that reach one term,
counted from the loop's instructions by the rules of test_gpu_hermite.py / test_gpu_newton.py (one per rounding, a refined v_rcp_f64
/ v_rsq_f64 charged 2, a square root halves its argument's relative error, an accumulating FMA's product is not rounded; one more
on top of the count, as there).
Law 0, the instruction order of K8: d_k, w_k 1 each; s 5; inv 7; mi = m_j inv 8; acceleration term mi d_k 9      -> K = 10
  beta = (d.w)(-2 inv): 5 + 7 + 1 = 13; beta d_k 14; u_k = w_k + beta d_k 15 (w part 2); times mi: 23            -> K = 24
Law 1: u = rsq(s): 5 / 2 + 2 = 4.5; u2 = u u 10; m_j u 5.5; mi = (m_j u) u2 16.5; acceleration term mi d_k 17.5   -> K = 19
  -3 u2 is a rounded product: 11; beta = (d.w)(-3 u2): 5 + 11 + 1 = 17; beta d_k 18; u_k 19 (w part 2); times mi: 35.5 -> K = 37"""
import functools
import math

import numpy as np
import pytest

from test_gpu_hermite import EPS, KEYS, _coincident, _engine, _sphere

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -53
K = {0: np.repeat([10, 24], 3), 1: np.repeat([19, 37], 3)}
CASES = {
    "one": lambda rx: _sphere(rx, 1, 1),
    "two": lambda rx: _sphere(rx, 2, 2),
    "wave+1": lambda rx: _sphere(rx, 65, 3),
    "block+1": lambda rx: _sphere(rx, 257, 4),
    "block64+1": lambda rx: _sphere(rx, 769, 4),               # 64 T k + 1 targets for T = 1, 2, 4
    "coincident": _coincident,                                 # 200 bodies + 4 at one position: finite jerk, zero acceleration
    "galaxies": lambda rx: rx.two_galaxies(515),               # planar: all z = 0 through the 3-D loop; mass ratio 1000
    "split3": lambda rx: _sphere(rx, 1100, 6),                 # NBX_OPT_JSPLIT = 3: 1100 sources in ranges of 367, 367, 366
}


@functools.lru_cache(maxsize=None)
def _exact(rx, name, law):
    """the state; the exact sums [n, 6]; the magnitudes the bound charges them with"""
    st = CASES[name](rx)
    P, V = (np.stack([np.asarray(st[k], np.longdouble) for k in keys], 1) for keys in (KEYS[0:3], KEYS[3:6]))
    mj = np.asarray(st["m"], np.longdouble)[:, None]
    val, mag = np.zeros((len(mj), 6)), np.zeros((len(mj), 6))
    for i in range(len(mj)):
        d, w = P - P[i], V - V[i]
        s = ((d * d).sum(1) + np.longdouble(EPS))[:, None]
        f, g = (1 / s, 2 / s ** 2) if law == 0 else (1 / (s * np.sqrt(s)), 3 / (s * s * np.sqrt(s)))
        dw, dw_abs = (d * w).sum(1)[:, None], np.abs(d * w).sum(1)[:, None]
        terms = np.hstack([mj * d * f, mj * (w * f - g * dw * d)]).astype(np.float64)
        val[i] = [math.fsum(c) for c in terms.T]
        mag[i] = np.hstack([np.abs(mj * d * f), mj * (np.abs(w) * f + g * dw_abs * np.abs(d))]).astype(np.float64).sum(0)
    return st, val, mag


def _law_engine(rx, name, law, **kw):
    e = _engine(rx, CASES[name](rx), name == "galaxies", **kw)
    e.set_law(("reference", "newton")[law])
    return e


@pytest.mark.parametrize("law", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_within_the_summation_bound(rx, name, law):
    st, val, mag = _exact(rx, name, law)
    n = len(st["m"])
    e = _law_engine(rx, name, law)
    if name == "split3":
        e.set_launch(jsplit=3)
    got = np.stack(e.acc_jerk_f64(), 1)
    ll = e.last_launch()
    assert ll["variant"] == 66 + law and ll["block"] == 256 and ll["jsplit"] == (3 if name == "split3" else max(ll["jsplit"], 1)), ll
    bound = (n + K[law] + 1) * U64 * mag
    err = np.abs(got - val)
    print(f"{name} law {law}: worst error / bound per component = {(err / np.maximum(bound, 1e-300)).max(0)}")
    assert np.all(err <= bound), name


@pytest.mark.parametrize("law", [0, 1])
def test_listed_rows_are_the_full_rows_bit_for_bit(rx, law):
    e = _law_engine(rx, "split3", law)
    e.set_launch(jsplit=3)
    full = np.stack(e.acc_jerk_f64(), 1)
    rng = np.random.default_rng(11)
    some = rng.permutation(1100)[:65]
    some[64] = some[5]
    for idx in ([7], some, rng.permutation(1100)):
        got = np.stack(e.acc_jerk_f64(idx), 1)
        assert e.last_launch()["jsplit"] == 3
        assert np.array_equal(got.view(np.uint64), full[np.asarray(idx)].view(np.uint64)), len(idx)
    e.set_launch(jsplit=3, bodies_per_thread=4)   # (T = 2 above, T = 1 for the short lists: the order of summation knows no T)
    assert np.array_equal(np.stack(e.acc_jerk_f64(), 1).view(np.uint64), full.view(np.uint64))
    assert e.last_launch()["bodies_per_thread"] == 4


def test_it_arbitrates_the_fp32_sweep_and_agrees_with_the_fp64_forces(rx):
    st, _, mag = _exact(rx, "split3", 0)
    e = _law_engine(rx, "split3", 0)
    err = np.abs(np.stack(e.acc_jerk(), 1).astype(np.float64) - np.stack(e.acc_jerk_f64(), 1))
    assert np.all(err <= (1100 + K[0]) * 2.0 ** -24 * mag)
    st, _, mag = _exact(rx, "block+1", 1)
    e = _law_engine(rx, "block+1", 1)
    m = st["m"].astype(np.float64)[:, None]
    err = np.abs(m * np.stack(e.acc_jerk_f64()[0:3], 1) - np.stack(e.forces_f64(potential=False)[0:3], 1))
    assert np.all(err <= (257 + 20 + K[1][0:3]) * U64 * m * mag[:, 0:3])


@pytest.mark.parametrize("block", [False, True])
def test_an_integrator_continues_as_if_it_had_not_been_called(rx, block):
    def run(probe):
        e = _law_engine(rx, "block+1", 0)
        if block:
            e.set_hermite_block_train(4)
        step = (lambda: e.step_hermite_block(0.01, 0.02)) if block else (lambda: e.step_hermite(0.01))
        step()
        if probe:
            before = [a.tobytes() for a in (*e.get_particles().values(), *e.hermite_kept())]
            e.acc_jerk_f64()
            e.acc_jerk_f64([3, 200])
            assert before == [a.tobytes() for a in (*e.get_particles().values(), *e.hermite_kept())]
        step()
        return [a.tobytes() for a in e.get_particles().values()]

    assert run(True) == run(False)


@pytest.mark.parametrize("what", ["shard", "group", "strict", "fp16"])
def test_refusals_leave_the_state_alone(rx, monkeypatch, what):
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
        if what in ("strict", "fp16"):
            e.set_law("newton")
        state = e.get_particles
    for idx in (None, [3]):
        with pytest.raises(rx.NBodyError) as err:
            e.acc_jerk_f64(idx)
        assert err.value.code == rx.NBX_ERR_STATE
    after = state()
    assert all(np.array_equal(st[k].view(np.uint32), after[k].view(np.uint32)) for k in KEYS)


def test_an_index_of_n_and_a_short_capacity_are_invalid(rx):
    e = _law_engine(rx, "wave+1", 0)
    with pytest.raises(rx.NBodyError) as err:
        e.acc_jerk_f64([0, 65])
    assert err.value.code == rx.NBX_ERR_INVALID
    assert rx.lib().nbx_acc_jerk_f64(e._h, None, 64, *[None] * 6) == rx.NBX_ERR_INVALID
    assert len(e.acc_jerk_f64([])) == 6 and e.acc_jerk_f64([64, 64])[0].shape == (2,)
