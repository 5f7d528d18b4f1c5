"""Hermite block time steps (K9, hermite_block.hip): nbx_acc_jerk_subset against the full sweep's rows, nbx_step_hermite_block
against the shared step and against the block scheme restated in numpy float64 (_block64: integer ticks, per-body prediction, the
same level table), the level criterion, and a system -- a tight binary among slow bodies -- where individual steps pay.  Cases,
states and the float64 pair sums are those of test_gpu_hermite.py."""
import numpy as np
import pytest

from test_gpu_hermite import K_ACC, K_JERK, KEYS, U, _acc_jerk64, _engine, _exact, _lattice, _sphere, _state64

pytestmark = pytest.mark.gpu

TICKS, MAX_LEVEL = 1 << 20, 20
DT = 1.0 / 16


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_state(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in KEYS)


def _ratio(a, j):
    ja = np.sqrt((j ** 2).sum(1))
    return np.where(ja > 0, np.sqrt((a ** 2).sum(1)) / np.where(ja > 0, ja, 1.0), np.inf)


def _block64(P, V, m, dt_max, levels, macro_steps, eta=0.0):
    """The block scheme in float64.  levels=None: from eta |a| / |j| of the first evaluation; eta > 0: the update rule of
    k_block_correct.  Returns P, V, levels, block steps and evaluations of the last macro-step."""
    P, V = P.copy(), V.copy()
    a0, j0 = _acc_jerk64(P, V, m)
    dts = dt_max * 2.0 ** -np.arange(MAX_LEVEL + 1)
    if levels is None:
        levels = np.minimum(np.ceil(np.log2(np.maximum(dt_max / (eta * _ratio(a0, j0)), 1.0))), MAX_LEVEL)
    levels = np.array(levels, np.int64)
    for _ in range(macro_steps):
        t, blocks, evals = np.zeros(len(m), np.int64), 0, 0
        while t.min() < TICKS:
            tn = (t + (TICKS >> levels)).min()
            due = t + (TICKS >> levels) == tn
            h = ((tn - t) * (dt_max / TICKS))[:, None]
            a1, j1 = _acc_jerk64(P + V * h + a0 * (h * h / 2) + j0 * (h ** 3 / 6), V + a0 * h + j0 * (h * h / 2), m)
            d, a1, j1 = h[due], a1[due], j1[due]
            V1 = V[due] + (a0[due] + a1) * (d / 2) + (j0[due] - j1) * (d * d / 12)
            P[due] += (V[due] + V1) * (d / 2) + (a0[due] - a1) * (d * d / 12)
            V[due], a0[due], j0[due], t[due] = V1, a1, j1, tn
            if eta > 0:
                lv, req = levels[due], eta * _ratio(a1, j1)
                deeper = np.array([next(k for k in range(l, MAX_LEVEL + 1) if dts[k] <= r or k == MAX_LEVEL) for l, r in zip(lv, req)])
                up = (deeper == lv) & (lv > 0) & (dts[np.maximum(lv - 1, 0)] <= req) & (tn % (2 * (TICKS >> lv)) == 0)
                levels[due] = deeper - up
            blocks, evals = blocks + 1, evals + int(due.sum())
    return P, V, levels, blocks, evals


@pytest.mark.parametrize("name,jsplit,count", [(nm, 3, c) for nm in ("split3", "galaxies") for c in (1, 64, 65, 129, 300, 0)]
                         + [("split3", 0, 1), ("split3", 0, 129)])
def test_subset_sweep_gives_the_full_sweeps_rows(rx, name, jsplit, count):
    """count 0 = every body, shuffled: the T = 2 kernel behind a gather (lists below n take T = 1).  jsplit 3: bit for bit.  jsplit 0
    (the split of each call sized by its own number of targets): the summation bound of test_gpu_hermite.py against exact sums."""
    st, val, mag = _exact(rx, name)
    n, planar = len(st["m"]), name == "galaxies"
    e = _engine(rx, st, planar)
    e.set_launch(jsplit=jsplit)
    idx = np.random.default_rng(count).permutation(n)[:count or n]
    before = e.get_particles()
    full = np.stack(e.acc_jerk(), 1)
    kept = np.stack(e.hermite_kept(), 1)
    got = np.stack(e.acc_jerk_subset(idx), 1)
    ll = e.last_launch()
    assert ll["variant"] == 41 and ll["block"] == 256 and ll["dim"] == (2 if planar else 3), ll
    assert ll["bodies_per_thread"] == (1 if count else 2), ll
    if jsplit:
        assert ll["jsplit"] == jsplit and np.array_equal(_bits(got), _bits(full[idx]))
    else:
        bound = (n + np.repeat([K_ACC, K_JERK], 3)) * U * mag[idx]
        err = np.abs(got - val[idx])
        print(f"{name} count={count} S={ll['jsplit']}: worst error / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}")
        assert np.all(err <= bound)
    assert _same_state(before, e.get_particles()) and np.array_equal(_bits(kept), _bits(np.stack(e.hermite_kept(), 1)))


@pytest.mark.parametrize("n", [65, 321])
def test_all_levels_zero_frozen_is_the_shared_step(rx, n):
    from rust_exp_amd.engine import NBX_STAT_HERMITE_BLOCK_EVALS, NBX_STAT_HERMITE_BLOCK_STEPS

    st = _lattice(n, 7 + n)
    shared, block = _engine(rx, st), _engine(rx, st)
    for _ in range(3):
        shared.step_hermite(DT)
        block.step_hermite_block(DT, 0.0)
        assert (block.get_stat(NBX_STAT_HERMITE_BLOCK_STEPS), block.get_stat(NBX_STAT_HERMITE_BLOCK_EVALS)) == (1, n)
    assert block.last_launch()["variant"] == 41
    assert _same_state(shared.get_particles(), block.get_particles())
    assert np.array_equal(_bits(np.stack(shared.hermite_kept())), _bits(np.stack(block.hermite_kept())))
    assert not block.hermite_block_levels().any()


def _prescribed(rx, st, planar, levels):
    e = _engine(rx, st, planar)
    e.set_hermite_block_levels(levels)
    for _ in range(2):
        e.step_hermite_block(DT, 0.0)
    return e


@pytest.mark.parametrize("n,planar,levels", [(2, False, [0, 2]), (65, False, np.arange(65) % 4),
                                             (321, True, np.random.default_rng(11).integers(0, 4, 321))])
def test_prescribed_levels_follow_the_scheme_in_float64(rx, n, planar, levels):
    from rust_exp_amd.engine import NBX_STAT_HERMITE_BLOCK_EVALS, NBX_STAT_HERMITE_BLOCK_STEPS

    st = _lattice(n, 7 + n, planar)
    P, V, m = _state64(st)
    amax = float(np.sqrt((_acc_jerk64(P, V, m)[0] ** 2).sum(1)).max())
    ptol, vtol = rx.fast_step_tolerances(amax, n, DT, 2 * 2 ** int(np.max(levels)))
    P, V, _, blocks, evals = _block64(P, V, m, DT, levels, 2)
    e = _prescribed(rx, st, planar, levels)
    got = e.get_particles()
    dp = np.abs(np.stack([got[k] for k in KEYS[0:3]], 1) - P).max()
    dv = np.abs(np.stack([got[k] for k in KEYS[3:6]], 1) - V).max()
    print(f"n={n} planar={planar}: |dp| = {dp:.3g} (tol {ptol:.3g}), |dv| = {dv:.3g} (tol {vtol:.3g}), {blocks} block steps, {evals} evaluations")
    assert dp <= ptol and dv <= vtol
    assert (e.get_stat(NBX_STAT_HERMITE_BLOCK_STEPS), e.get_stat(NBX_STAT_HERMITE_BLOCK_EVALS)) == (blocks, evals)
    assert np.array_equal(e.hermite_block_levels(), levels)
    assert _same_state(got, _prescribed(rx, st, planar, levels).get_particles())


@pytest.mark.parametrize("n", [65, 1100])
def test_levels_satisfy_the_criterion(rx, n):
    """From the device's own kept pair after the call: dt(level) <= eta |a| / |j| within the 16 * 2^-24 nbx_hermite_timestep states,
    and no more than one level deeper than that asks for (a body doubles its step once per update at most)."""
    e = _engine(rx, _sphere(rx, n, 8))
    eta, dt_max = float(np.float32(0.02)), float(np.float32(1e-6))
    e.step_hermite_block(dt_max, eta)
    aj = np.stack(e.hermite_kept(), 1).astype(np.float64)
    lv = e.hermite_block_levels().astype(np.int64)
    req, dt = eta * _ratio(aj[:, 0:3], aj[:, 3:6]), dt_max * 2.0 ** -lv
    print(f"n={n}: levels {np.bincount(lv)}, smallest eta |a| / |j| = {req.min():.3g}")
    assert np.all((dt <= req * (1 + 16 * U)) | (lv == MAX_LEVEL))
    assert np.all((lv <= 1) | (4 * dt > req * (1 - 16 * U)))


def _binary_among_slow_bodies():
    """63 lattice bodies + two unit masses 0.05 apart on the circular orbit of the 1/r law (period 0.23), well outside the lattice"""
    st = {k: np.append(c, [0, 0]).astype(np.float32) for k, c in _lattice(63, 70).items()}
    sep, eps = 0.05, 1e-4
    v = 0.5 * np.sqrt(2.0 * sep * sep / (sep * sep + eps))   # relative speed^2 = relative acceleration * separation
    st["px"][-2:], st["py"][-2:], st["pz"][-2:] = (-4 - sep / 2, -4 + sep / 2), -4, -4
    st["vy"][-2:], st["m"][-2:] = (-v, v), 1
    return st


def test_block_steps_pay_for_a_tight_binary(rx):
    """In float64 (_block64 with eta, _hermite64) the block scheme's |dE/E| on this input is 8.8e-8 and the shared step's 1.1e-3: the
    first assertion does not hang on fp32 noise."""
    from rust_exp_amd.engine import NBX_STAT_HERMITE_BLOCK_EVALS

    st = _binary_among_slow_bodies()
    n, eta = len(st["m"]), float(np.float32(0.02))
    shared, block = _engine(rx, st), _engine(rx, st)
    energy = lambda e: sum(e.conserved()[k] for k in ("kinetic", "potential"))
    e0, evals = energy(shared), 0
    for _ in range(5):
        shared.step_hermite(DT)
        block.step_hermite_block(DT, eta)
        evals += block.get_stat(NBX_STAT_HERMITE_BLOCK_EVALS)
    lv = block.hermite_block_levels()
    err_shared, err_block = abs(energy(shared) / e0 - 1), abs(energy(block) / e0 - 1)
    print(f"|dE/E| block {err_block:.3g}, shared {err_shared:.3g}; levels {np.bincount(lv)}, binary at {lv[-2:]}; {evals} evaluations")
    assert err_block < err_shared
    assert lv[-2:].min() > np.median(lv)
    assert evals < n * 2 ** int(lv.max()) * 5


@pytest.mark.parametrize("what", ["shard", "group", "strict", "fp16", "arguments"])
def test_refusals_leave_the_state_alone(rx, monkeypatch, what):
    from rust_exp_amd.engine import NBX_ERR_INVALID, NBX_ERR_STATE

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
    calls = [lambda: e.step_hermite_block(0.01, 0.02), lambda: e.set_hermite_block_levels(np.zeros(65)), lambda: e.acc_jerk_subset([3])]
    if what == "arguments":
        calls = [lambda: e.set_hermite_block_levels(np.full(65, 21)), lambda: e.acc_jerk_subset([0, 65]), lambda: e.step_hermite_block(0.0, 0.02)]
    for call in calls:
        with pytest.raises(rx.NBodyError) as err:
            call()
        assert err.value.code == (NBX_ERR_INVALID if what == "arguments" else NBX_ERR_STATE)
    assert _same_state(st, state())
