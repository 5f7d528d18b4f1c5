"""Hermite block steps for small blocks, in trains (K10, hermite_train.hip, NBX_OPT_HERMITE_BLOCK_TRAIN): the lane-split sweep behind
nbx_acc_jerk_subset against exact sums, its independence of what else is listed, and nbx_step_hermite_block with the train on against
the float64 restatement of test_gpu_hermite_block.py.  Cases, states, bounds and the restatement are those of the two modules below.

Measured (docs/rounds/r11.md): the sweep's worst error is 0.011 of the bound; the prescribed-level runs land 14 - 1 800 times below the
tolerance; the tight binary's |dE/E| is 7.0e-8 with the train on (K9: 6.9e-8, shared step: 1.0e-3)."""
import numpy as np
import pytest

from test_gpu_hermite import K_ACC, K_JERK, KEYS, U, _acc_jerk64, _engine, _exact, _lattice, _state64
from test_gpu_hermite_block import DT, TICKS, _binary_among_slow_bodies, _bits, _block64, _same_state

pytestmark = pytest.mark.gpu

SMALL = 64   # kTrainMaxBlock
CASES = [(nm, js) for nm in ("split3", "galaxies") for js in (0, 3)]


def _train_engine(rx, st, planar, jsplit=0, length=16):
    e = _engine(rx, st, planar)
    e.set_launch(jsplit=jsplit)
    e.set_hermite_block_train(length)
    return e


@pytest.mark.parametrize("count", [1, 63, 64, 65])
@pytest.mark.parametrize("name,jsplit", CASES)
def test_small_list_sweep_within_the_summation_bound(rx, name, jsplit, count):
    st, val, mag = _exact(rx, name)
    n, planar = len(st["m"]), name == "galaxies"
    e = _train_engine(rx, st, planar, jsplit)
    idx = np.random.default_rng(count).permutation(n)[:count]
    before = e.get_particles()
    e.acc_jerk()
    kept = np.stack(e.hermite_kept(), 1)
    got = np.stack(e.acc_jerk_subset(idx), 1)
    ll = e.last_launch()
    assert ll["block"] == 256 and ll["bodies_per_thread"] == 1 and ll["dim"] == (2 if planar else 3), ll
    if count <= SMALL:
        assert ll["variant"] == 42 and ll["jsplit"] == ll["grid"] == (jsplit or -(-n // 256)), ll
        bound = (n + np.repeat([K_ACC, K_JERK], 3)) * U * mag[idx]
        err = np.abs(got - val[idx])
        print(f"{name} count={count} G={ll['jsplit']}: worst error / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}")
        assert np.all(err <= bound)
    else:
        assert ll["variant"] == 41, ll
        off = _engine(rx, st, planar)
        off.set_launch(jsplit=jsplit)
        assert np.array_equal(_bits(got), _bits(np.stack(off.acc_jerk_subset(idx), 1)))
    assert _same_state(before, e.get_particles()) and np.array_equal(_bits(kept), _bits(np.stack(e.hermite_kept(), 1)))


@pytest.mark.parametrize("name,jsplit", CASES)
def test_a_row_does_not_depend_on_the_rest_of_the_block(rx, name, jsplit):
    st = _exact(rx, name)[0]
    e = _train_engine(rx, st, name == "galaxies", jsplit)
    idx = np.random.default_rng(5).permutation(len(st["m"]))[:SMALL]
    rows = np.stack(e.acc_jerk_subset(idx), 1)
    for slot in (0, 7, 8, 37, 63):   # first and last of a chunk of 8 targets, of the list
        alone = np.stack(e.acc_jerk_subset(idx[slot:slot + 1]), 1)
        assert e.last_launch()["variant"] == 42
        assert np.array_equal(_bits(alone[0]), _bits(rows[slot])), slot


def _block_sizes(levels):
    """the blocks of one macro-step under frozen levels, in time order"""
    steps = TICKS >> np.asarray(levels, np.int64)
    times = np.unique(np.concatenate([np.arange(s, TICKS + 1, s) for s in np.unique(steps)]))
    return np.array([(t % steps == 0).sum() for t in times])


def _prescribed(rx, st, planar, levels, length):
    e = _train_engine(rx, st, planar, length=length)
    e.set_hermite_block_levels(levels)
    for _ in range(2):
        e.step_hermite_block(DT, 0.0)
    return e


@pytest.mark.parametrize("n,planar,levels", [(2, False, [0, 2]), (65, False, np.arange(65) % 4), (129, False, np.arange(129) < 64),
                                             (130, False, np.arange(130) < 65),
                                             (321, True, np.random.default_rng(11).integers(0, 4, 321))])
def test_prescribed_levels_follow_the_scheme_in_float64(rx, n, planar, levels):
    from rust_exp_amd.engine import (NBX_STAT_HERMITE_BLOCK_EVALS, NBX_STAT_HERMITE_BLOCK_READS, NBX_STAT_HERMITE_BLOCK_STEPS,
                                     NBX_STAT_HERMITE_BLOCK_TRAIN_STEPS)

    levels = np.asarray(levels, np.int32)
    st = _lattice(n, 7 + n, planar)
    P, V, m = _state64(st)
    amax = float(np.sqrt((_acc_jerk64(P, V, m)[0] ** 2).sum(1)).max())
    ptol, vtol = rx.fast_step_tolerances(amax, n, DT, 2 * 2 ** int(np.max(levels)))
    P, V, _, blocks, evals = _block64(P, V, m, DT, levels, 2)
    sizes = _block_sizes(levels)
    small = int((sizes <= SMALL).sum())
    assert (len(sizes), int(sizes.sum())) == (blocks, evals)
    e = _prescribed(rx, st, planar, levels, 16)
    got = e.get_particles()
    dp = np.abs(np.stack([got[k] for k in KEYS[0:3]], 1) - P).max()
    dv = np.abs(np.stack([got[k] for k in KEYS[3:6]], 1) - V).max()
    stats = [e.get_stat(s) for s in (NBX_STAT_HERMITE_BLOCK_STEPS, NBX_STAT_HERMITE_BLOCK_EVALS, NBX_STAT_HERMITE_BLOCK_TRAIN_STEPS,
                                     NBX_STAT_HERMITE_BLOCK_READS)]
    print(f"n={n} planar={planar}: |dp| = {dp:.3g} (tol {ptol:.3g}), |dv| = {dv:.3g} (tol {vtol:.3g}), blocks {sizes}, "
          f"steps / evaluations / train steps / reads = {stats}")
    assert dp <= ptol and dv <= vtol
    assert stats[:3] == [blocks, evals, small]
    if small:
        assert stats[3] < blocks
    if n == 65:
        assert stats[3] <= 2
    assert np.array_equal(e.hermite_block_levels(), levels)
    assert _same_state(got, _prescribed(rx, st, planar, levels, 16).get_particles())
    if not small:
        assert _same_state(got, _prescribed(rx, st, planar, levels, 0).get_particles())


def test_trains_pay_for_a_tight_binary(rx):
    from rust_exp_amd.engine import NBX_STAT_HERMITE_BLOCK_READS, NBX_STAT_HERMITE_BLOCK_STEPS, NBX_STAT_HERMITE_BLOCK_TRAIN_STEPS

    st = _binary_among_slow_bodies()
    eta = float(np.float32(0.02))
    shared, train = _engine(rx, st), _train_engine(rx, st, False)
    energy = lambda e: sum(e.conserved()[k] for k in ("kinetic", "potential"))
    e0, total = energy(shared), np.zeros(3, np.int64)
    for _ in range(5):
        shared.step_hermite(DT)
        train.step_hermite_block(DT, eta)
        total += [train.get_stat(s) for s in (NBX_STAT_HERMITE_BLOCK_STEPS, NBX_STAT_HERMITE_BLOCK_TRAIN_STEPS, NBX_STAT_HERMITE_BLOCK_READS)]
    lv = train.hermite_block_levels()
    err_shared, err_train = abs(energy(shared) / e0 - 1), abs(energy(train) / e0 - 1)
    print(f"|dE/E| train {err_train:.3g}, shared {err_shared:.3g}; levels {np.bincount(lv)}, binary at {lv[-2:]}; "
          f"steps / train steps / reads = {total}")
    assert err_train < err_shared
    assert lv[-2:].min() > np.median(lv)
    assert 2 * total[1] > total[0] and 4 * total[2] <= total[0]
