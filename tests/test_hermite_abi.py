"""nbx_step_hermite / nbx_acc_jerk / nbx_hermite_timestep without a GPU: symbols, wrappers and statuses."""
import numpy as np
import pytest


def test_symbols_and_wrappers_exist(rx):
    L = rx.lib()
    assert L.nbx_step_hermite and L.nbx_acc_jerk and L.nbx_hermite_timestep
    assert all(callable(getattr(rx.NBodyEngine, k)) for k in ("step_hermite", "acc_jerk", "hermite_timestep"))


def test_statuses_with_and_without_a_device(rx):
    from rust_exp_amd.engine import NBX_ERR_NO_DEVICE, NBX_ERR_STATE

    e = rx.NBodyEngine(mode="strict")   # (a configuration the step refuses: without a device that is not looked at)
    one = np.ones(8, np.float32)
    e.set_particles(np.arange(8), one, one, one, one)
    code = NBX_ERR_NO_DEVICE if rx.device_count() == 0 else NBX_ERR_STATE
    for call in (lambda: e.step_hermite(0.01), e.acc_jerk, lambda: e.hermite_timestep(0.02)):
        with pytest.raises(rx.NBodyError) as err:
            call()
        assert err.value.code == code
