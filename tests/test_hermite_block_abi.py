"""nbx_step_hermite_block and its companions without a GPU: exported symbols, the header's prototypes against the ctypes signatures
engine.py binds, the appended stat ids, wrappers and statuses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbody_mi355x.h")
F6 = ["float *"] * 6
PROTOS = {   # name -> the header's parameter types after the engine
    "nbx_step_hermite_block": ["float", "float"],
    "nbx_hermite_block_set_levels": ["const int32_t *", "int32_t"],
    "nbx_hermite_block_levels": ["int32_t", "int32_t *"],
    "nbx_hermite_kept": ["int32_t"] + F6,
    "nbx_acc_jerk_subset": ["const int32_t *", "int32_t"] + F6,
}
CTYPES = {"float": C.c_float, "int32_t": C.c_int32}


@pytest.mark.parametrize("name", list(PROTOS))
def test_symbol_header_and_binding_agree(rx, name):
    fn = getattr(rx.lib(), name)   # (AttributeError: the library does not export it)
    text = " ".join(open(HEADER).read().split())
    m = re.search(r"int32_t %s\(nbx_engine \*e, ([^)]*)\);" % name, text)
    assert m, name + " is not declared in the header"
    params = [re.sub(r"\w+$", "", p).strip() for p in m.group(1).split(",")]
    assert params == PROTOS[name]
    assert fn.restype is C.c_int32
    assert list(fn.argtypes) == [C.c_void_p] + [CTYPES.get(p, C.c_void_p) for p in params]


def test_stat_ids_and_wrappers(rx):
    from rust_exp_amd import engine as eng

    text = open(HEADER).read()
    for name in ("NBX_STAT_HERMITE_BLOCK_STEPS", "NBX_STAT_HERMITE_BLOCK_EVALS"):
        assert int(re.search(name + r" = (\d+)", text).group(1)) == getattr(eng, name)
    assert int(re.search(r"#define NBX_HERMITE_MAX_LEVEL (\d+)", text).group(1)) == eng.NBX_HERMITE_MAX_LEVEL == 20
    assert all(callable(getattr(rx.NBodyEngine, k)) for k in ("step_hermite_block", "set_hermite_block_levels", "hermite_block_levels",
                                                              "hermite_kept", "acc_jerk_subset"))


def test_statuses_with_and_without_a_device(rx):
    from rust_exp_amd.engine import NBX_ERR_NO_DEVICE, NBX_ERR_STATE

    e = rx.NBodyEngine(mode="strict")   # (a configuration the step refuses: without a device that is not looked at)
    one = np.ones(8, np.float32)
    e.set_particles(np.arange(8), one, one, one, one)
    code = NBX_ERR_NO_DEVICE if rx.device_count() == 0 else NBX_ERR_STATE
    for call in (lambda: e.step_hermite_block(0.01, 0.02), lambda: e.set_hermite_block_levels(np.zeros(8)), e.hermite_block_levels,
                 e.hermite_kept, lambda: e.acc_jerk_subset([0, 1])):
        with pytest.raises(rx.NBodyError) as err:
            call()
        assert err.value.code == code
    assert e.get_stat(rx.engine.NBX_STAT_HERMITE_BLOCK_STEPS) == 0
