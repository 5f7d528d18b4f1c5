"""nbx_forces_f64 / nbx_conserved without a GPU: symbols, constants, wrappers, statuses, and the sweep kernels' resources."""
import os
import re

import numpy as np
import pytest

from test_kernel_resources import CSRC, _metadata


def test_symbols_constants_and_wrappers_exist(rx):
    L = rx.lib()
    assert L.nbx_forces_f64 and L.nbx_conserved
    names = ("KINETIC", "POTENTIAL", "MASS", "PX", "PY", "PZ", "LX", "LY", "LZ", "MRX", "MRY", "MRZ", "COUNT")
    assert [getattr(rx, "NBX_CONS_" + k) for k in names] == list(range(13))
    assert callable(rx.NBodyEngine.forces_f64) and callable(rx.NBodyEngine.conserved)


def test_statuses_with_and_without_a_device(rx):
    from rust_exp_amd.engine import NBX_ERR_INVALID, NBX_ERR_NO_DEVICE

    e = rx.NBodyEngine()
    one = np.ones(8, np.float32)
    e.set_particles(np.arange(8), one, one, one, one)
    if rx.device_count() == 0:
        calls, code = (e.forces_f64, e.conserved), NBX_ERR_NO_DEVICE
    else:
        calls, code = (lambda: e.conserved(count=11),), NBX_ERR_INVALID
    for call in calls:
        with pytest.raises(rx.NBodyError) as err:
            call()
        assert err.value.code == code


def test_sweep_kernels_keep_four_waves_per_simd(tmp_path):
    """k_sweep64<POT> (both): no scratch, no spills, at most 128 VGPRs -- four waves per SIMD, i.e. the four workgroups per CU that
    sweep64_split sizes the source split for."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    k = _metadata(tmp_path, "diag64.hip", re.search(r"^NOPK\s*:=\s*(.*)$", mk, re.M).group(1).split())
    sweeps = [v for n, v in k.items() if "k_sweep64" in n]
    assert len(sweeps) == 2
    for v in sweeps:
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, v
        assert v["vgpr_count"] <= 128 and 4 * v["group_segment_fixed_size"] <= 160 * 1024, v
