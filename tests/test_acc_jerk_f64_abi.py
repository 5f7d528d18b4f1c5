"""nbx_acc_jerk_f64 without a GPU: symbol, wrapper, status, and the resources of every k_acc_jerk64 instantiation (acc_jerk64.hip)."""
import os
import re

import numpy as np
import pytest

from test_kernel_resources import CSRC, _metadata


def test_symbol_wrapper_and_status_without_a_device(rx):
    assert rx.lib().nbx_acc_jerk_f64 and callable(rx.NBodyEngine.acc_jerk_f64)
    e = rx.NBodyEngine()
    e.set_particles(np.arange(8), *[np.ones(8, np.float32)] * 4)
    if rx.device_count() == 0:
        for idx in (None, [3]):
            with pytest.raises(rx.NBodyError) as err:
                e.acc_jerk_f64(idx)
            assert err.value.code == rx.NBX_ERR_NO_DEVICE
    else:
        assert [a.shape for a in e.acc_jerk_f64([3, 3])] == [(2,)] * 6


def test_every_sweep_keeps_four_waves_per_simd(tmp_path):
    """k_acc_jerk64<LAW, T>, laws x built T: no scratch, no spills, at most 128 VGPRs, and LDS for four workgroups per CU"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    k = _metadata(tmp_path, "acc_jerk64.hip", re.search(r"^NOPK\s*:=\s*(.*)$", mk, re.M).group(1).split())
    sweeps = [v for n, v in k.items() if "k_acc_jerk64" in n]
    assert len(sweeps) == 2 * 3   # laws x built T (1, 2, 4)
    for v in sweeps:
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, v
        assert v["vgpr_count"] <= 128 and 4 * v["group_segment_fixed_size"] <= 160 * 1024, v
