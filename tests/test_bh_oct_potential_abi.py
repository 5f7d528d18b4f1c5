"""K14 without a GPU: nbx_bh_potential / nbx_bh_conserved declared, exported, wrapped; NBX_ERR_NO_DEVICE; the kernels' resources."""
import ctypes as C
import os
import re

import pytest

from test_kernel_resources import CSRC, ROOT, _metadata


def test_entry_points_are_declared_exported_and_wrapped(rx):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbody_mi355x.h")).read(), flags=re.S)
    L = C.CDLL(rx.lib_path())
    for name in ("nbx_bh_potential", "nbx_bh_conserved"):
        assert re.search(r"\bint32_t\s+%s\s*\(\s*nbx_engine\s*\*e,\s*float theta," % name, header), name
        assert hasattr(L, name) and callable(getattr(rx.NBodyEngine, name[4:]))
    e = rx.NBodyEngine()
    e.set_bh_dim(3)
    e.set_law("newton")
    e.random_disk(16)
    if rx.device_count() == 0:
        for call in (lambda: e.bh_potential(0.5), lambda: e.bh_conserved(0.5)):
            with pytest.raises(rx.NBodyError) as err:
                call()
            assert err.value.code == rx.NBX_ERR_NO_DEVICE


def test_potential_walk_kernels_use_no_scratch_and_keep_eight_waves_per_simd(tmp_path):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = [f for var in ("STRICT", "NOPK") for f in re.search(r"^%s\s*:=\s*(.*)$" % var, mk, re.M).group(1).split()]
    k = _metadata(tmp_path, "bh_oct_potential.hip", flags)
    assert len([n for n in k if "k_oct_phi" in n]) == 4
    for n, v in k.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["vgpr_count"] <= 64, (n, v)
