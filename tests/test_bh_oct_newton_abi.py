"""K13 without a GPU: NBX_OPT_BH_QUADRUPOLE, nbx_bh_oct_moments, and the resources of bh_oct_newton.hip's kernels."""
import os
import re

import pytest

from test_kernel_resources import CSRC, ROOT, _metadata


def test_quadrupole_option_and_moments_entry_point(rx):
    header = open(os.path.join(ROOT, "include", "nbody_mi355x.h")).read()
    assert int(re.search(r"NBX_OPT_BH_QUADRUPOLE\s*=\s*(\d+)", header).group(1)) == rx.NBX_OPT_BH_QUADRUPOLE == 25
    e = rx.NBodyEngine()
    assert e.get_option(rx.NBX_OPT_BH_QUADRUPOLE) == e.query_option(rx.NBX_OPT_BH_QUADRUPOLE) == 1
    for on in (False, True, False):
        e.set_bh_quadrupole(on)
        assert e.get_option(rx.NBX_OPT_BH_QUADRUPOLE) == e.query_option(rx.NBX_OPT_BH_QUADRUPOLE) == int(on)
    with pytest.raises(rx.NBodyError) as err:
        e.set_option(rx.NBX_OPT_BH_QUADRUPOLE, 2)
    assert err.value.code == rx.NBX_ERR_INVALID and e.get_option(rx.NBX_OPT_BH_QUADRUPOLE) == 0
    if rx.device_count() == 0:   # without a device the moments answer as the dump does
        e.random_disk(16)
        codes = []
        for call in (e.bh_oct_dump, e.bh_oct_moments):
            with pytest.raises(rx.NBodyError) as err:
                call()
            codes.append(err.value.code)
        assert codes[0] == codes[1] == rx.NBX_ERR_NO_DEVICE


def test_newtonian_octree_kernels_use_no_scratch(tmp_path):
    """the four k_oct_walk_newton<KICK, QUAD> and the moments kernels: no scratch, no spills (registers: docs/rounds/r14.md)"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = [f for var in ("STRICT", "NOPK") for f in re.search(r"^%s\s*:=\s*(.*)$" % var, mk, re.M).group(1).split()]
    k = _metadata(tmp_path, "bh_oct_newton.hip", flags)
    assert len([n for n in k if "k_oct_walk_newton" in n]) == 4
    assert all(any(name in n for n in k) for name in ("k_oct_mom_index", "k_oct_mom_sweep", "k_oct_quads", "k_oct_moment_rows"))
    for n, v in k.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (n, v)
