"""NBX_OPT_LAW without a GPU: number, values, set / read back; resources of k_newton_pkw (force_newton.hip), k_newton64 (diag64.hip)."""
import os
import re

import pytest

from test_kernel_resources import CSRC, ROOT, _metadata


def test_option_id_default_round_trip_and_invalid_values(rx):
    header = open(os.path.join(ROOT, "include", "nbody_mi355x.h")).read()
    assert int(re.search(r"NBX_OPT_LAW\s*=\s*(\d+)", header).group(1)) == rx.NBX_OPT_LAW == 24
    assert (rx.NBX_LAW_REFERENCE, rx.NBX_LAW_NEWTON) == (0, 1)
    e = rx.NBodyEngine()
    assert e.get_option(rx.NBX_OPT_LAW) == e.query_option(rx.NBX_OPT_LAW) == 0
    for law, value in (("newton", 1), ("reference", 0), ("newton", 1)):
        e.set_law(law)
        assert e.get_option(rx.NBX_OPT_LAW) == e.query_option(rx.NBX_OPT_LAW) == value
    for bad in (2, -1):
        with pytest.raises(rx.NBodyError) as err:
            e.set_option(rx.NBX_OPT_LAW, bad)
        assert err.value.code == rx.NBX_ERR_INVALID and e.get_option(rx.NBX_OPT_LAW) == 1


def test_newtonian_sweeps_keep_their_occupancy(tmp_path):
    """four k_newton_pkw: no scratch, no spills, <= 64 VGPRs (8 waves per SIMD, as K1); two k_newton64: the same at 128 (as K7)"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    nopk = re.search(r"^NOPK\s*:=\s*(.*)$", mk, re.M).group(1).split()
    for source, flags, count, vgprs in (("force_newton.hip", [], 4, 64), ("diag64.hip", nopk, 2, 128)):
        sweeps = [v for n, v in _metadata(tmp_path, source, flags).items() if "k_newton" in n]
        assert len(sweeps) == count, (source, len(sweeps))
        for v in sweeps:
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, v
            assert v["vgpr_count"] <= vgprs, v
