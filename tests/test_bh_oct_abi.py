"""NBX_OPT_BH_DIM (the 3-D Barnes-Hut path) without a GPU: the option's values, and the walk kernel's resources."""
import os
import re

import pytest

from test_kernel_resources import CSRC, _metadata


def test_bh_dim_option_round_trips_and_21_stays_invalid(rx):
    from rust_exp_amd.engine import NBX_ERR_INVALID, NBX_OPT_BH_DIM

    assert NBX_OPT_BH_DIM == 22
    e = rx.NBodyEngine()
    assert e.query_option(NBX_OPT_BH_DIM) == 2            # the default never changes behaviour
    for v in (3, 2):
        e.set_bh_dim(v)
        assert e.query_option(NBX_OPT_BH_DIM) == v and e.get_option(NBX_OPT_BH_DIM) == v
    for bad in (0, 1, 4):
        with pytest.raises(rx.NBodyError) as err:
            e.set_bh_dim(bad)
        assert err.value.code == NBX_ERR_INVALID and e.query_option(NBX_OPT_BH_DIM) == 2
    for call in (lambda: e.query_option(21), lambda: e.set_option(21, 2)):
        with pytest.raises(rx.NBodyError) as err:
            call()
        assert err.value.code == NBX_ERR_INVALID


def test_octree_walk_keeps_eight_waves_per_simd(tmp_path):
    """k_oct_walk (step and forces-only forms): no scratch, no VGPR spill, at most 64 VGPRs."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = [f for var in ("STRICT", "NOPK") for f in re.search(r"^%s\s*:=\s*(.*)$" % var, mk, re.M).group(1).split()]
    k = _metadata(tmp_path, "bh_oct_walk.hip", flags)
    walks = [v for n, v in k.items() if "k_oct_walk" in n]
    assert len(walks) == 2
    for v in walks:
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["vgpr_count"] <= 64, v
