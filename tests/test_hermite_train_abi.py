"""NBX_OPT_HERMITE_BLOCK_TRAIN and its two stats without a GPU: ids in the header against engine.py, default, range, wrapper."""
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbody_mi355x.h")
IDS = {"NBX_OPT_HERMITE_BLOCK_TRAIN": 23, "NBX_STAT_HERMITE_BLOCK_TRAIN_STEPS": 10, "NBX_STAT_HERMITE_BLOCK_READS": 11}


@pytest.mark.parametrize("name", list(IDS))
def test_ids_agree_between_header_and_binding(rx, name):
    assert int(re.search(name + r" = (\d+)", open(HEADER).read()).group(1)) == getattr(rx.engine, name) == IDS[name]


def test_option_default_range_and_wrapper(rx):
    from rust_exp_amd.engine import (NBX_ERR_INVALID, NBX_OPT_HERMITE_BLOCK_TRAIN, NBX_STAT_HERMITE_BLOCK_READS,
                                     NBX_STAT_HERMITE_BLOCK_TRAIN_STEPS)

    e = rx.NBodyEngine()
    assert e.query_option(NBX_OPT_HERMITE_BLOCK_TRAIN) == e.get_option(NBX_OPT_HERMITE_BLOCK_TRAIN) == 0
    e.set_hermite_block_train(16)
    assert e.query_option(NBX_OPT_HERMITE_BLOCK_TRAIN) == 16
    for bad in (-1, 257):
        with pytest.raises(rx.NBodyError) as err:
            e.set_hermite_block_train(bad)
        assert err.value.code == NBX_ERR_INVALID
    assert e.query_option(NBX_OPT_HERMITE_BLOCK_TRAIN) == 16
    assert e.get_stat(NBX_STAT_HERMITE_BLOCK_TRAIN_STEPS) == e.get_stat(NBX_STAT_HERMITE_BLOCK_READS) == 0
