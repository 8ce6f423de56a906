"""The Python tile tables (ops/tiles.py) against the C++ ones the kernels are
instantiated from (gemm_core.h, conv.hip, conv_halo.hip), exported by the
extension's host-only ``tile_tables()``.  The Python copies feed the candidate
lists, the CU-time ranking and the split-K workspace bound, so every field must
match.  Host calls only: no GPU."""
import pytest

from ray_dynamic_batching_amd import ops


@pytest.fixture(scope="module")
def cxx():
    try:
        ext = ops._ops()
    except Exception as e:   # extension not built in this checkout
        pytest.skip(f"ops extension unavailable: {e}")
    return ext.tile_tables()


def test_gemm_tile_tables_match(cxx):
    assert cxx["num_tiles"] == ops.NUM_TILE_CFGS == len(ops._ALL_BM) == len(ops._ALL_BN) == len(ops._ALL_NW)
    assert cxx["num_tiles4"] == ops.NUM_CONV_TILE_CFGS
    assert ops.NUM_LN_TILE_CFGS <= cxx["num_tiles"]
    assert tuple(cxx["bm"]) == ops._ALL_BM
    assert tuple(cxx["bn"]) == ops._ALL_BN
    assert tuple(cxx["nw"]) == ops._ALL_NW
    assert ops._TILE_BM == ops._ALL_BM[:cxx["num_tiles4"]] and ops._TILE_BN == ops._ALL_BN[:cxx["num_tiles4"]]
    assert len(cxx["blocks_per_cu"]) == cxx["num_tiles"]
    for t in range(cxx["num_tiles"]):
        assert ops._blocks_per_cu(t) == cxx["blocks_per_cu"][t], t
    assert tuple(cxx["stg_tiles"]) == ops.STG_TILE_CFGS
    assert cxx["deep_flag"] == ops.DEEP
    assert cxx["splitk_header"] == ops.SPLITK_HEADER
    assert tuple(cxx["pp_splitk_tiles"]) == ops._PP_SPLITK_TILES


def test_conv_tile_tables_match(cxx):
    assert tuple(cxx["conv_pp_bm"]) == ops._CONV_PP_BM
    assert tuple(cxx["conv_pp_bn"]) == ops._CONV_PP_BN
    assert tuple(cxx["conv_pp_bk"]) == ops._CONV_PP_BK
    assert tuple(cxx["halo_bm"]) == ops._CONV_HALO_BM
    assert tuple(cxx["halo_bn"]) == ops._CONV_HALO_BN
    assert max(ops._CONV_HALO_RW + ops._CONV_HALO_SK) < len(cxx["halo_bm"])
