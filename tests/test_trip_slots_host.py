"""The LDS size rule behind round 11's one-row-per-sphere scene table (csrc/rtm_render_kernel.h: render_lds_bytes, lds_table_bytes;
csrc/rtm_path.h: SceneLdsRows), on the host through rtm_debug_tol_lds_bytes: for every shape of the tolerance row and 1 .. 24
spheres the row layout costs exactly its padding — 8 bytes a sphere, geometry (32) + normal row (24) -> one row of 64 — plus at
most the near-unit Normalize table where the two layouts disagree about it, and at 7 spheres, the only count whose kernels take
it (the axis-signature instantiations), every shape stays under the 10 240 bytes a wave may take for 16 waves per CU (4 per SIMD)
WITH the near-unit table, as before."""
import ctypes as C

import pytest

from raytracingmin_amd import _lib

LDS_PER_CU = 160 * 1024
WAVES_PER_CU = 16          # 4 per SIMD at the kernels' 128 registers
UNIT_TABLE_BYTES = 256     # csrc/rtm_render_kernel.h: kUnitTableBytes
ROW_PADDING = 8            # bytes per sphere


def _bytes(n, any_depth, split, rows):
    out = (C.c_uint64 * 2)()
    _lib.check(_lib.lib().rtm_debug_tol_lds_bytes(n, any_depth, split, rows, out), "lds bytes")
    return int(out[0]), int(out[1])


def _waves(b):
    return min(WAVES_PER_CU, LDS_PER_CU // b)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("any_depth", [0, 1])
def test_row_layout_costs_its_padding_and_no_wave(any_depth, split):
    for n in range(1, 25):
        old, old_unit = _bytes(n, any_depth, split, 0)
        new, new_unit = _bytes(n, any_depth, split, 1)
        tables_only = (new - new_unit * UNIT_TABLE_BYTES) - (old - old_unit * UNIT_TABLE_BYTES)
        assert tables_only == ROW_PADDING * n, (n, old, new)
        assert new <= old + ROW_PADDING * n + UNIT_TABLE_BYTES * max(0, new_unit - old_unit), (n, old, new)
        assert old % 8 == 0 and new % 8 == 0
    # the kernels that take the rows are launched for exactly 7 spheres
    old, old_unit = _bytes(7, any_depth, split, 0)
    new, new_unit = _bytes(7, any_depth, split, 1)
    assert old_unit == 1 and new_unit == 1
    assert new == old + ROW_PADDING * 7
    assert new * WAVES_PER_CU <= LDS_PER_CU and _waves(new) == _waves(old) == WAVES_PER_CU


def test_where_the_rows_would_stop_fitting():
    """why the chunked kernel (8 .. 24 spheres here) keeps three tables: with rows the any-depth shape loses a wave per CU at 22
    and 23 spheres and the depth-capped one the near-unit table at 24"""
    lost = [n for n in range(1, 25) if _waves(_bytes(n, 1, 0, 1)[0]) < _waves(_bytes(n, 1, 0, 0)[0])]
    assert lost == [22, 23]
    assert _bytes(24, 0, 0, 0)[1] == 1 and _bytes(24, 0, 0, 1)[1] == 0
    assert all(_bytes(n, 0, 0, 1)[1] == 1 for n in range(1, 24))


def test_arguments_are_checked():
    out = (C.c_uint64 * 2)()
    assert _lib.lib().rtm_debug_tol_lds_bytes(0, 0, 0, 0, out) != 0
    assert _lib.lib().rtm_debug_tol_lds_bytes(25, 0, 0, 0, out) != 0
    assert _lib.lib().rtm_debug_tol_lds_bytes(7, 0, 0, 0, None) != 0
