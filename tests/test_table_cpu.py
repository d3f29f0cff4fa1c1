"""CPU-only: the packer of the tensor tables (offsetguided_amd/_table.py) on hand-written rows and counts -- the prefix, the layout of
the bytes the device gets, their alignment -- and the contract of csrc/table.h's bisection over that prefix, restated in numpy: rows
without workgroups are passed over."""
import numpy as np
import pytest

from offsetguided_amd import _table

COUNTS = [0, 0, 3, 0, 2, 0]


def find_row(prefix, n_rows, wg):
    """og_find_row of csrc/table.h, statement by statement"""
    lo, hi = 0, n_rows
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if prefix[mid] <= wg:
            lo = mid
        else:
            hi = mid
    return lo


@pytest.mark.parametrize('words', [4, 5, 16])
def test_pack_lays_out_rows_then_prefix(words):
    table = (np.arange(len(COUNTS) * words, dtype=np.int64).reshape(len(COUNTS), words) + 1) * 0x0102030405060708 % (1 << 62)
    raw, prefix, at = _table.pack(table, COUNTS)
    assert prefix.dtype == np.int32 and prefix.tolist() == [0, 0, 0, 3, 3, 5, 5]
    assert raw.dtype == np.uint8 and raw.ndim == 1 and raw.size == 8 * table.size + 4 * (len(COUNTS) + 1)
    assert at == 8 * table.size and at % 8 == 0                  # the rows sit at byte 0 of an allocation: both parts are aligned
    assert np.array_equal(raw[:at].view(np.int64).reshape(table.shape), table)
    assert np.array_equal(raw[at:].view(np.int32), prefix)
    assert np.array_equal(_table.pack(table, np.array(COUNTS))[0], raw)


def test_rows_without_workgroups_are_passed_over():
    _, prefix, _ = _table.pack(np.zeros((len(COUNTS), 4), np.int64), COUNTS)
    assert [find_row(prefix, len(COUNTS), wg) for wg in range(5)] == [2, 2, 2, 4, 4]


def test_an_empty_table_packs_to_its_prefix_alone():
    """No caller special-cases it here: range_stats and the optimizers return before they pack, and the entry points refuse
    n_rows == 0 ('bad table size')."""
    raw, prefix, at = _table.pack(np.zeros((0, 5), np.int64), [])
    assert prefix.tolist() == [0] and at == 0 and raw.tobytes() == b'\0\0\0\0'
