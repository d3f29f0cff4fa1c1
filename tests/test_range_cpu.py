"""CPU-only: the numpy restatement of the range report's nine words (tests/range_common.py) against numpy's own fp32 -> fp16 cast and
torch-CPU's fp32 -> bf16 cast, on the directed values at every edge of the two types and on 10^5 seeded random bit patterns; the
--range-report flag parses; range_report.decode turns words 7 and 8 back into the magnitudes."""
import numpy as np
import pytest
import torch

import range_common as rg
from offsetguided_amd import evaluate
from offsetguided_amd.models import range_report


def _cases():
    rs = np.random.RandomState(7)
    return np.concatenate([rg.directed32(), rs.randint(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32)])


def _cast(x_bits, target):
    """fp32 patterns -> (the cast's own 16-bit patterns without the sign, as int64)"""
    x = x_bits.view(np.float32)
    if target == 'f16':
        with np.errstate(over='ignore', under='ignore', invalid='ignore'):
            y = x.astype(np.float16).view(np.uint16)
    else:
        y = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    return (y & np.uint16(0x7fff)).astype(np.int64)


@pytest.mark.parametrize('target', ['f16', 'bf16'])
def test_rounding_restated_equals_the_casts(target):
    x = _cases()
    mine = (rg.f32_to_f16_bits(x) if target == 'f16' else rg.f32_to_bf16_bits(x)).astype(np.int64)
    theirs = _cast(x, target)
    inf_t = rg.LP[target][0]
    nan = (x & np.uint32(0x7fffffff)) > rg.F32_INF
    assert np.array_equal(mine[~nan], theirs[~nan])
    assert (mine[nan] > inf_t).all() and (theirs[nan] > inf_t).all()          # a NaN stays a NaN; the payload is the cast's business


@pytest.mark.parametrize('target', ['f16', 'bf16'])
def test_nine_words_against_the_casts(target):
    """Every class from VALUES (the cast's result and float comparisons) == the restatement's, element by element and summed."""
    inf_t, normal_t = rg.LP[target]
    for x in (_cases(), rg.directed32()):
        y = _cast(x, target)
        with np.errstate(invalid='ignore'):          # signalling NaNs among the patterns
            v = x.view(np.float32).astype(np.float64)
        fin = np.isfinite(v)
        want = np.zeros(rg.WORDS, np.int64)
        want[0] = x.size
        want[1] = np.isnan(v).sum()
        want[2] = np.isinf(v).sum()
        want[3] = (fin & (y == inf_t)).sum()
        want[4] = (v == 0).sum()
        want[5] = ((v != 0) & ~np.isnan(v) & (y == 0)).sum()
        want[6] = ((y > 0) & (y < normal_t)).sum()
        want[7] = np.float32(np.abs(v[fin]).max()).view(np.uint32)
        want[8] = rg.F32_INF - int(np.float32(np.abs(v[fin & (v != 0)]).min()).view(np.uint32))
        assert np.array_equal(rg.stats_ref(x, 'f32', target), want)
        for i in range(len(rg.DIRECTED32) * 2):      # the directed values one by one: a miscounted edge cannot hide in a sum
            one = rg.stats_ref(rg.directed32()[i:i + 1], 'f32', target)
            yi, vi = _cast(rg.directed32()[i:i + 1], target)[0], rg.directed32()[i:i + 1].view(np.float32)[0]
            assert one[3] == int(np.isfinite(vi) and yi == inf_t) and one[5] == int(vi != 0 and not np.isnan(vi) and yi == 0)
            assert one[6] == int(0 < yi < normal_t), hex(int(rg.directed32()[i]))


def test_the_named_edges():
    """The figures the header states, spelled out."""
    def one(bits, target):
        return dict(zip(rg.NAMES, rg.stats_ref(np.array([bits], np.uint32), 'f32', target)))
    assert np.float32(65520.0).view(np.uint32) == 0x477ff000 and np.float32(2.0 ** -25).view(np.uint32) == 0x33000000
    assert one(0x477ff000, 'f16')['over'] == 1 and one(0x477fefff, 'f16')['over'] == 0 and one(0x477fe000, 'f16')['over'] == 0
    assert one(0x33000000, 'f16')['flush'] == 1 and one(0x32ffffff, 'f16')['flush'] == 1 and one(0x33000001, 'f16')['flush'] == 0
    assert one(0x33000001, 'f16')['sub'] == 1 and one(0x33800000, 'f16')['sub'] == 1
    assert one(0x387fffff, 'f16')['sub'] == 0 and one(0x38800000, 'f16')['sub'] == 0 and one(0x387fdfff, 'f16')['sub'] == 1
    assert one(0x7f7f7fff, 'bf16')['over'] == 0 and one(0x7f7f8000, 'bf16')['over'] == 1
    assert one(0x00008000, 'bf16')['flush'] == 1 and one(0x00008001, 'bf16')['flush'] == 0 and one(0x00008001, 'bf16')['sub'] == 1
    assert one(0x80000000, 'f16')['zero'] == 1 and one(0xff800000, 'f16')['inf'] == 1 and one(0xffc12345, 'bf16')['nan'] == 1
    assert one(0x7f7fffff, 'f16')['max'] == 0x7f7fffff and one(0x00000001, 'f16')['min'] == rg.F32_INF - 1
    assert one(0x7fc00000, 'f16')['max'] == 0 and one(0, 'f16')['min'] == 0


@pytest.mark.parametrize('target', ['f16', 'bf16'])
def test_sixteen_bit_sources(target):
    """S = T: every one of the 65536 patterns; nothing rounds, the magnitudes are widened exactly."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    got = dict(zip(rg.NAMES, rg.stats_ref(bits, target, target)))
    inf_t, normal_t = rg.LP[target]
    assert got['n'] == 65536 and got['over'] == 0 and got['flush'] == 0 and got['zero'] == 2 and got['inf'] == 2
    assert got['nan'] == 2 * (0x7fff - inf_t) and got['sub'] == 2 * (normal_t - 1)
    big, tiny = (65504.0, 2.0 ** -24) if target == 'f16' else (float(np.array([0x7f7f0000], np.uint32).view(np.float32)[0]), 2.0 ** -133)
    assert got['max'] == np.float32(big).view(np.uint32) and got['min'] == rg.F32_INF - int(np.float32(tiny).view(np.uint32))
    # a 16-bit tensor counts as its fp32 copy does, apart from the words that are about rounding
    wide = rg.stats_ref(rg.widen(bits, target), 'f32', target)
    assert np.array_equal(wide, rg.stats_ref(bits, target, target))


def test_range_report_flag_parses():
    assert evaluate.evaluate_cli(['--range-report', 'r.json']).range_report == 'r.json'
    assert evaluate.evaluate_cli([]).range_report is None


def test_decode_round_trips_max_and_min():
    values = np.array([1.5, -3.0e4, 2.0 ** -20, 0.0, np.inf, np.nan, 2.0 ** -140], np.float32)
    row = rg.stats_ref(values.view(np.uint32), 'f32', 'f16')
    empty = rg.stats_ref(np.array([0x7f800000, 0], np.uint32), 'f32', 'f16')
    got, none = range_report.decode(torch.from_numpy(np.stack([row, empty])))
    assert got['max'] == 3.0e4 and got['min'] == 2.0 ** -140 and none['max'] == 0.0 and none['min'] == 0.0
    assert [got[k] for k in rg.NAMES[:7]] == [7, 1, 1, 0, 1, 1, 1] and tuple(got) == rg.NAMES
    both = range_report.combine([torch.from_numpy(row).reshape(1, -1), torch.from_numpy(empty).reshape(1, -1)])
    assert np.array_equal(both.numpy()[0], rg.combine([row, empty]))
