"""tests/engine_schedule.py's checker and role table on hand-written logs: no GPU, no library.  Streams are letters, byte ranges are
small integers; every log is the issue order of one imagined forward."""
import ctypes as C

import pytest

import engine_schedule as es
from engine_schedule import Launch, Record, Wait

X, UP, LOW, OUT, W = (0, 100), (100, 200), (200, 300), (300, 400), (1000, 1100)      # activations and one weight tensor


def _pairs(log, readonly=()):
    races, bad = es.check(log, readonly)
    return [(log[r.first].label, log[r.second].label, r.kind) for r in races], bad


def _fork_join(join=True):
    """trunk T writes x; side S forks from it, computes up = f(x); T computes low = g(x); join; merge up += low on T."""
    return [Launch('T', 'conv', (W,), (X,), (), 'producer'),
            Record('T', 'fork'), Wait('S', 'fork'),
            Launch('S', 'conv', (X, W), (UP,), (), 'up1'),
            Launch('T', 'conv', (X, W), (LOW,), (), 'low'),
            Record('S', 'done')] + ([Wait('T', 'done', 'level')] if join else []) + [
            Launch('T', 'og_upsample2_add', (UP, LOW), (UP,), (), 'merge')]


def test_fork_and_join_is_clean():
    assert _pairs(_fork_join()) == ([], [])


def test_missing_join_names_the_merge():
    pairs, _ = _pairs(_fork_join(join=False))
    assert pairs == [('up1', 'merge', 'write-write')]
    log = _fork_join()
    at = es.joins(log, 'level', 'T')
    assert len(at) == 1 and _pairs(es.without(log, at[0]))[0] == pairs
    assert 'up1' in es.report(es.without(log, at[0]), es.check(es.without(log, at[0]))) and 'merge' in es.describe(
        es.without(log, at[0]), es.check(es.without(log, at[0]))[0][0])


def test_missing_fork_names_the_branch():
    log = [e for e in _fork_join() if not (isinstance(e, Wait) and e.stream == 'S')]
    assert _pairs(log)[0] == [('producer', 'up1', 'write-read')]


def test_read_read_sharing_is_allowed():
    """Two streams read the same weights and the same input with no edge between them; only the read-only rule guards the weights."""
    log = [Launch('A', 'conv', (W, X), (UP,), (), 'a'), Launch('B', 'conv', (W, X), (LOW,), (), 'b')]
    assert _pairs(log, readonly=[W, X]) == ([], [])
    log.append(Launch('B', 'pack', (), ((1050, 1060),), (), 'repack'))
    pairs, bad = _pairs(log, readonly=[W, X])
    assert pairs == [('a', 'repack', 'read-write')] and [(b.index, b.lo, b.hi) for b in bad] == [(2, 1050, 1060)]


def test_scratch_is_a_write_between_streams_but_may_preexist():
    ws = (5000, 6000)
    log = [Launch('A', 'conv', (X,), (UP,), (ws,), 'a'), Launch('B', 'conv', (X,), (LOW,), (ws,), 'b')]
    pairs, bad = _pairs(log, readonly=[ws, X])
    assert pairs == [('a', 'b', 'write-write')] and bad == []
    assert _pairs([log[0], Launch('A', 'conv', (X,), (LOW,), (ws,), 'b')], readonly=[ws]) == ([], [])


def _shared_deep(join3):
    """Two branches in fork order on ONE side stream S (depth 3, then depth 4); the trunk joins the inner one first.  join3: how the
    trunk joins depth 4 -- 'event': the branch's own event; 'early': the event of depth 3, recorded BEFORE depth 4's work was queued;
    'stream': wait_stream at the join."""
    up3, up4, low3, low4 = UP, OUT, LOW, (400, 500)
    log = [Launch('T', 'conv', (), (X,), (), 'x'),
           Record('T', 'f3'), Wait('S', 'f3'), Launch('S', 'conv', (X,), (up3,), (), 'up1@3'), Record('S', 'done3'),
           Launch('T', 'conv', (X,), (low3,), (), 'low1@3'),
           Record('T', 'f4'), Wait('S', 'f4'), Launch('S', 'conv', (low3,), (up4,), (), 'up1@4'), Record('S', 'done4'),
           Launch('T', 'conv', (low3,), (low4,), (), 'low@4')]
    if join3 == 'stream':
        log += [Record('S', 'ws'), Wait('T', 'ws')]
    else:
        log += [Wait('T', 'done4' if join3 == 'event' else 'done3')]
    return log + [Launch('T', 'og_upsample2_add', (up4, low4), (up4,), (), 'merge@4'),
                  Wait('T', 'done3'), Launch('T', 'og_upsample2_add', (up3, up4), (up3,), (), 'merge@3')]


def test_shared_stream_per_branch_event_versus_wait_stream():
    assert _pairs(_shared_deep('event')) == ([], [])
    assert _pairs(_shared_deep('stream')) == ([], [])
    # an event recorded behind depth 3's work says nothing about what was queued on the stream after it
    assert _pairs(_shared_deep('early'))[0] == [('up1@4', 'merge@4', 'write-write'), ('up1@4', 'merge@3', 'write-read')]
    races, _ = es.check(_shared_deep('early'))
    assert [(_shared_deep('early')[r.second].label) for r in es.minimal(races, _shared_deep('early'))] == ['merge@4']
    # the join of depth 3 is implied by the join of depth 4 on a shared stream: stream order carries it
    log = _shared_deep('event')
    assert _pairs(es.without(log, es.joins(log, '', 'T')[-1])) == ([], [])


def test_event_recorded_again_is_a_new_point_in_time():
    log = [Record('S', 'e'), Launch('S', 'conv', (), (UP,), (), 'late'), Wait('T', 'e'), Launch('T', 'conv', (UP,), (LOW,), (), 'reader')]
    assert _pairs(log)[0] == [('late', 'reader', 'write-read')]
    log.insert(2, Record('S', 'e'))
    assert _pairs(log) == ([], [])
    assert _pairs([Wait('T', 'never'), Launch('T', 'conv', (), (UP,), (), 'a')]) == ([], [])


def test_address_reuse_after_free_on_another_stream():
    """S reads tensor t at [100, 200).  The host drops t; the allocator hands the block to the trunk's next output while nothing orders
    the trunk behind S's read."""
    log = [Launch('T', 'conv', (), (UP,), (), 'writes t'), Record('T', 'f'), Wait('S', 'f'),
           Launch('S', 'conv', (UP,), (LOW,), (), 'reads t'),
           Launch('T', 'conv', (X,), ((120, 180),), (), 'writes t2 into the freed block')]
    pairs, _ = _pairs(log)
    assert ('reads t', 'writes t2 into the freed block', 'read-write') in pairs
    joined = log[:4] + [Record('S', 'd'), Wait('T', 'd')] + log[4:]
    assert _pairs(joined) == ([], [])


def test_transitive_order_through_a_third_stream():
    log = [Launch('A', 'conv', (), (X,), (), 'a'), Record('A', 'ab'), Wait('B', 'ab'),
           Launch('B', 'conv', (X,), (UP,), (), 'b'), Record('B', 'bc'), Wait('C', 'bc'),
           Launch('C', 'conv', (X, UP), (OUT,), (), 'c')]
    assert _pairs(log) == ([], [])
    # without the second edge C knows of neither
    assert _pairs(es.without(log, 5))[0] == [('a', 'c', 'write-read'), ('b', 'c', 'write-read')]
    # an edge taken from A BEFORE a launched says nothing about a
    early = [Record('A', 'ab')] + [e for e in log if e != Record('A', 'ab')]
    assert ('a', 'b', 'write-read') in _pairs(early)[0]


def test_minimal_keeps_independent_races():
    log = [Launch('S', 'conv', (), (UP,), (), 's1'), Launch('S', 'conv', (), (LOW,), (), 's2'),
           Launch('T', 'conv', (LOW,), (OUT,), (), 't1'), Launch('T', 'conv', (UP,), (X,), (), 't2'),
           Launch('R', 'conv', (UP,), ((600, 700),), (), 'r')]
    races, _ = es.check(log)
    assert len(races) == 3
    assert [(log[r.first].label, log[r.second].label) for r in es.minimal(races, log)] == [('s1', 'r'), ('s2', 't1')]


def test_two_lanes_share_weights_only():
    """Engines A and B on two lanes, nothing between them: clean while their activations are disjoint, reported where they meet."""
    def forward(lane, base, w=W):
        a, b = (base, base + 50), (base + 50, base + 100)
        return [Launch(lane, 'conv', (w,), (a,), (), f'{lane}1'), Launch(lane, 'conv', (w, a), (b,), (), f'{lane}2')]
    assert _pairs(forward('A', 0) + forward('B', 100) + forward('A', 0), readonly=[W]) == ([], [])
    assert _pairs(forward('A', 0) + forward('B', 50))[0] == [('A2', 'B1', 'write-write'), ('A2', 'B2', 'write-read')]


# ------------------------------------------------------------------------------------------------------------------ role table
def _p(v):
    return C.c_void_p(v) if v else None


def test_launch_entry_roles_and_scratch():
    ext = {0x100: (0x100, 0x180), 0x210: (0x200, 0x280), 0x300: (0x300, 0x340), 0x400: (0x400, 0x480), 0x500: (0x500, 0x580)}
    a = (_p(0x100), _p(0x210), _p(0x300), None, _p(0x500), 1, 8, 8, 64, 64, 1, _p(0x9000), 256, _p(0x77))
    e = es.launch_entry('og_conv3x3_tiled_f16', a, ext, 'layer')
    assert e == Launch(0x77, 'og_conv3x3_tiled', ((0x100, 0x180), (0x200, 0x280), (0x300, 0x340)), ((0x500, 0x580),), ((0x9000, 0x9100),), 'layer')
    up2 = es.launch_entry('og_conv3x3_tiled_up2_bf16', a, ext)
    assert (0x500, 0x580) in up2.reads and up2.writes == ((0x500, 0x580),)             # in place
    add = es.launch_entry('og_upsample2_add_f16', (_p(0x100), _p(0x400), 1, 8, 8, 64, None), ext)
    assert add.stream == 0 and add.writes == ((0x100, 0x180),) and add.reads == ((0x100, 0x180), (0x400, 0x480))
    with pytest.raises(AssertionError, match='did not come from _lib.ptr'):
        es.launch_entry('og_upsample2_add_f16', (_p(0x100), _p(0x404), 1, 8, 8, 64, None), ext)


def test_launch_entry_heads_outputs_from_the_arguments():
    ext = {0x100: (0x100, 0x180), 0x200: (0x200, 0x280), 0x300: (0x300, 0x340)}
    chans, ptrs = (C.c_int * 2)(17, 38), (C.c_void_p * 2)(0x10000, 0x20000)
    e = es.launch_entry('og_conv1x1_heads_bf16', (_p(0x100), 256, _p(0x200), _p(0x300), 2, 4, 8, 64, 2, chans, ptrs, _p(0x5)), ext)
    assert e.writes == ((0x10000, 0x10000 + 2 * 17 * 32 * 4), (0x20000, 0x20000 + 2 * 38 * 32 * 4)) and len(e.reads) == 3


def test_an_entry_point_without_a_row_fails():
    with pytest.raises(AssertionError, match='no row in engine_schedule.ROLES'):
        es.launch_entry('og_hmp_nms_f32', (_p(0x100), 1, 1, 1, _p(0x200), None), {})


def test_role_table_covers_the_engine_and_matches_the_abi():
    """Every 16-bit entry point and layout pass that models/engine.py names has a row, every row is an entry point of the ABI, and a
    role never points at an argument that is not a pointer (or a scratch pointer not followed by its size)."""
    import os
    import re

    from offsetguided_amd import _lib
    src = open(os.path.join(os.path.dirname(_lib.__file__), 'models', 'engine.py')).read()
    called = set(re.findall(r"_lib\.lp\(lib, '(\w+)'", src)) | set(re.findall(r'lib\.(og_\w+)\(', src))
    missing = {n for n in called if es.stem_of(n) not in es.ROLES and n not in es.HOST_ONLY}
    assert not missing, missing
    for stem, roles in es.ROLES.items():
        names = [n for n in (stem, stem + '_bf16', stem + '_f16') if n in _lib.SIGNATURES]
        assert names, stem
        for name in names:
            args = _lib.SIGNATURES[name][1]
            assert args[-1] is C.c_void_p
            for i, role in roles:
                assert args[i] is C.c_void_p, (name, i)
                assert role != 's' or args[i + 1] is C.c_size_t, (name, i)
    assert es.HOST_ONLY <= set(_lib.SIGNATURES)


def test_a_shared_side_stream_is_released_once():
    """The deep stream of a dead engine sits in several levels' _side tables.  The first eviction frees its handle, a new engine takes
    it; the second table's eviction of the same dead key must not free it again under the new owner (found by the two-lane audit:
    two live engines ended up on one side stream)."""
    import types

    from offsetguided_amd import _lib
    from offsetguided_amd.models import engine as E
    h = 0x7777
    st = types.SimpleNamespace(cuda_stream=h, device=types.SimpleNamespace(index=0))
    free = _lib._free_streams.setdefault(0, set())
    dead, new = (0, -5), (0, -6)
    try:
        E._side_owner[h] = dead
        E._release_side(st, dead)                        # first table
        assert h in free and h not in E._side_owner
        free.discard(h)                                  # _lib.new_stream hands it to the next engine
        E._side_owner.setdefault(h, new)
        E._release_side(st, dead)                        # second table, same dead key
        assert h not in free and E._side_owner[h] == new
        E._release_side(st, new)
        assert h in free
    finally:
        free.discard(h)
        E._side_owner.pop(h, None)
