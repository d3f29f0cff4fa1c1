"""The schedule of models/engine.py as a log of issued work, and a happens-before check over it (tests/test_engine_schedule_cpu.py,
tests/test_gpu_engine_schedule.py).

The engine forks the up1 branch of every hourglass level onto a side stream and joins it with events.  Whether the joins are
sufficient does not depend on how the hardware happened to time one run: it is a property of the ORDER in which launches, event
records and event waits are issued.  `Recorder` logs that order during an eager forward; `check` runs vector clocks over the log and
reports every pair of accesses to overlapping bytes, on different streams, at least one of them a write, that no chain of
record -> wait edges orders.

The log is a list of three kinds of entries:
    Launch(stream, name, reads, writes, scratch, label)   reads / writes / scratch: tuples of (lo, hi) byte ranges, hi exclusive
    Record(stream, event, label)                          `event`: any hashable; recording it again replaces the snapshot
    Wait(stream, event, label)                            a wait on an event never recorded is a no-op, as in HIP
Streams are any hashable.  Work on one stream is ordered by issue order.  Stream.wait_stream(other) is Record(other, e) + Wait(self, e)
with a fresh e.  The checker knows addresses, not tensors: a block the caching allocator hands to a second tensor while another
stream may still read the first shows up as what it is, two unordered accesses to the same bytes.

Torch ops the engine issues between its launches (cat, copy_, zeros, contiguous, ...) are recorded through a TorchDispatchMode
(`_TorchOps`), not listed by hand: every dispatched op that is neither an allocation nor a pure view is an access on the current
stream, reading its tensor arguments and writing the arguments its schema marks as mutated plus every output with storage of its own."""
from collections import namedtuple

Launch = namedtuple('Launch', 'stream name reads writes scratch label', defaults=((), (), (), ''))
Record = namedtuple('Record', 'stream event label', defaults=('',))
Wait = namedtuple('Wait', 'stream event label', defaults=('',))

# first / second: log indices of the two launches (first was issued earlier); lo, hi: the overlap
Race = namedtuple('Race', 'first second lo hi kind')               # kind: 'write-write' | 'read-write' | 'write-read' (first-second)
ReadonlyWrite = namedtuple('ReadonlyWrite', 'index lo hi')         # a launch that writes bytes that existed before the forward


# ------------------------------------------------------------------------------------------------------------------- the checker
def _clocks(log):
    """-> {log index of a launch: (stream, tick on its stream, clock at issue {stream: tick})}"""
    clock, events, out = {}, {}, {}
    for idx, e in enumerate(log):
        mine = clock.setdefault(e.stream, {})
        if isinstance(e, Launch):
            mine[e.stream] = mine.get(e.stream, 0) + 1
            out[idx] = (e.stream, mine[e.stream], dict(mine))
        elif isinstance(e, Record):
            events[e.event] = dict(mine)                # everything issued on this stream so far, and what that had waited for
        elif isinstance(e, Wait):
            for s, t in events.get(e.event, {}).items():
                if t > mine.get(s, 0):
                    mine[s] = t
        else:
            raise TypeError(f'log entry {idx}: {e!r}')
    return out


def happens_before(clocks, a, b):
    """Launch a (log index) is complete before launch b starts, by stream order or a chain of record -> wait edges."""
    sa, ta, _ = clocks[a]
    return clocks[b][2].get(sa, 0) >= ta and a != b and (sa != clocks[b][0] or a < b)


def check(log, readonly=()):
    """-> (races, readonly_writes).  readonly: (lo, hi) ranges that existed before the log began (weights, inputs); a non-scratch write
    into one is reported.  Scratch ranges count as writes between launches but may lie in a range that existed before."""
    clocks = _clocks(log)
    acc = []                                                        # (lo, hi, log index, is write)
    for idx, e in enumerate(log):
        if isinstance(e, Launch):
            acc += [(lo, hi, idx, False) for lo, hi in e.reads if hi > lo]
            acc += [(lo, hi, idx, True) for lo, hi in tuple(e.writes) + tuple(e.scratch) if hi > lo]
    acc.sort()
    races = {}
    for i, (lo, hi, a, wa) in enumerate(acc):
        for j in range(i + 1, len(acc)):
            lo2, hi2, b, wb = acc[j]
            if lo2 >= hi:
                break
            if not (wa or wb) or log[a].stream == log[b].stream:
                continue
            first, second, wf, ws = (a, b, wa, wb) if a < b else (b, a, wb, wa)
            if happens_before(clocks, first, second) or happens_before(clocks, second, first):
                continue
            kind = 'write-write' if wf and ws else ('write-read' if wf else 'read-write')
            key = (first, second)
            if key not in races or (kind == 'write-write' and races[key].kind != kind):
                races[key] = Race(first, second, max(lo, lo2), min(hi, hi2), kind)
    ro = sorted((lo, hi) for lo, hi in readonly if hi > lo)
    bad = []
    for idx, e in enumerate(log):
        if isinstance(e, Launch):
            for lo, hi in e.writes:
                hit = next(((max(lo, a), min(hi, b)) for a, b in ro if a < hi and lo < b), None)
                if hit is not None:
                    bad.append(ReadonlyWrite(idx, *hit))
    return sorted(races.values()), bad


def minimal(races, log):
    """The races that are not consequences of another one: (a, b) follows from (a2, b2) when a2 is the same launch as a or a later one
    on a's stream and b2 is the same launch as b or an earlier one on b's stream -- the edge a2 -> b2 that mends the second orders the
    first as well.  A join taken out leaves many unordered pairs (everything the branch did against everything the trunk does with
    its bytes afterwards) and ONE minimal pair: the branch's last writer and the join's consumer."""
    def implied(r, by):
        return (by != r and log[by.first].stream == log[r.first].stream and log[by.second].stream == log[r.second].stream
                and by.first >= r.first and by.second <= r.second)
    return [r for r in races if not any(implied(r, by) for by in races)]


def _s(stream):
    return f'{stream:#x}' if isinstance(stream, int) else str(stream)


def describe(log, finding):
    """One line naming both launches, their layers and streams."""
    if isinstance(finding, ReadonlyWrite):
        e = log[finding.index]
        return (f'#{finding.index} {e.name} [{e.label}] on stream {_s(e.stream)} writes [{finding.lo:#x}, {finding.hi:#x}), '
                'bytes that existed before the forward (weights / inputs are read-only)')
    a, b = log[finding.first], log[finding.second]
    return (f'{finding.kind} on [{finding.lo:#x}, {finding.hi:#x}): #{finding.first} {a.name} [{a.label}] on stream {_s(a.stream)} and '
            f'#{finding.second} {b.name} [{b.label}] on stream {_s(b.stream)} are not ordered')


def report(log, findings):
    races, bad = findings
    return '\n'.join(describe(log, f) for f in list(bad) + list(races))


def without(log, index):
    """A copy of the log with one entry taken out (the teeth test: a join removed from the LOG, never from a schedule that runs)."""
    return log[:index] + log[index + 1:]


def joins(log, level_label, stream):
    """Log indices of the waits issued on `stream` (the trunk) while the level `level_label` was running: its join (the fork waits of
    that level are issued on the side stream)."""
    return [i for i, e in enumerate(log) if isinstance(e, Wait) and e.stream == stream and e.label.endswith(level_label)]


# ------------------------------------------------------------------------------------------------------------------ role table
# entry point (without its _bf16 / _f16 suffix) -> ((argument index, role), ...).  Roles: 'r' input, 'w' output, 'rw' updated in
# place (og_upsample2_add's and og_conv3x3_tiled_up2's `up`, og_bias_act's y), 's' scratch (extent = the byte count that follows the
# pointer: one buffer per (engine, branch), split-K slabs and tickets, written and read back inside the launch).
# Extents of 'r' / 'w' / 'rw' come from the STORAGE of the tensor whose pointer _lib.ptr handed out (address, nbytes), not from the
# shape arguments: a kernel that strays inside its tensor's storage is the exact tests' business, one that touches bytes another
# stream owns is this one's.  og_conv1x1_heads takes its outputs as a table of raw pointers that never passes _lib.ptr: their extents
# are computed from the arguments (N * channels[i] * H * W fp32), see _heads_outputs.
_CONV5 = ((0, 'r'), (1, 'r'), (2, 'r'), (3, 'r'), (4, 'w'))
ROLES = {
    'og_stem7x7': ((0, 'r'), (1, 'r'), (2, 'r'), (3, 'w')),
    'og_nchw_f32_to_nhwc': ((0, 'r'), (1, 'w')),
    'og_conv3x3': _CONV5 + ((11, 's'),),
    'og_conv3x3_tiled': _CONV5 + ((11, 's'),),
    'og_conv3x3_tiled_up2': ((0, 'r'), (1, 'r'), (2, 'r'), (3, 'r'), (4, 'rw'), (11, 's')),
    'og_conv3x3s2_tiled': _CONV5,
    'og_conv2d': _CONV5 + ((13, 's'),),
    'og_conv2d_proj': _CONV5 + ((17, 's'),),
    'og_conv_band': ((0, 'r'), (1, 'r'), (2, 'r'), (3, 'r'), (4, 'r'), (5, 'w')),
    'og_conv1x1_tiled': ((0, 'r'), (5, 'r'), (10, 'r'), (11, 'r'), (12, 'r'), (13, 'w')),
    'og_conv1x1_heads': ((0, 'r'), (2, 'r'), (3, 'r')),
    'og_upsample2_add': ((0, 'rw'), (1, 'r')),
    'og_bias_act': ((0, 'rw'), (1, 'r'), (2, 'r')),
    'og_nhwc_bf16_to_nchw_f32': ((0, 'r'), (4, 'r'), (5, 'w')),
    'og_nhwc_f16_to_nchw_f32': ((0, 'r'), (4, 'r'), (5, 'w')),
    'og_conv3x3_pack_w16': ((0, 'r'), (4, 'w')),
    'og_conv_band_pack_w16': ((0, 'r'), (1, 'r'), (5, 'w')),
}
# calls that launch nothing: shape questions, and og_conv_next_weights_hint, which stores (pointer, size) on the host for the next
# launch to touch -- a read of packed weights, which are read-only to every launch
HOST_ONLY = {'og_abi_version', 'og_last_error', 'og_device_count', 'og_conv3x3_workspace_bytes', 'og_conv3x3_workspace_bytes_nhw',
             'og_conv2d_workspace_bytes', 'og_conv2d_proj_workspace_bytes', 'og_conv_band_supported', 'og_conv3x3_tiled_supported',
             'og_conv3x3s2_tiled_supported', 'og_conv3x3_tiled_workspace_bytes', 'og_conv_next_weights_hint'}


def stem_of(name):
    for suffix in ('_bf16', '_f16'):
        if name.endswith(suffix) and name[:-len(suffix)] in ROLES:
            return name[:-len(suffix)]
    return name


def _value(p):
    """Address in a ctypes pointer argument (None / c_void_p(0) -> 0)."""
    return (getattr(p, 'value', p) or 0) if p is not None else 0


def _heads_outputs(a):
    n, h, w, count = a[4], a[5], a[6], a[8]
    return tuple((a[10][i], a[10][i] + n * a[9][i] * h * w * 4) for i in range(count))


def launch_entry(name, a, extents, label=''):
    """The Launch of one library call: name (with or without dtype suffix), its ctypes arguments (stream last), extents: address ->
    (lo, hi) of the storage behind every pointer that _lib.ptr handed out."""
    stem = stem_of(name)
    if stem not in ROLES:
        raise AssertionError(f'{name}: the engine called an entry point that has no row in engine_schedule.ROLES')
    reads, writes, scratch = [], [], []
    for i, role in ROLES[stem]:
        p = _value(a[i])
        if not p:
            continue
        if role == 's':
            scratch.append((p, p + int(a[i + 1])))
            continue
        if p not in extents:
            raise AssertionError(f'{name}: argument {i} ({p:#x}) did not come from _lib.ptr: its storage is unknown')
        if 'r' in role:
            reads.append(extents[p])
        if 'w' in role:
            writes.append(extents[p])
    if stem == 'og_conv1x1_heads':
        writes += _heads_outputs(a)
    return Launch(_value(a[-1]), stem, tuple(reads), tuple(writes), tuple(scratch), label)


# -------------------------------------------------------------------------------------------------------------------- recorder
_NO_KERNEL = ('empty', 'new_empty', 'detach', 'alias', 'lift_fresh', 'is_', 'sym_', 'size', 'stride', 'numel', 'dim', 'storage_offset',
              'record_stream', '_local_scalar_dense')


def named_parts(layers):
    """-> ({id(level): 'kps.0.low2'}, {address: conv name}) for an engine's _Layers bundle: the _Level objects by their path, and
    every tensor a launch of a layer may be handed (raw / tiled / band / concatenated weights, bias) -> that layer's module name."""
    from offsetguided_amd.models import engine as E
    levels, tensors, seen = {}, {}, set()

    def walk(o, path):
        if id(o) in seen:
            return
        seen.add(id(o))
        if isinstance(o, E._Conv):
            for attr in ('w', 'w_tiled', 'w_band', 'w_alt', 'b32'):
                t = getattr(o, attr, None)
                if t is not None and t.is_cuda:
                    tensors.setdefault(t.data_ptr(), o.name if o.name != 'Conv2d' else path)
        elif isinstance(o, (list, tuple)):
            for i, v in enumerate(o):
                walk(v, f'{path}.{i}')
        elif isinstance(o, (E._Level, E._Residual)):
            if isinstance(o, E._Level):
                levels[id(o)] = path
            for k, v in vars(o).items():
                if not k.startswith('_'):
                    walk(v, f'{path}.{k}')
    for field in ('pre', 'kps', 'cnvs', 'inters', 'inters_', 'cnvs_', 'hm', 'off', 'scale', 'jitter'):
        walk(getattr(layers, field), field)
    for name, t in (('stem', layers.stem_w), ('heads', (getattr(layers, 'heads_tiled', None) or (None,))[0])):
        if t is not None:
            tensors.setdefault(t.data_ptr(), name)
    return levels, tensors


def preexisting_ranges(device):
    """(lo, hi) of every block the caching allocator holds as allocated right now."""
    import torch
    out = []
    for seg in torch.cuda.memory_snapshot():
        if seg['device'] != (device.index or 0):
            continue
        at = seg['address']
        for blk in seg['blocks']:
            if blk['state'].startswith('active'):
                out.append((at, at + blk['size']))
            at += blk['size']
    return out


class Recorder:
    """rec = Recorder(monkeypatch, layers); with rec.recording(device): engine.forward_raw(x) -> rec.log, rec.readonly.
    Patches (through pytest's monkeypatch, undone with it): every entry point of the loaded library, _lib.ptr (storage extents),
    torch.cuda.Stream.wait_event / wait_stream, torch.cuda.Event.record, models.engine._Level.__call__ (which level is running: the
    label of a join).  Nothing is logged outside `recording`."""

    def __init__(self, monkeypatch, layers):
        import torch

        from offsetguided_amd import _lib
        from offsetguided_amd.models import engine as E
        self.log, self.readonly, self.on = [], [], False
        self.extents, self.levels, self.stack, self.layers = {}, {}, [], layers
        self.tensors = {}
        self._keep, self._event_ids = [], {}
        lib = _lib.load()
        rec = self

        def wrap(name, fn):
            def call(*a):
                if rec.on and name not in HOST_ONLY:
                    rec.log.append(launch_entry(name, a, rec.extents, rec._label(a)))
                return fn(*a)
            if getattr(fn, 'records_conv_launch', False):        # conv_exact.record_launches may sit underneath or on top
                call.records_conv_launch = True
            return call
        for name in _lib.SIGNATURES:
            monkeypatch.setattr(lib, name, wrap(name, getattr(lib, name)))
        orig_ptr = _lib.ptr

        def ptr(t):
            if rec.on:
                st = t.untyped_storage()
                rec.extents[t.data_ptr()] = (st.data_ptr(), st.data_ptr() + st.nbytes())
            return orig_ptr(t)
        monkeypatch.setattr(_lib, 'ptr', ptr)

        record, wait_event, wait_stream = torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream

        def ev_record(ev, stream=None):
            if rec.on:
                s = stream if stream is not None else torch.cuda.current_stream()
                rec.log.append(Record(s.cuda_stream, rec._event(ev, new=True), rec._where()))
            return record(ev, stream) if stream is not None else record(ev)

        def st_wait_event(st, ev):
            if rec.on:
                rec.log.append(Wait(st.cuda_stream, rec._event(ev), rec._where()))
            return wait_event(st, ev)

        def st_wait_stream(st, other):
            before = len(rec.log)
            out = wait_stream(st, other)                 # torch's own is record_event + wait_event: logged by the two patches above
            if rec.on and len(rec.log) == before:        # (a torch whose wait_stream does not go through them)
                ev = ('wait_stream', before)
                rec.log += [Record(other.cuda_stream, ev, rec._where()), Wait(st.cuda_stream, ev, rec._where())]
            return out
        monkeypatch.setattr(torch.cuda.Event, 'record', ev_record)
        monkeypatch.setattr(torch.cuda.Stream, 'wait_event', st_wait_event)
        monkeypatch.setattr(torch.cuda.Stream, 'wait_stream', st_wait_stream)
        level_call = E._Level.__call__

        def call_level(level, x):
            rec.stack.append(id(level))
            try:
                return level_call(level, x)
            finally:
                rec.stack.pop()
        monkeypatch.setattr(E._Level, '__call__', call_level)
        self._issuer = E._issuer

    def _event(self, ev, new=False):
        """(id, generation): an event recorded again is a new point in time; the object is kept so that its id is not reused."""
        if id(ev) not in self._event_ids:
            self._keep.append(ev)
            self._event_ids[id(ev)] = 0
        if new:
            self._event_ids[id(ev)] += 1
        return (id(ev), self._event_ids[id(ev)])

    def _where(self):
        if self.stack and self.stack[-1] not in self.levels:
            self.levels, self.tensors = named_parts(self.layers)
        return f'engine {self._issuer.engine} {self.levels.get(self.stack[-1], "?") if self.stack else "top"}'

    def _label(self, a):
        ptrs = [_value(p) for p in a[:-1] if p is None or hasattr(p, 'value')]
        for attempt in (0, 1):
            name = next((self.tensors[p] for p in ptrs if p in self.tensors), None)
            if name is not None or attempt:
                break
            self.levels, self.tensors = named_parts(self.layers)       # weights packed since the last look
        return f'{self._where()}: {name or "merge / layout pass"}'

    def recording(self, device):
        import contextlib

        import torch
        rec = self

        @contextlib.contextmanager
        def ctx():
            torch.cuda.synchronize(device)
            if not rec.log:
                rec.readonly = preexisting_ranges(device)
            rec.on = True
            try:
                with _torch_ops(rec):
                    yield rec
            finally:
                rec.on = False
        return ctx()


def _torch_ops(rec):
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    from torch.utils._pytree import tree_leaves

    def extent(t):
        st = t.untyped_storage()
        return (st.data_ptr(), st.data_ptr() + st.nbytes())

    class _TorchOps(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            kwargs = kwargs or {}
            out = func(*args, **kwargs)
            name = func._schema.name.split('::')[-1]
            if not rec.on or name.startswith(_NO_KERNEL):
                return out
            schema = func._schema.arguments
            named = list(zip(schema, args)) + [(s, kwargs[s.name]) for s in schema if s.name in kwargs]
            ins = [t for _, v in named for t in tree_leaves(v) if isinstance(t, torch.Tensor) and t.is_cuda]
            mutated = [t for s, v in named if s.alias_info is not None and s.alias_info.is_write
                       for t in tree_leaves(v) if isinstance(t, torch.Tensor) and t.is_cuda]
            theirs = {extent(t) for t in ins}
            fresh = [t for t in tree_leaves(out) if isinstance(t, torch.Tensor) and t.is_cuda and extent(t) not in theirs]
            if not mutated and not fresh:                 # a view
                return out
            dev = (mutated + fresh + ins)[0].device
            rec.log.append(Launch(torch.cuda.current_stream(dev).cuda_stream, f'torch.{name}', tuple(extent(t) for t in ins),
                                  tuple(extent(t) for t in mutated + fresh), (), rec._where() + ': torch op'))
            return out
    return _TorchOps()
