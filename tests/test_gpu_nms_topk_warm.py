"""K1 (csrc/nms_topk.hip) in WARM state on the directed planes of tests/nms_topk_cases.py.

The admission threshold, the helper wave, the score histogram and the per-plane slot table of band_topk_kernel are switched on only
when the workspace carries this geometry's magic word, i.e. from the second call with one (planes, H, W, k) on.  Every case here is
therefore called behind a DECOY of its own geometry (peaks of 3.5 in every band: whatever bound or slot leaks from one call into the
next is far above the case's values and drops real peaks), the test reads the magic word back and asserts that the state is warm, and
the case is called twice.  All comparisons are for equality with the C oracle: scores (values and sign bits), flat indices, ys, xs."""
import numpy as np
import pytest
import torch

import oracle
import nms_topk_cases as nc
from offsetguided_amd import _lib, decoder, synth
from helpers import assert_limbs_match
from test_gpu_generate_limbs import SK, run_single, run_three

pytestmark = pytest.mark.gpu
NAMES = [c.name for c in nc.CASES]
PLAIN_NAMES = [c.name for c in nc.CASES if c.pattern in nc.PLAIN_PATTERNS and nc.GEOMS[c.geom].entry == 'nms' and c.k in (32, 5)
               and c.geom in ('g644x256', 'g324x125')]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    _lib.load()
    return torch.device("cuda:0")


def to_dev(x, dev, aligned=True):
    """Device copy of x; aligned=False: a view one float into its storage (16-byte alignment lost, rows still contiguous)"""
    t = torch.from_numpy(np.array(x, dtype=np.float32, order="C"))        # (a copy: the shared case arrays are read-only)
    if aligned:
        return t.to(dev)
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def call(geom, t, k):
    return (decoder.joint_dets_lowres if geom.entry == 'fused' else decoder.joint_dets)(t, k)


def same(got, ref, what=""):
    s, i, ys, xs = (a.cpu().numpy() for a in got)
    rs, ri, ry, rx = ref
    bad = np.argwhere((s != rs) | (i != ri))
    assert np.array_equal(s, rs) and np.array_equal(i, ri), f"{what}: first mismatches (n, c, rank) {bad[:4].tolist()} of {len(bad)}"
    assert np.array_equal(np.signbit(s), np.signbit(rs)), f"{what}: sign bits"
    assert np.array_equal(ys, ry) and np.array_equal(xs, rx), f"{what}: ys / xs"


def magic_word(dev, planes, H, W, k):
    """The first 8 bytes of the shared top-k workspace, after everything queued has finished"""
    torch.cuda.synchronize()
    nbytes = _lib.load().og_topk_workspace_bytes(planes, H, W, k)
    return int(_lib.workspace(dev, nbytes, "topk")[:8].view(torch.int64).item())


def warm_up(dev, case, planes):
    """The decoy call of the case's geometry; afterwards the workspace carries the geometry's magic word."""
    geom = nc.GEOMS[case.geom]
    call(geom, to_dev(nc.decoy(case.geom, case.k, planes), dev, geom.aligned), case.k)
    assert magic_word(dev, planes, geom.H, geom.W, case.k) != 0, "the workspace is not warm after a call of this geometry"


@pytest.mark.parametrize("name", NAMES)
def test_warm_case(dev, name):
    case = nc.BY_NAME[name]
    geom = nc.GEOMS[case.geom]
    x = nc.build(name)
    ref = nc.reference(name)
    t = to_dev(x, dev, geom.aligned)
    warm_up(dev, case, x.shape[1])
    same(call(geom, t, case.k), ref, "first call behind the decoy")
    assert magic_word(dev, x.shape[1], geom.H, geom.W, case.k) != 0
    same(call(geom, t, case.k), ref, "second call")


@pytest.mark.parametrize("name", PLAIN_NAMES)
def test_plain_topk_cold_and_warm(dev, name):
    """og_topk_channel_f32 on the planes that mean something without the NMS (all equal, the tie, the clamped ranges, the overflow
    lattice): exact behind an NMS call that left the workspace warm and again behind itself, and it leaves the magic word zero."""
    case = nc.BY_NAME[name]
    geom = nc.GEOMS[case.geom]
    x = nc.build(name)
    ref = nc.reference_plain(name)
    t = to_dev(x, dev)
    warm_up(dev, case, x.shape[1])
    for rep in range(2):
        same(decoder.topK_channel(t, K=case.k), ref, f"plain call {rep}")
        assert magic_word(dev, x.shape[1], geom.H, geom.W, case.k) == 0, "plain top-k must invalidate the slot-table state"
    same(call(geom, t, case.k), nc.reference(name), "the NMS call behind plain top-k (cold)")


# ---------------------------------------------------------------------------------- sequences
def _tiled(plane, c):
    """(1, c, H, W): the plane rolled down by 8 rows per channel (the lattice step: peaks stay isolated)"""
    return np.ascontiguousarray(np.stack([np.roll(plane, 8 * j, axis=0) for j in range(c)])[None])


@pytest.mark.parametrize("planes", [1, 3, 17])
def test_loud_then_quiet(dev, planes):
    """One geometry, one workspace: peaks >= 3.75 (bin 255), then peaks < 2^-30 (bin 0), and again.  Whatever the loud call leaves
    behind -- a slot, a bound, a histogram bin -- is above everything the quiet call holds."""
    k = 32
    six = nc.build('g644x256_k32_p6')
    loud, quiet = _tiled(six[0, 1], planes), _tiled(six[0, 0], planes)
    assert loud[loud > 0].min() >= 2.0 and quiet.max() <= 2.0 ** -20
    refs = [oracle.nms_topk(loud, k), oracle.nms_topk(quiet, k)]
    ts = [to_dev(loud, dev), to_dev(quiet, dev)]
    for rep in range(2):
        for j in (0, 1):
            same(decoder.joint_dets(ts[j], k), refs[j], f"{'loud' if j == 0 else 'quiet'} call, round {rep}")
            assert magic_word(dev, planes, 644, 256, k) != 0


def test_entries_alternate_on_one_geometry(dev):
    """og_upsample_nms_topk_f32 and og_nms_topk_f32 share a magic word on one (planes, H, W, k): each runs warm behind the other."""
    k = 32
    lo = [nc.build('f161x64_k32_p4'), nc.build('f161x64_k32_p7')]
    hi = [oracle.bicubic4(x) for x in lo]
    refs = [nc.reference('f161x64_k32_p4'), nc.reference('f161x64_k32_p7')]
    t_lo, t_hi = [to_dev(x, dev) for x in lo], [to_dev(x, dev) for x in hi]
    decoder.joint_dets(to_dev(oracle.bicubic4(nc.decoy('f161x64', k, 2)), dev), k)
    for step in range(6):
        j = step % 2
        assert magic_word(dev, 2, 644, 256, k) != 0
        if step % 3 == 0:
            same(decoder.joint_dets_lowres(t_lo[j], k), refs[j], f"fused, step {step}")
            same(decoder.joint_dets(t_hi[1 - j], k), refs[1 - j], f"unfused behind fused, step {step}")
        else:
            same(decoder.joint_dets(t_hi[j], k), refs[j], f"unfused, step {step}")
            same(decoder.joint_dets_lowres(t_lo[1 - j], k), refs[1 - j], f"fused behind unfused, step {step}")


def test_state_invalidation(dev):
    """A plain top-k call and a call of another geometry in between each leave the next NMS call exact, warm or not."""
    name, other = 'g644x256_k32_p7', 'g324x125_k32_p2'
    case = nc.BY_NAME[name]
    t, ref = to_dev(nc.build(name), dev), nc.reference(name)
    t_o, ref_o = to_dev(nc.build(other), dev), nc.reference(other)
    warm_up(dev, case, 2)
    same(decoder.joint_dets(t, 32), ref, "warm")
    z = synth.noise_batch(5, (1, 2, 644, 256))
    same(decoder.topK_channel(to_dev(z, dev), K=32), oracle.topk(z, 32), "plain top-k of the same geometry")
    assert magic_word(dev, 2, 644, 256, 32) == 0
    same(decoder.joint_dets(t, 32), ref, "behind plain top-k (cold)")
    same(decoder.joint_dets(t, 32), ref, "warm again")
    same(decoder.joint_dets(t_o, 32), ref_o, "another geometry (cold)")
    same(decoder.joint_dets(t, 32), ref, "behind another geometry (cold)")
    same(decoder.joint_dets(t_o, 32), ref_o, "the other geometry behind it (cold)")
    same(decoder.joint_dets(t_o, 32), ref_o, "the other geometry, warm")
    same(decoder.joint_dets(t, 32), ref, "and back")


# ---------------------------------------------------------------------------------- through the descriptor
@pytest.mark.parametrize("name", ['g644x256_k32_p4', 'g644x256_k32_p7'])
def test_descriptor_tail_warm(dev, name):
    """og_generate_limbs_f32 (band kernel + merge_collect_kernel) in warm state: 17 planes that cycle through the case's planes."""
    lib = _lib.load()
    k, n, c, H, W = 32, 1, 17, 644, 256
    x = nc.build(name)
    hr = np.ascontiguousarray(x[:, [j % x.shape[1] for j in range(c)]])
    off = (synth.noise_batch(11, (n, 2 * len(SK), H // 4, W // 4)) * 8).astype(np.float32)
    t_hr, t_off = to_dev(hr, dev), to_dev(off, dev)
    rs, ri, _, _ = oracle.nms_topk(hr, k)
    ws = torch.zeros(lib.og_generate_limbs_workspace_bytes(n, c, H, W, k), dtype=torch.uint8, device=dev)
    run_single(to_dev(nc.decoy('g644x256', k, c), dev), t_off, k, dev, ws=ws)
    torch.cuda.synchronize()
    assert int(ws[65536:65544].view(torch.int64).item()) != 0, "the descriptor's top-k workspace is not warm"
    l3, s3, i3 = run_three(t_hr, t_off, k, dev)
    for rep in range(2):
        limbs, sc, ix, _ = run_single(t_hr, t_off, k, dev, ws=ws)
        assert np.array_equal(sc.cpu().numpy(), rs) and np.array_equal(ix.cpu().numpy(), ri), rep
        assert torch.equal(s3, sc) and torch.equal(i3, ix)
        assert torch.equal(limbs.view(torch.int32), l3.view(torch.int32)), rep                 # same bits, NaN rows included
    ref = oracle.collect_limbs(rs, ri, off, True, (H, W), SK, 0.04, 0.5)
    assert_limbs_match(ref, limbs.cpu().numpy(), 1e-4)


# ---------------------------------------------------------------------------------- refusals
def test_refusals_leave_outputs_untouched(dev):
    """Each refusal comes before any accepted call of its geometry, returns its code, writes nothing; the next accepted call is exact."""
    lib = _lib.load()
    st = _lib.stream_ptr(dev)

    def raw(entry, t, planes, H, W, k, ws, nbytes, ws_off=0):
        s = torch.full((planes, k), -7.0, device=dev)
        i = torch.full((planes, k), -7, dtype=torch.int64, device=dev)
        rc = getattr(lib, entry)(_lib.ptr(t), planes, H, W, k, _lib.ptr(s), _lib.ptr(i), ws.data_ptr() + ws_off, nbytes, st)
        torch.cuda.synchronize()
        return rc, s, i

    def untouched(s, i):
        return bool((s == -7.0).all()) and bool((i == -7).all())

    big = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    assert big.data_ptr() % 16 == 0
    for entry, cases in (("og_nms_topk_f32", [((2, 3), 7, _lib.OG_EINVAL, b"out of range"),        # k > H * W
                                              ((12, 20), 61, _lib.OG_EINVAL, b"border")]),         # k > 2 (H + W) - 4
                         ("og_topk_channel_f32", [((2, 3), 7, _lib.OG_EINVAL, b"out of range")])):
        for (H, W), k, code, word in cases:
            z = synth.noise_batch(61, (1, 1, H, W))
            rc, s, i = raw(entry, to_dev(z, dev), 1, H, W, k, big, big.numel())
            assert rc == code and word in lib.og_last_error() and untouched(s, i), (entry, H, W, k)
    H, W, k = 92, 44, 9                                            # a geometry no other test uses
    z = np.abs(synth.noise_batch(62, (1, 2, H, W)))
    t = to_dev(z, dev)
    need = lib.og_topk_workspace_bytes(2, H, W, k)
    assert 0 < need < big.numel() - 8
    rc, s, i = raw("og_nms_topk_f32", t, 2, H, W, k, big, need - 1)
    assert rc == _lib.OG_ENOSPC and b"workspace" in lib.og_last_error() and untouched(s, i)
    rc, s, i = raw("og_nms_topk_f32", t, 2, H, W, k, big, need, ws_off=4)
    assert rc == _lib.OG_EINVAL and b"aligned" in lib.og_last_error() and untouched(s, i)
    assert int(big.view(torch.int64).abs().sum()) == 0, "a refused call wrote into the workspace"
    rs, ri, _, _ = oracle.nms_topk(z, k)
    for rep in range(2):                                           # accepted: cold, then warm
        rc, s, i = raw("og_nms_topk_f32", t, 2, H, W, k, big, need)
        assert rc == _lib.OG_OK
        assert np.array_equal(s.cpu().numpy(), rs[0]) and np.array_equal(i.cpu().numpy(), ri[0]), rep
