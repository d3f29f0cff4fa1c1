"""GPU: the input chain (csrc/preprocess.hip, og_center_pad_normalize_u8 of csrc/epilogue.hip) against the oracle composition of
tests/input_chain_common.py, bit for bit: both tap paths of the fused kernel (the labels are the host restatement of the launcher's
decision; the path itself cannot be observed), the geometry edges of the 64 x 4 tiling, the batch entry against the reference rather
than against the per-image kernel, the mask shrink at every stride, the wrappers, and every refusal.  Shapes are small: targets of at
most 256 per side, large sources only where the scale needs them."""
import ctypes as C

import numpy as np
import pytest
import torch

import input_chain_common as ic
from offsetguided_amd import _lib, transforms
from offsetguided_amd.config import data_mean, data_std

pytestmark = pytest.mark.gpu
GUARD = 4096                     # floats (bytes for uint8 outputs) kept around every output


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    _lib.load()
    return torch.device("cuda:0")


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


MEAN, STD, FILL = _f3(data_mean), _f3(data_std), _f3(transforms.pad.FILL)


def _guarded(dev, numel, dtype=torch.float32):
    """(whole buffer, the output view in its middle): NaN (or 0xA5 for bytes) everywhere."""
    whole = torch.full((numel + 2 * GUARD,), float('nan') if dtype == torch.float32 else 0xA5, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + numel]


def _untouched(t):
    return bool(torch.isnan(t).all()) if t.dtype == torch.float32 else bool((t == 0xA5).all())


def _guards_intact(whole):
    return _untouched(whole[:GUARD]) and _untouched(whole[-GUARD:])


def _first_diff(got, ref):
    bad = np.argwhere((got != ref).numpy().any(axis=0))
    return f'{len(bad)} pixels differ, first (row, col) {bad[:5].tolist()}'


# ------------------------------------------------------------------------------------------------------------ the per-image entry
@pytest.mark.parametrize('kind', ic.KINDS)
def test_per_image_entry_over_the_table(dev, kind):
    """og_rescale_pad_normalize_u8 on every case of the table == resize by the oracle, paste, normalise; ltrb; nothing written
    outside the output.  A failure names the case and its path label."""
    lib = _lib.load()
    failures = []
    for c in ic.CASES:
        src = torch.from_numpy(ic.image(kind, c.h, c.w)).to(dev)
        whole, out = _guarded(dev, 3 * c.TH * c.TW)
        ltrb = (C.c_int * 4)()
        rc = lib.og_rescale_pad_normalize_u8(_lib.ptr(src), c.h, c.w, c.nh, c.nw, c.TH, c.TW, c.corner, MEAN, STD, FILL, _lib.ptr(out), ltrb,
                                             _lib.stream_ptr(dev))
        assert rc == _lib.OG_OK, (c.name, lib.og_last_error())
        ref, ref_ltrb = ic.expected(kind, c.h, c.w, c.nh, c.nw, c.TH, c.TW, c.corner)
        got = out.view(3, c.TH, c.TW).cpu()
        if not torch.equal(got, ref):
            failures.append(f'[{c.label}] {c.name}: {_first_diff(got, ref)}')
        assert list(ltrb) == ref_ltrb, c.name
        assert _guards_intact(whole), c.name
    assert not failures, '\n'.join(failures)


# ----------------------------------------------------------------------------------------------------------------- the batch entry
def _batch(dev, sizes, seeds, kind, TH, TW, corner, poison):
    """One og_rescale_pad_normalize_batch_u8 call on images packed last first with poisoned gaps -> (output on the host, ltrb list)."""
    lib = _lib.load()
    n = len(sizes)
    images = [ic.image(kind, h, w, seed) for (h, w, _, _), seed in zip(sizes, seeds)]
    buf, offsets = ic.pack_reversed(images, poison)
    raw = torch.from_numpy(buf).to(dev)
    offs, hw4, ltrb = (C.c_long * n)(*offsets), (C.c_int * (4 * n))(), (C.c_int * (4 * n))()
    for i, s in enumerate(sizes):
        hw4[4 * i:4 * i + 4] = list(s)
    whole, out = _guarded(dev, n * 3 * TH * TW)
    rc = lib.og_rescale_pad_normalize_batch_u8(_lib.ptr(raw), offs, hw4, n, TH, TW, corner, MEAN, STD, FILL, _lib.ptr(out), ltrb,
                                               _lib.stream_ptr(dev))
    assert rc == _lib.OG_OK, lib.og_last_error()
    got = out.view(n, 3, TH, TW).cpu()
    assert _guards_intact(whole)
    return got, list(ltrb)


def _check_batch(dev, sizes, seeds, labels, kind, TH, TW, corner):
    refs = [ic.expected(kind, h, w, nh, nw, TH, TW, corner, seed) for (h, w, nh, nw), seed in zip(sizes, seeds)]
    for poison in (0x00, 0xFF):                   # a read outside an image cannot agree with the reference under both
        got, ltrb = _batch(dev, sizes, seeds, kind, TH, TW, corner, poison)
        bad = [f'image {i} [{labels[i]}] {sizes[i]}: {_first_diff(got[i], refs[i][0])}' for i in range(len(sizes))
               if not torch.equal(got[i], refs[i][0])]
        assert not bad, f'poison {poison:#x}\n' + '\n'.join(bad)
        assert ltrb == [v for _, r in refs for v in r]


@pytest.mark.parametrize('corner', (0, 1))
def test_batch_entry_mixes_both_paths_in_one_launch(dev, corner):
    """Every pair of the table that fits 250 x 250 in ONE launch: 'lds' and 'direct' images side by side, against the reference."""
    mix = ic.mixed_launch()
    assert len(mix) <= 64 and {m[4] for m in mix} == {'lds', 'direct'}
    _check_batch(dev, [m[:4] for m in mix], [0] * len(mix), [m[4] for m in mix], 'noise', 250, 250, corner)


@pytest.mark.parametrize('kind', ('index', 'salt'))
@pytest.mark.parametrize('corner', (0, 1))
def test_batch_entry_across_the_descriptor_table_boundary(dev, corner, kind):
    """70 images, two launches of 64 and 6 descriptors: images 63, 64 and 65 are a large LDS image, a direct one and a single pixel."""
    sizes = ic.seventy()
    _check_batch(dev, sizes, list(range(70)), [ic.label_of(*s) for s in sizes], kind, 130, 200, corner)      # (sizes repeat: every image its own seed)


# ---------------------------------------------------------------------------------------------------------------- the resize entry
@pytest.mark.parametrize('kind', ic.KINDS)
def test_resize_entry_over_the_table_pairs(dev, kind):
    lib = _lib.load()
    for h, w, nh, nw in ic.pairs():
        src = torch.from_numpy(ic.image(kind, h, w)).to(dev)
        whole, out = _guarded(dev, nh * nw * 3, torch.uint8)
        assert lib.og_resize_cubic_u8(_lib.ptr(src), h, w, _lib.ptr(out), nh, nw, _lib.stream_ptr(dev)) == _lib.OG_OK
        got, ref = out.view(nh, nw, 3).cpu().numpy(), ic.resized(kind, h, w, nh, nw)
        assert np.array_equal(got, ref), f'{(h, w)} -> {(nh, nw)}: first (row, col) {np.argwhere((got != ref).any(2))[:5].tolist()}'
        assert _guards_intact(whole)
    im = ic.image(kind, 17, 31)
    assert np.array_equal(transforms.resize_cubic(im, 70, 128).cpu().numpy(), ic.resized(kind, 17, 31, 70, 128))


# ------------------------------------------------------------------------------------------------------------------ the mask shrink
@pytest.mark.parametrize('N', (1, 3))
def test_mask_shrink_over_strides_sizes_and_greys(dev, N):
    """og_shrink_mask_miss_u8 == oracle.shrink_mask_miss_u8 per plane: strides 1 .. 16, sizes the stride does not divide (exact halves
    round to even), a mask as small as the stride, grey values on both sides of 179, constants 178 / 179 / 180."""
    import oracle
    lib = _lib.load()
    for stride, (h, w), kind in ic.MASK_CASES:
        m = ic.mask(kind, N, h, w)
        ref = np.stack([oracle.shrink_mask_miss_u8(m[n], stride) for n in range(N)])
        nh, nw = ref.shape[1:]
        whole, out = _guarded(dev, N * nh * nw, torch.uint8)
        rc = lib.og_shrink_mask_miss_u8(_lib.ptr(torch.from_numpy(m).to(dev)), N, h, w, stride, _lib.ptr(out), _lib.stream_ptr(dev))
        assert rc == _lib.OG_OK, (stride, h, w, lib.og_last_error())
        got = out.view(N, nh, nw).cpu().numpy()
        assert set(np.unique(got)) <= {0, 1}
        for n in range(N):
            assert np.array_equal(got[n].astype(bool), ref[n]), (stride, h, w, kind, n, np.argwhere(got[n] != ref[n])[:5].tolist())
        assert _guards_intact(whole)
        if N == 3 and not kind.startswith('const'):
            assert not np.array_equal(m[0], m[1]) and not np.array_equal(m[1], m[2])


# -------------------------------------------------------------------------------------------------------------------- centre pad
@pytest.mark.parametrize('tw, th, sizes', [(96, 40, [(40, 96), (1, 1), (17, 31), (40, 1), (1, 96), (39, 95)]),
                                           (70, 130, [(130, 70), (3, 5), (129, 1)]),
                                           (1, 1, [(1, 1)])])
def test_center_pad_normalize_wrapper(dev, tw, th, sizes):
    """CenterPadNormalize((w, h)): a non-square target, images equal to the target, single pixels; the metas' CenterPad updates."""
    images = [ic.image('noise', h, w) for h, w in sizes]
    metas = [{'offset': np.array([0.0, 0.0]), 'valid_area': np.array([0.0, 0.0, w, h])} for h, w in sizes]
    out = transforms.CenterPadNormalize((tw, th), device=dev)(images, metas).cpu()
    assert out.shape == (len(sizes), 3, th, tw)
    for im, got, meta in zip(images, out, metas):
        ref, (left, top, right, bottom) = ic.paste(im, th, tw, 0)
        assert torch.equal(got, ref), im.shape
        assert (left, top, right, bottom) == transforms.center_pad_ltrb(im.shape[1], im.shape[0], tw, th)
        assert tuple(meta['offset']) == (-left, -top) and tuple(meta['valid_area']) == (left, top, im.shape[1], im.shape[0])
        assert tuple(meta['width_height']) == (tw, th)


# ---------------------------------------------------------------------------------------------------------------------- wrappers
WRAPPER_SIZES = [(90, 160), (200, 150), (700, 900)]          # (h, w): landscape, portrait, and a x7 reduction at long edge 128
FIXED_SIZES = [(96, 160), (300, 500), (60, 110)]             # fixed height 128: widths 213, 213, 234 -> all padded to 256


def _check_wrapper_output(out, metas, sizes, T, PH, PW, fixed, ids):
    assert out.shape == (len(sizes), 3, PH, PW)
    got = out.cpu()
    for i, (h, w) in enumerate(sizes):
        tw, th = transforms.rescale_size(w, h, T, fixed)
        ref, ltrb = ic.expected('noise', h, w, th, tw, PH, PW, int(fixed))
        assert torch.equal(got[i], ref), (i, T, ic.label_of(h, w, th, tw))
        m, _ = transforms.rescale_meta(transforms.initial_meta(w, h, ids[i]), None, w, h, tw, th)
        assert np.array_equal(metas[i]['scale'], m['scale']) and np.array_equal(metas[i]['scale'], [(tw - 1) / (w - 1), (th - 1) / (h - 1)])
        assert np.array_equal(metas[i]['offset'], m['offset'] - np.array(ltrb[:2], np.float64))
        assert np.array_equal(metas[i]['offset'], [-ltrb[0], -ltrb[1]])
        assert np.array_equal(metas[i]['valid_area'], [ltrb[0], ltrb[1], w * m['scale'][0], h * m['scale'][1]])
        assert tuple(metas[i]['width_height']) == (PW, PH) and metas[i]['image_id'] == ids[i]


def test_eval_preprocess_wrappers(dev):
    """EvalPreprocess(128), its fixed-height form and multi_scale at (0.5, 1.0, 2.0): tensors against the oracle composition, metas
    against rescale_meta and the reference paddings; four calls each, so the ring of three staging buffers comes round."""
    images = [ic.image('noise', h, w) for h, w in WRAPPER_SIZES]
    assert {ic.label_of(h, w, *transforms.rescale_size(w, h, 128)[::-1]) for h, w in WRAPPER_SIZES} == {'lds', 'direct'}
    pre = transforms.EvalPreprocess(128, device=dev)
    for _ in range(4):
        out, metas = pre(images, image_ids=[3, 4, 5])
        _check_wrapper_output(out, metas, WRAPPER_SIZES, 128, 128, 128, False, [3, 4, 5])
    fixed = transforms.EvalPreprocess(128, device=dev, fixed_height=True)
    fimages = [ic.image('noise', h, w) for h, w in FIXED_SIZES]
    for _ in range(4):
        out, metas = fixed(fimages)
        _check_wrapper_output(out, metas, FIXED_SIZES, 128, 128, 256, True, [None] * 3)
    for _ in range(2):
        res = pre.multi_scale(images, (0.5, 1.0, 2.0), image_ids=[7, 8, 9])
        assert len(res) == 3
        for (out, metas), (T, P) in zip(res, ((64, 128), (128, 128), (256, 256))):
            _check_wrapper_output(out, metas, WRAPPER_SIZES, T, P, P, False, [7, 8, 9])
    out, metas = pre(images[1:2])                                    # and the plain call still works after multi_scale's turn
    _check_wrapper_output(out, metas, WRAPPER_SIZES[1:2], 128, 128, 128, False, [None])


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_are_status_codes_that_leave_the_output_alone(dev):
    """Host-side refusals: OG_EINVAL, the entry's name in og_last_error(), nothing launched -- the prefilled outputs stay as they were."""
    lib = _lib.load()
    st = _lib.stream_ptr(dev)
    src = torch.from_numpy(ic.image('noise', 20, 30)).to(dev)
    whole, out = _guarded(dev, 3 * 3 * 16 * 16)                       # room for the three images of the accepted batch call
    wholeb, outb = _guarded(dev, 3 * 16 * 16, torch.uint8)
    p, o, ob = _lib.ptr(src), _lib.ptr(out), _lib.ptr(outb)

    def refused(rc, name, what):
        assert rc == _lib.OG_EINVAL, (name, what, rc)
        assert name.encode() + b':' in lib.og_last_error(), (name, what, lib.og_last_error())

    def nothing_written(name):
        """After an entry's refusals and BEFORE any accepted call to it: both outputs, guards included, are as they were prefilled."""
        torch.cuda.synchronize()
        assert _untouched(whole) and _untouched(wholeb), name

    name = 'og_rescale_pad_normalize_u8'
    one = lambda **k: lib.og_rescale_pad_normalize_u8(*[k.get(a, d) for a, d in (  # noqa: E731
        ('img', p), ('h', 20), ('w', 30), ('nh', 10), ('nw', 15), ('TH', 16), ('TW', 16), ('corner', 0), ('mean', MEAN), ('std', STD),
        ('fill', FILL), ('out', o), ('ltrb', None), ('st', st))])
    for bad in ({'img': None}, {'mean': None}, {'std': None}, {'fill': None}, {'out': None}, {'h': 0}, {'w': 0}, {'h': -20}, {'w': -1},
                {'nh': 0}, {'nw': 0}, {'nh': -10}, {'nw': 17}, {'nh': 17}, {'TH': 9}, {'TW': 14}, {'TH': 0}, {'TW': -16}):
        refused(one(**bad), name, bad)
    nothing_written(name)
    assert one() == _lib.OG_OK                                        # (the same arguments without the fault are accepted)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[:768]).any()) and _untouched(out[768:])
    out.fill_(float('nan'))

    name = 'og_rescale_pad_normalize_batch_u8'
    good_hw = [20, 30, 10, 15] * 3

    def batch(hw=good_hw, offs=(0, 0, 0), **k):
        a = {'raw': p, 'offs': offs and (C.c_long * 3)(*offs), 'hw4': (C.c_int * 12)(*hw), 'n': 3, 'TH': 16, 'TW': 16, 'corner': 0, 'mean': MEAN,
             'std': STD, 'fill': FILL, 'out': o, 'ltrb': None, 'st': st}
        a.update(k)
        return lib.og_rescale_pad_normalize_batch_u8(*a.values())

    for bad in ({'raw': None}, {'offs': None}, {'hw4': None}, {'mean': None}, {'std': None}, {'fill': None}, {'out': None}, {'n': 0},
                {'n': -3}, {'TH': 0}, {'TW': 0}, {'TH': 9}, {'TW': 14}):
        refused(batch(**bad), name, bad)
    for at, v in ((4, 0), (5, 0), (8, -20), (9, -1), (6, 0), (7, 0), (10, 17), (11, 17), (6, 17), (7, -15)):     # image 1 or 2, never the first
        hw = list(good_hw)
        hw[at] = v
        refused(batch(hw=hw), name, (at, v))
        assert f'image {at // 4}'.encode() in lib.og_last_error(), (at, v, lib.og_last_error())
    refused(batch(offs=(0, 0, -1)), name, 'negative offset')
    assert b'image 2' in lib.og_last_error()
    refused(batch(offs=(0, -1800, 0)), name, 'negative offset')
    nothing_written(name)
    ltrb = (C.c_int * 12)()
    assert batch(ltrb=ltrb) == _lib.OG_OK and list(ltrb) == [0, 3, 1, 3] * 3
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()) and _guards_intact(whole)
    out.fill_(float('nan'))

    name = 'og_resize_cubic_u8'
    for args in ((None, 20, 30, ob, 10, 15), (p, 20, 30, None, 10, 15), (p, 0, 30, ob, 10, 15), (p, 20, 0, ob, 10, 15), (p, -20, 30, ob, 10, 15),
                 (p, 20, 30, ob, 0, 15), (p, 20, 30, ob, 10, 0), (p, 20, 30, ob, 10, -15), (p, 20, 30, ob, -10, 15)):
        refused(lib.og_resize_cubic_u8(*args, st), name, args[1:3] + args[4:])
    nothing_written(name)

    name = 'og_shrink_mask_miss_u8'
    for args in ((None, 1, 20, 30, 4, ob), (p, 1, 20, 30, 4, None), (p, 0, 20, 30, 4, ob), (p, -1, 20, 30, 4, ob), (p, 1, 0, 30, 4, ob),
                 (p, 1, 20, -30, 4, ob), (p, 1, 20, 30, 0, ob), (p, 1, 20, 30, -4, ob),
                 (p, 1, 1, 30, 4, ob), (p, 1, 20, 2, 4, ob), (p, 3, 7, 7, 16, ob)):                                  # stride larger than the mask
        refused(lib.og_shrink_mask_miss_u8(*args, st), name, args[1:5])
    assert b'stride larger than the mask' in lib.og_last_error()
    nothing_written(name)

    name = 'og_center_pad_normalize_u8'
    pad = lambda **k: lib.og_center_pad_normalize_u8(*[k.get(a, d) for a, d in (  # noqa: E731
        ('img', p), ('h', 10), ('w', 15), ('TH', 16), ('TW', 16), ('mean', MEAN), ('std', STD), ('fill', FILL), ('out', o), ('ltrb', None),
        ('st', st))])
    for bad in ({'img': None}, {'mean': None}, {'std': None}, {'fill': None}, {'out': None}, {'h': 0}, {'w': 0}, {'h': -10}, {'w': -15},
                {'h': 17}, {'w': 17}, {'TH': 9}, {'TW': 14}, {'TH': 0}, {'TW': -16}):
        refused(pad(**bad), name, bad)
    nothing_written(name)
