"""The four kernels of csrc/encoder.hip (heat maps + background, jitter, guiding offsets + person scales, keypoint scales) held
to the reference across flags, skeletons and shapes: the sweep fixture (tests/golden/encoder_sweep.npz), a seeded fuzz against
the C oracle (itself held to the reference on the fixture by tests/test_encoder_sweep.py), the raw entry points for what the
Python wrapper never sends, and the layout the training step consumes.

Offsets, keypoint scales, person scales and jitter are bit-exact; bg == 1 - hm.max(0) exactly against the kernel's own heat map;
heat maps within 1e-6 of the reference with at most 2 cells per image on the other side of the clip threshold
(test_encoder.heatmaps_match).  Every output buffer starts filled with a canary no encoder can produce, so a cell a kernel
skips cannot pass by luck."""
import numpy as np
import pytest
import torch

from offsetguided_amd.config import coco_data as cd
from encoder_sweep_common import (CANARY, FUZZ_SEEDS, SWEEP_CASES, case_params, fuzz_config, heatmap_figures, load_sweep,
                                  oracle_outputs, skeleton_of)
from test_encoder import heatmaps_match

pytestmark = pytest.mark.gpu


@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    return torch.device("cuda:0")


class _CanaryTorch:
    """`torch` as the encoder wrapper sees it, with empty() handing out canary-filled memory."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(size, dtype=None, device=None):
        return torch.full(size, CANARY if dtype == torch.float32 else 0xA5, dtype=dtype, device=device)


def configured_encoders(monkeypatch, prm):
    """HeatMaps / OffsetMaps of a case; the class-level settings go through monkeypatch and leave with the test."""
    from offsetguided_amd import encoder
    from offsetguided_amd.encoder import factory
    for k, v in dict(include_jitter_offset=True, include_background=True, n_keypoints=17, keypoints=cd.COCO_KEYPOINTS,
                     sigma=prm["sigma"], clip_thre=prm["clip"], fill_jitter_size=prm["fill_jitter"]).items():
        monkeypatch.setattr(encoder.HeatMaps, k, v)
    for k, v in dict(include_scale=True, skeleton=skeleton_of(prm["head"]), fill_scale_size=prm["fill_scale"],
                     min_jscale=prm["min_jscale"]).items():
        monkeypatch.setattr(encoder.OffsetMaps, k, v)
    monkeypatch.setattr(factory, "torch", _CanaryTorch())
    size = [prm["in_w"], prm["in_h"]]
    return encoder.HeatMaps(size, prm["stride"]), encoder.OffsetMaps(size, prm["stride"])


def padded_batch(images, pad=2):
    """(N, P, 17, 4) + n_persons: rows behind an image's persons hold labelled garbage that n_persons must mask."""
    P = max(max(j.shape[0] for j in images), 1) + pad
    batch = np.full((len(images), P, 17, 4), 7.0, np.float32)
    for n, j in enumerate(images):
        batch[n, :j.shape[0]] = j
    return batch, np.array([j.shape[0] for j in images], np.int32)


def assert_image_matches(got, ref, prm, tag):
    """One image: got / ref = (hm, bg, jit, off, sc, ps) numpy with ref's bg ignored (the kernel's own heat map defines it)."""
    hm, bg, jit, off, sc, ps = got
    r_hm, _, r_jit, r_off, r_sc, r_ps = ref
    worst, edge = heatmap_figures(hm, r_hm, prm["clip"])
    print(f"{tag}: heat-map worst error {worst:.3e}, {edge} clip-edge cells")
    assert heatmaps_match(hm, r_hm, prm["clip"]), (tag, worst, edge)
    assert np.array_equal(bg[0], 1 - hm.max(0)), tag
    assert np.array_equal(jit, r_jit), tag
    assert np.array_equal(off, r_off), tag
    assert np.array_equal(ps, r_ps), tag
    assert np.array_equal(sc, r_sc, equal_nan=True), tag


def assert_empty_image(got, tag):
    hm, bg, jit, off, sc, ps = got
    assert (hm == 0).all() and (bg == 1).all() and np.isposinf(jit).all() and np.isposinf(off).all(), tag
    assert np.isnan(sc).all() and (ps == 1).all(), tag


def encode(hm_enc, off_enc, batch, n_persons):
    hm, bg, jit, mask = hm_enc.encode_batch(batch, n_persons)
    off, sc, ps, mask2 = off_enc.encode_batch(batch, n_persons)
    n, h, w = batch.shape[0], hm_enc.input_size[1] // hm_enc.stride, hm_enc.input_size[0] // hm_enc.stride
    assert mask.dtype == torch.bool and bool(mask.all()) and mask.shape == (n, 1, h, w) and bool(mask2.all())
    assert hm.shape == (n, 17, h, w) and bg.shape == (n, 1, h, w) and jit.shape == (n, 2, h, w)
    L = len(off_enc.skeleton)
    assert off.shape == ps.shape == (n, 2 * L, h, w) and sc.shape == (n, 17, h, w)
    return [t.cpu().numpy() for t in (hm, bg, jit, off, sc, ps)]


@pytest.mark.parametrize("case", SWEEP_CASES)
def test_gpu_encoder_matches_reference_sweep(case, dev, monkeypatch):
    g = load_sweep()
    j, prm = g[f"{case}_joints"], case_params(g, case)
    hm_enc, off_enc = configured_encoders(monkeypatch, prm)
    # batch of 3: the case, the case with its persons reversed and padded (n_persons masks the padding), no person
    batch, n_persons = padded_batch([j, j[::-1], j[:0]])
    out = encode(hm_enc, off_enc, batch, n_persons)
    ref = (g[f"{case}_hm"], None, g[f"{case}_jitter"], g[f"{case}_off"], g[f"{case}_scale"], g[f"{case}_pscale"])
    assert_image_matches([t[0] for t in out], ref, prm, f"sweep {case}")
    _, r_jit, r_off, r_sc, r_ps = oracle_outputs(j[::-1], prm)
    assert_image_matches([t[1] for t in out], (ref[0], None, r_jit, r_off, r_sc, r_ps), prm, f"sweep {case} reversed")   # max: order-free
    assert_empty_image([t[2] for t in out], case)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_gpu_encoder_fuzz_matches_oracle(seed, dev, monkeypatch):
    prm, images = fuzz_config(seed)
    tag = f"fuzz seed {seed} {prm} persons {[j.shape[0] for j in images]}"
    print(tag)
    hm_enc, off_enc = configured_encoders(monkeypatch, prm)
    batch, n_persons = padded_batch(images, pad=seed % 3)
    out = encode(hm_enc, off_enc, batch, n_persons)
    for n, j in enumerate(images):
        hm, jit, off, sc, ps = oracle_outputs(j, prm)
        assert_image_matches([t[n] for t in out], (hm, None, jit, off, sc, ps), prm, f"{tag} image {n}")


# ---- the raw entry points ------------------------------------------------------------------------------------------------
TAIL = 256     # canary floats behind every output buffer
RAW_PRM = dict(in_w=76, in_h=52, stride=4, sigma=7, clip=0.01, fill_jitter=3, fill_scale=7, min_jscale=1.0, head="omp")   # 19 x 13 cells
KEYS = ("hm", "bg", "jit", "off", "sc", "ps")


class _Raw:
    """The three entry points on buffers of the test's own: each output is a canary-filled tensor with TAIL more floats than
    the entry point may write, so a write past the end lands in memory the test owns and is seen."""

    def __init__(self, dev, prm, N):
        from offsetguided_amd import _lib
        self._lib, self.lib, self.dev, self.prm, self.N = _lib, _lib.load(), dev, prm, N
        sk = skeleton_of(prm["head"])
        L = self.L = len(sk)
        self.jf = torch.tensor([a for a, _ in sk], dtype=torch.int32, device=dev)
        self.jt = torch.tensor([b for _, b in sk], dtype=torch.int32, device=dev)
        self.sig = torch.tensor(cd.COCO_PERSON_SIGMAS, dtype=torch.float32, device=dev)
        h, w = prm["in_h"] // prm["stride"], prm["in_w"] // prm["stride"]
        self.shapes = dict(hm=(N, 17, h, w), bg=(N, 1, h, w), jit=(N, 2, h, w), off=(N, 2 * L, h, w), sc=(N, 17, h, w),
                           ps=(N, 2 * L, h, w))
        self.fresh()

    def fresh(self):
        self.buf = {k: torch.full((int(np.prod(s)) + TAIL,), CANARY, dtype=torch.float32, device=self.dev)
                    for k, s in self.shapes.items()}

    def call(self, joints, n_persons, P, only=(1, 1, 1), **over):
        """-> the return codes of (heat maps, jitter, offsets); 0 for an entry point `only` leaves out.  `over` replaces
        arguments by name; a pointer replaced by None is passed as NULL."""
        p = dict(self.prm, joints=joints, jf=self.jf, jt=self.jt, sig=self.sig, n_kp=17, N=self.N, **self.buf)
        p.update(over)
        q = lambda t: None if t is None else self._lib.ptr(t)  # noqa: E731
        lib, st, rc = self.lib, self._lib.stream_ptr(self.dev), [0, 0, 0]
        if only[0]:
            rc[0] = lib.og_encode_heatmaps_f32(q(p["joints"]), q(n_persons), p["N"], P, p["n_kp"], p["in_w"], p["in_h"], p["stride"],
                                               p["sigma"], p["clip"], q(p["hm"]), q(p["bg"]), st)
        if only[1]:
            rc[1] = lib.og_encode_jitter_f32(q(p["joints"]), q(n_persons), p["N"], P, p["n_kp"], p["in_w"], p["in_h"], p["stride"],
                                             p["fill_jitter"], q(p["jit"]), st)
        if only[2]:
            rc[2] = lib.og_encode_offsets_f32(q(p["joints"]), q(n_persons), p["N"], P, p["n_kp"], q(p["jf"]), q(p["jt"]), self.L,
                                              p["in_w"], p["in_h"], p["stride"], p["fill_scale"], p["min_jscale"], q(p["sig"]),
                                              q(p["off"]), q(p["sc"]), q(p["ps"]), st)
        torch.cuda.synchronize(self.dev)
        return tuple(rc)

    def outputs(self, skipped=()):
        """The outputs as numpy, after checking every tail; a skipped output must still be all canary, the others hold none."""
        out = {}
        for k, s in self.shapes.items():
            a = self.buf[k].cpu().numpy()
            assert (a[-TAIL:] == CANARY).all(), f"{k}: written past its end"
            out[k] = a[:-TAIL].reshape(s)
            if k in skipped:
                assert (out[k] == CANARY).all(), f"{k}: written although NULL was passed"
            else:
                assert not (out[k] == CANARY).any(), f"{k}: cells the kernels never wrote"
        return out

    def untouched(self):
        return all(bool((b == CANARY).all()) for b in self.buf.values())


def _raw_batch(dev):
    """(2, 6, 17, 4): six persons; their first three followed by three rows of labelled garbage."""
    from encoder_sweep_common import fuzz_joints
    from offsetguided_amd import synth
    j = fuzz_joints(synth.HashRng(4242), 6, RAW_PRM["in_w"], RAW_PRM["in_h"], 4, 1.0)
    batch, _ = padded_batch([j, j[:3]], pad=0)
    return batch, torch.from_numpy(batch).to(dev)


def _image(out, n):
    return [out[k][n] for k in KEYS]


def _oracle_ref(j):
    hm, jit, off, sc, ps = oracle_outputs(j, RAW_PRM)
    return hm, None, jit, off, sc, ps


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def test_raw_n_persons_clamped_and_null(dev):
    batch, joints = _raw_batch(dev)
    raw = _Raw(dev, RAW_PRM, 2)
    P = batch.shape[1]
    assert raw.call(joints, torch.tensor([P, P], dtype=torch.int32, device=dev), P) == (0, 0, 0)
    ref = raw.outputs()
    for n in range(2):       # all P rows of either image, the garbage rows of image 1 included
        assert_image_matches(_image(ref, n), _oracle_ref(batch[n]), RAW_PRM, f"raw image {n}")
    raw.fresh()              # n_persons[n] > P is clamped to P
    assert raw.call(joints, torch.tensor([P + 5, 2 ** 30], dtype=torch.int32, device=dev), P) == (0, 0, 0)
    assert _same(raw.outputs(), ref)
    raw.fresh()              # n_persons == NULL: all P rows
    assert raw.call(joints, None, P) == (0, 0, 0)
    assert _same(raw.outputs(), ref)
    raw.fresh()              # and a count below P masks the rows behind it
    assert raw.call(joints, torch.tensor([P, 3], dtype=torch.int32, device=dev), P) == (0, 0, 0)
    got = raw.outputs()
    assert_image_matches(_image(got, 1), _oracle_ref(batch[1, :3]), RAW_PRM, "raw image 1, 3 persons")
    assert all(np.array_equal(got[k][0], ref[k][0], equal_nan=True) for k in KEYS)


def test_raw_optional_outputs_null(dev):
    batch, joints = _raw_batch(dev)
    raw = _Raw(dev, RAW_PRM, 2)
    P = batch.shape[1]
    assert raw.call(joints, None, P) == (0, 0, 0)
    ref = raw.outputs()
    raw.fresh()
    assert raw.call(joints, None, P, bg=None, sc=None) == (0, 0, 0)
    got = raw.outputs(skipped=("bg", "sc"))      # their buffers were not passed: all canary; every tail intact
    assert all(np.array_equal(got[k], ref[k]) for k in ("hm", "jit", "off", "ps"))


def test_raw_no_persons(dev):
    batch, joints = _raw_batch(dev)
    raw = _Raw(dev, RAW_PRM, 2)
    for n_persons in (None, torch.tensor([3, 0], dtype=torch.int32, device=dev)):      # P == 0 bounds n_persons too
        raw.fresh()
        assert raw.call(joints, n_persons, 0) == (0, 0, 0)
        got = raw.outputs()
        for n in range(2):
            assert_empty_image(_image(got, n), f"P == 0, image {n}")


def test_raw_bad_arguments_launch_nothing(dev):
    from offsetguided_amd import _lib
    batch, joints = _raw_batch(dev)
    raw = _Raw(dev, RAW_PRM, 2)
    P = batch.shape[1]
    E = _lib.OG_EINVAL
    bad = [
        (dict(joints=None), (E, E, E)),
        (dict(hm=None), (E, 0, 0)), (dict(jit=None), (0, E, 0)), (dict(off=None), (0, 0, E)), (dict(ps=None), (0, 0, E)),
        (dict(jf=None), (0, 0, E)), (dict(jt=None), (0, 0, E)), (dict(sig=None), (0, 0, E)),
        (dict(clip=0.0), (E, 0, 0)), (dict(clip=1.0), (E, 0, 0)), (dict(clip=-0.25), (E, 0, 0)), (dict(clip=1.5), (E, 0, 0)),
        (dict(clip=float("nan")), (E, 0, 0)),
        (dict(stride=0), (E, E, E)), (dict(in_w=3), (E, E, E)), (dict(in_h=3), (E, E, E)), (dict(N=0), (E, E, E)),
        (dict(sigma=0), (E, 0, 0)), (dict(fill_jitter=0), (0, E, 0)), (dict(fill_scale=0), (0, 0, E)),
    ]
    for over, want in bad:   # only the entry points the bad argument reaches are called: none of them may launch anything
        args = dict(over)
        rc = raw.call(args.pop("joints", joints), None, P, only=want, **args)
        assert rc == want, (over, rc)
        assert raw.untouched(), over
    # 4 * n_kp floats (one person's joints of a channel round) no longer fit the heat-map kernel's staging buffer: refused
    # before any launch, so the too-small joints buffer is never read
    assert raw.call(joints, None, 0, only=(1, 0, 0), n_kp=1025) == (_lib.OG_EUNSUPPORTED, 0, 0)
    assert raw.untouched() and b"og_encode_heatmaps_f32" in raw.lib.og_last_error()


# ---- the layout the training step consumes -----------------------------------------------------------------------------------
def test_encode_targets_training_layout(dev, monkeypatch):
    """train_dist.encode_targets with factory_heads(['hmp', 'omp44'], ...) on a non-default square length: the annos of the
    training step equal the oracle's maps for the same annotations."""
    from offsetguided_amd import encoder, train_dist
    prm = dict(in_w=192, in_h=192, stride=4, sigma=7, clip=0.01, fill_jitter=3, fill_scale=7, min_jscale=1.0, head="omp")
    configured_encoders(monkeypatch, prm)            # the defaults, and factory_head's class-level writes leave with the test
    encs = encoder.factory_heads(["hmp", "omp44"], 192, [4, 4], dev)
    assert encoder.OffsetMaps.skeleton == cd.DENSER_COCO_PERSON_SKELETON and encs[0].input_size == [192, 192]
    prm["head"] = "omp44"
    from encoder_sweep_common import fuzz_joints
    from offsetguided_amd import synth
    rng = synth.HashRng(31337)
    images = [fuzz_joints(rng, n, 192, 192, 4, 1.0) for n in (7, 0, 19)]
    batch, n_persons = padded_batch(images)
    (hm, bg, jit, mask), (off, sc, ps, mask2) = train_dist.encode_targets(encs, torch.from_numpy(batch).to(dev),
                                                                          torch.from_numpy(n_persons).to(dev))
    assert hm.shape == (3, 17, 48, 48) and off.shape == ps.shape == (3, 88, 48, 48) and sc.shape == (3, 17, 48, 48)
    assert mask is not None and mask.dtype == torch.bool and bool(mask.all()) and mask.shape == (3, 1, 48, 48)
    assert all(t.is_cuda and t.dtype == torch.float32 for t in (hm, bg, jit, off, sc, ps))
    out = [t.cpu().numpy() for t in (hm, bg, jit, off, sc, ps)]
    for n, j in enumerate(images):
        r_hm, r_jit, r_off, r_sc, r_ps = oracle_outputs(j, prm)
        assert_image_matches([t[n] for t in out], (r_hm, None, r_jit, r_off, r_sc, r_ps), prm, f"training layout image {n}")
    assert_empty_image([t[1] for t in out], "training layout, empty image")
