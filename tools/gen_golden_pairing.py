#!/usr/bin/env python3
"""Generate tests/golden/pairing_edges.npz by running the IMPORTED reference's LimbsCollect.generate_limbs on the directed scenes of
tests/pairing_cases.py (planted peaks, dyadic stride-4 maps: distance ties, border peaks, guide points in (-1, 0) and beyond the
image, sub-threshold candidates, K on both sides of 32 and 64).

Per case the reference sees the planted heat maps at input resolution and the torch-CPU x4 upsamples of the stride-4 maps (bilinear
offsets and jitter maps; the scale maps once bicubic, once bilinear), as tools/gen_golden.py builds them.  Stored: its top-k lists,
its limbs (column-major, (13,N,L,K): the columns compress far better apart) and the sha256 of the inputs.  The scale cases share the
scene of the plain case of the same K -- asserted here: their limbs are the plain case's except columns 11 / 12, which are stored for both resize modes.  Asserted on the spot: the C oracle reproduces
lists and limbs (EXACT_LIMB_COLS bit for bit, the score within SCORE_TOL) from the hi-res and from the stride-4 maps, and every
coverage count of pairing_cases.conditions is >= 1.  The archive is written with fixed zip time stamps: a second run gives the same
bytes.

Size: the fixture must stay below the largest other file of tests/golden (tests/test_pairing_cpu.py asserts it) and is about 3 % under
it -- thanks to the LZMA members, the column-major limbs and the shared scale scenes; np.savez cannot rewrite it.  A new case does
not fit as arrays: it goes to pairing_cases.DIGEST (below).

The cases of pairing_cases.DIGEST (the fallback K, scale head on 4-component offsets, scale and jitter heads together, the 44-limb
skeleton past K = 7) do not fit as arrays.  For them the same assertions hold on the spot -- reference == oracle on lists and limbs,
every coverage count >= 1 -- and what is stored is the SHA-256 of the reference's lists and of its EXACT_LIMB_COLS bytes (per resize
mode of the scale maps) plus the counts; pairing_cases.load recomputes the oracle's rows and holds them to those digests.  The cases
with a scale head share the scene of the head-less (or jitter-only) case of the same K: all but columns 11 / 12 is asserted equal, so
the loader takes every other column, the score included, from that case's stored reference limbs; columns 11 / 12 of the cases of
pairing_cases.SCALES_STORED are stored as arrays besides.
The members of the archive that was there before are asserted unchanged.

Needs the reference checkout (OG_REFERENCE); the GPU machine never sees it.   usage: python tools/gen_golden_pairing.py
"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

SCORE_TOL = 1e-4


def save_npz(path, arrays):
    """An .npz archive with fixed time stamps (reproducible bytes), LZMA members (np.load reads them through zipfile like deflated ones)."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_LZMA) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_LZMA
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    import torch
    import oracle
    import pairing_cases as pc
    from helpers import EXACT_LIMB_COLS
    from tools import gen_golden as G
    torch.set_num_threads(8)
    decoder = G.load_reference()
    up = lambda x, mode: torch.nn.functional.interpolate(torch.from_numpy(x), scale_factor=4, mode=mode)  # noqa: E731
    out, plain, digests = {'names': np.array([c.name for c in pc.CASES])}, {}, []

    def check(tag, ref, got):
        bad = int((ref[..., EXACT_LIMB_COLS] != got[..., EXACT_LIMB_COLS]).sum())
        ds = float(np.abs(ref[..., 10] - got[..., 10]).max())
        assert bad == 0 and ds <= SCORE_TOL, f'{tag}: {bad} limb fields differ from the reference, score err {ds}'

    path = os.path.join(G.GOLD, 'pairing_edges.npz')
    committed = os.path.join(ROOT, 'tests', 'golden', 'pairing_edges.npz')
    before = dict(np.load(committed)) if os.path.exists(committed) else {}
    for case in pc.CASES:
        sk, K = pc.skeleton(case), case.K
        scene = pc.build(case)
        hm, off_lr, scl_lr, jit_lr = (scene[k] for k in ('hm_hr', 'off_lr', 'scl_lr', 'jit_lr'))
        t_hm, off_hr = torch.from_numpy(hm), up(off_lr, 'bilinear')
        jit_hr = up(jit_lr, 'bilinear') if jit_lr is not None else None
        assert (oracle.bilinear4(off_lr) == off_hr.numpy()).all(), f'{case.name}: bilinear not bit-exact'
        lc = decoder.LimbsCollect(4, 4, topk=K, thre_hmp=pc.THRE, min_len=pc.MIN_LEN, include_jitter_offset=jit_lr is not None,
                                  include_scale=scl_lr is not None, use_jitter_offset=True, skeleton=sk)
        dets = decoder.joint_dets(t_hm, K)
        sc, idx = dets[0].numpy(), dets[1].numpy()
        assert (sc > 0).all(), f'{case.name}: zero filler in a list'
        o_sc, o_idx, _, _ = oracle.nms_topk(hm, K)
        assert (o_sc == sc).all() and (o_idx == idx).all(), f'{case.name}: top-k'
        runs = {}
        for mode in pc.modes(case):
            scl_hr = up(scl_lr, mode) if scl_lr is not None else None
            limbs = lc.generate_limbs(t_hm, jit_hr if jit_hr is not None else [], off_hr.clone(),
                                      scl_hr if scl_hr is not None else [], case.nd).numpy()
            assert limbs.shape == (pc.N_IMAGES, len(sk), K, 13)
            o_scl = None if scl_lr is None else (oracle.bicubic4 if mode == 'bicubic' else oracle.bilinear4)(scl_lr)
            assert o_scl is None or (o_scl == scl_hr.numpy()).all(), f'{case.name}: {mode} scale maps not bit-exact'
            o_jit = None if jit_lr is None else oracle.bilinear4(jit_lr)
            assert o_jit is None or (o_jit == jit_hr.numpy()).all(), f'{case.name}: jitter maps not bit-exact'
            for lowres in (True, False):
                got = oracle.collect_limbs(sc, idx, off_lr if lowres else off_hr.numpy(), lowres, (case.H, case.W), sk, pc.THRE,
                                           pc.MIN_LEN, vector_nd=case.nd, scales_hr=o_scl, jitter_hr=o_jit)
                check(f'{case.name}/{mode}/lowres={lowres}', limbs, got)
            runs[mode] = limbs
        limbs = runs['bicubic' if scl_lr is not None else 'none']
        cnt = pc.counts(case, sc, idx, limbs, off_hr.numpy(), None if jit_hr is None else jit_hr.numpy(),
                        None if scl_lr is None else oracle.bicubic4(scl_lr))
        assert all(v >= 1 for v in cnt.values()), f'{case.name}: a condition the case is built for does not occur: {cnt}'
        in_sha = [G.sha(a) for a in pc.input_arrays(scene)]
        if case in pc.DIGEST:      # one text member for all of them: a zip member of its own per digest would not fit
            digests.append(f"{case.name}/in_sha {','.join(in_sha)}")
            digests.append(f'{case.name}/lists_sha {pc.lists_digest(sc, idx)}')
            for mode, limbs in runs.items():
                digests.append(f"{case.name}/{'limbs' if mode == 'none' else 'limbs_' + mode}_sha {pc.exact_digest(limbs)}")
            digests.append(f"{case.name}/counts {','.join(f'{k}={v}' for k, v in sorted(cnt.items()))}")
            base = (K, case.H, case.nd, case.skeleton, 'jitter' if case.heads == 'both' else 'none')
            if scl_lr is not None:     # the head-less (jitter-only) case of the same scene: all but the scale columns
                p_sc, p_idx, p_limbs = plain[base]
                assert (p_sc == sc).all() and (p_idx == idx).all()
                for mode in runs:
                    assert (np.delete(runs[mode], [11, 12], -1) == np.delete(p_limbs, [11, 12], -1)).all(), case.name
                assert (runs['bicubic'][..., 11:13] != runs['bilinear'][..., 11:13]).any() and (runs['bicubic'][..., 11:13] != 4).all()
                if case.name in pc.SCALES_STORED:      # small enough to sit in the fixture as arrays, like the scale_k* cases
                    for mode in runs:
                        out[f'{case.name}/scales_{mode}'] = np.ascontiguousarray(np.moveaxis(runs[mode][..., 11:13], -1, 0))
            print(f'{case.name}: reference == oracle, coverage {cnt} (digests)')
            continue
        out[f'{case.name}/in_sha'] = np.array(in_sha)
        if scl_lr is None:
            out[f'{case.name}/scores'], out[f'{case.name}/inds'], out[f'{case.name}/limbs'] = sc, idx.astype(np.int32), np.ascontiguousarray(np.moveaxis(limbs, -1, 0))
            plain[(K, case.H, case.nd, case.skeleton, case.heads)] = (sc, idx, limbs)
        else:
            p_sc, p_idx, p_limbs = plain[(K, case.H, case.nd, case.skeleton, 'none')]
            assert (p_sc == sc).all() and (p_idx == idx).all()
            for mode in runs:
                assert (np.delete(runs[mode], [11, 12], -1) == np.delete(p_limbs, [11, 12], -1)).all(), case.name
                out[f'{case.name}/scales_{mode}'] = np.ascontiguousarray(np.moveaxis(runs[mode][..., 11:13], -1, 0))
            assert (runs['bicubic'][..., 11:13] != runs['bilinear'][..., 11:13]).any()
            assert (runs['bicubic'][..., 11:13] != 4).all()
        print(f'{case.name}: reference == oracle, coverage {cnt}')
    out['digests'] = np.array(digests, dtype='S')
    changed = [k for k in before if k != 'names' and not (k in out and np.array_equal(before[k], out[k]))]
    assert not changed, f'members of the committed archive changed: {changed}'
    assert list(out['names'][:len(before.get('names', []))]) == list(before.get('names', []))
    save_npz(path, out)
    print(f'{path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
