#!/usr/bin/env python3
"""How close the JPEG round trip's specification (csrc/jpeg_sim.hip, restated in tests/photometric_common.py) is to PIL's: PSNR figures on
the two structured 64 x 64 images of the CPU test, written to profiles/photometric_parity.json.  CPU only.  Per image: the restatement
against PIL's quality-50 4:2:0 round trip, that round trip against the original (the loss itself, which the former must exceed:
tests/test_photometric_cpu.py asserts it), and PIL at quality 40 and 60 against PIL at 50 -- what one step of the quality scale is
worth, recorded for comparison, not asserted.

    python tools/photometric_parity.py [--out profiles/photometric_parity.json]"""
import argparse
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def pil_roundtrip(image, quality):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(image).save(f, 'jpeg', quality=quality, subsampling=2)          # 2 = 4:2:0
    return np.asarray(Image.open(f).convert('RGB'))


def figures():
    import PIL
    import photometric_common as pc
    rows = []
    for image in pc.structured_images():
        p50, rest = pil_roundtrip(image, 50), pc.jpeg_roundtrip(image, 50)
        rows.append({'psnr_restatement_vs_pil_q50': round(pc.psnr(rest, p50), 2), 'psnr_pil_q50_vs_original': round(pc.psnr(p50, image), 2),
                     'psnr_restatement_vs_original': round(pc.psnr(rest, image), 2),
                     'psnr_pil_q40_vs_pil_q50': round(pc.psnr(pil_roundtrip(image, 40), p50), 2),
                     'psnr_pil_q60_vs_pil_q50': round(pc.psnr(pil_roundtrip(image, 60), p50), 2)})
    return {'metric': 'jpeg_roundtrip_parity', 'unit': 'dB (PSNR over 64 x 64 x 3 bytes)', 'pil_version': PIL.__version__,
            'subsampling': '4:2:0', 'images': rows}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'photometric_parity.json'))
    a = ap.parse_args()
    line = json.dumps(figures())
    print(line)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
