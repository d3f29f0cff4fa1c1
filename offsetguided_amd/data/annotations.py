"""COCO keypoint annotations for training: the file with its segmentations (load_annotations), the (P,17,4) keypoint array of
transforms/annotations.py:41-63 (normalize_annotations) and the packed tables og_coco_masks_u8 rasterises mask_miss / mask_all from
(mask_tables; layout: OgCocoImage / OgCocoAnn / OgCocoPiece of include/og_decoder.h)."""
import math

import numpy as np

from ..cocoeval import annotation_arrays, person_annotations
from ..config.coco_data import COCO_KEYPOINTS, COCO_PERSON_SIGMAS

IMAGE_DT = np.dtype([('out_off', '<i8'), ('h', '<i4'), ('w', '<i4'), ('ann_first', '<i4'), ('n_anns', '<i4')])
ANN_DT = np.dtype([('piece_first', '<i4'), ('n_pieces', '<i4'), ('flags', '<i4'), ('reserved', '<i4')])
PIECE_DT = np.dtype([('word_off', '<i8'), ('image', '<i4'), ('kind', '<i4'), ('first', '<i4'), ('count', '<i4')])
POLYGON, RLE = 0, 1
CROWD, MISS = 1, 2


def load_annotations(annotation_file):
    """The person annotations of a COCO keypoint file with their segmentations, per image in the order of the file's `images` list and,
    inside an image, in file order: {image_id: record}, record = cocoeval.load_ground_truth's arrays ('keypoints' (g,17,3), 'area',
    'bbox', 'iscrowd', 'num_keypoints') + 'segmentation' (a list of g entries: a list of polygons [x0, y0, x1, y1, ...] or an RLE dict
    {'size': [h, w], 'counts': list or compressed string}) + 'image_id', 'file_name', 'height', 'width' and the file's 'image' entry."""
    images, rows = person_annotations(annotation_file)
    info = {im['id']: im for im in images}
    out = {}
    for image_id, anns in rows.items():
        im = info.get(image_id, {})
        record = annotation_arrays(anns)
        record.update(segmentation=[a.get('segmentation', []) for a in anns], image_id=image_id, file_name=im.get('file_name'),
                      height=im.get('height'), width=im.get('width'), image=im)
        out[image_id] = record
    return out


def normalize_annotations(anns):
    """NormalizeAnnotations.normalize_annotations (transforms/annotations.py:41-63) for a load_annotations record: the non-crowd
    annotations with keypoints -> (P,17,4) fp32 rows [x, y, v, scale], scale = sqrt(bbox_w bbox_h) sigmas, v = 0 when area <= 32 * 32."""
    keep = [i for i in range(len(anns['area'])) if anns['iscrowd'][i] == 0 and anns['num_keypoints'][i] > 0]
    keypoints = np.zeros((len(keep), len(COCO_KEYPOINTS), 4), dtype=np.float32)
    for row, i in enumerate(keep):
        keypoints[row, :, :3] = np.asarray(anns['keypoints'][i], dtype=np.float32).reshape(-1, 3)
        scale = math.sqrt(anns['bbox'][i][-1] * anns['bbox'][i][-2])
        keypoints[row, :, 3] = scale * np.array(COCO_PERSON_SIGMAS)
        if anns['area'][i] <= 32 * 32:
            keypoints[row, :, 2] = 0
    return keypoints


def rle_counts(counts):
    """Run lengths of an RLE's `counts`: a list passes through; a compressed string is decoded as maskApi's rleFrString does -- 5 payload
    bits per character at ord - 48, bit 0x20 continues, bit 0x10 of the last group is the sign, and from the third count on the value
    is a delta to the count two back."""
    if not isinstance(counts, (str, bytes)):
        return [int(c) for c in counts]
    data = counts.encode('ascii') if isinstance(counts, str) else counts
    runs, p = [], 0
    while p < len(data):
        x, k, more = 0, 0, True
        while more:
            if p >= len(data):
                raise ValueError('RLE counts string ends inside a value')
            c = data[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(runs) > 2:
            x += runs[-2]
        runs.append(x)
    return runs


class MaskTables:
    """The packed tables of a batch (one uint8 numpy buffer, sections 16-byte aligned) + what the host knows about the outputs:
    sizes [(h, w)], offsets (byte offset of image i's plane in the packed output), out_bytes."""

    def __init__(self, buffer, counts, at, sizes, offsets, out_bytes):
        self.buffer, self.counts, self.at = buffer, counts, at
        self.sizes, self.offsets, self.out_bytes = sizes, offsets, out_bytes


def _align16(v):
    return (v + 15) // 16 * 16


def mask_tables(records):
    """load_annotations records of a batch of images -> MaskTables.  A polygon list with an odd number of values, an RLE whose size is
    not the image's, or a negative run is a ValueError here; what the library refuses (an empty polygon, a non-finite vertex, runs that
    do not sum to h w) is left to it."""
    images = np.zeros(len(records), IMAGE_DT)
    anns, pieces, vertices, cums = [], [], [], []
    sizes, offsets, out, words, n_vert, n_cum = [], [], 0, 0, 0, 0
    for i, rec in enumerate(records):
        h, w = int(rec['height']), int(rec['width'])
        n = len(rec['area'])
        images[i] = (out, h, w, len(anns), n)
        sizes.append((h, w))
        offsets.append(out)
        out += max(h, 0) * max(w, 0)
        plane = (max(h, 0) * max(w, 0) + 31) // 32
        for j in range(n):
            crowd = int(rec['iscrowd'][j]) == 1
            miss = not crowd and (rec['num_keypoints'][j] <= 0 or rec['area'][j] <= 32 * 32)
            seg = rec['segmentation'][j]
            first = len(pieces)
            if isinstance(seg, dict):
                if [int(v) for v in seg['size']] != [h, w]:
                    raise ValueError(f"image {rec.get('image_id')}: RLE of size {seg['size']} in an image of size {[h, w]}")
                runs = np.asarray(rle_counts(seg['counts']), np.int64)
                if (runs < 0).any() or runs.sum() >= 1 << 32:
                    raise ValueError(f"image {rec.get('image_id')}: RLE with a negative run or beyond 2^32")
                pieces.append((words, i, RLE, n_cum, len(runs)))
                cums.append(np.cumsum(runs).astype(np.uint32))
                n_cum += len(runs)
                words += plane
            else:
                for poly in seg:
                    xy = np.asarray(poly, np.float64).reshape(-1)
                    if len(xy) % 2:
                        raise ValueError(f"image {rec.get('image_id')}: polygon with an odd number of values")
                    pieces.append((words, i, POLYGON, n_vert, len(xy) // 2))
                    vertices.append(xy)
                    n_vert += len(xy) // 2
                    words += plane
            anns.append((first, len(pieces) - first, CROWD if crowd else (MISS if miss else 0), 0))
    sections = [images, np.array(anns, ANN_DT) if anns else np.zeros(0, ANN_DT), np.array(pieces, PIECE_DT) if pieces else np.zeros(0, PIECE_DT),
                np.concatenate(vertices) if vertices else np.zeros(0, np.float64), np.concatenate(cums) if cums else np.zeros(0, np.uint32)]
    at, total = [], 0
    for sec in sections:
        at.append(total)
        total += max(16, _align16(sec.nbytes))
    buffer = np.zeros(total, np.uint8)
    for sec, o in zip(sections, at):
        buffer[o:o + sec.nbytes] = sec.reshape(-1).view(np.uint8)
    return MaskTables(buffer, (len(records), len(anns), len(pieces), n_vert, n_cum), at, sizes, offsets, out)
