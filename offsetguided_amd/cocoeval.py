"""COCO keypoint AP without pycocotools: COCOeval's iouType='keypoints' protocol (pycocotools/cocoeval.py: computeOks, evaluateImg,
accumulate, summarize) with the OKS of every (detection, ground truth) pair and the greedy matching of every (image, area range,
threshold) as two HIP launches (csrc/oks.hip, include/og_decoder.h) and the precision / recall accumulation in numpy.

    gt = load_ground_truth('person_keypoints_val2017.json')
    ev = KeypointEval(gt)
    ev.evaluate(*run_images(args, loader))          # the result dicts and image ids run_images returns
    ev.summarize()                                  # COCOeval's ten lines; -> stats (10)

Pinned: the specification, restated in numpy with straight loops in tests/cocoeval_common.py.  Not pinned: pycocotools itself (absent
from the build) and the device's double exp against libm beyond 1e-12.  There is no CPU path: without a HIP device evaluate raises.
"""
import ctypes as C
import json

import numpy as np
import torch

from . import _lib
from .config.coco_data import COCO_PERSON_SIGMAS

K = 17
MAX_DETS = 20
IOU_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1)
REC_THRS = np.linspace(0.0, 1.0, int(np.round((1.0 - 0.0) / 0.01)) + 1)
AREA_RANGES = np.array([[0.0, 1e10], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]])
AREA_NAMES = ('all', 'medium', 'large')
# summarize(): (average precision?, IoU threshold or None, area range), COCOeval._summarizeKps
SUMMARY = ((True, None, 0), (True, 0.5, 0), (True, 0.75, 0), (True, None, 1), (True, None, 2),
           (False, None, 0), (False, 0.5, 0), (False, 0.75, 0), (False, None, 1), (False, None, 2))


def load_ground_truth(annotation_file):
    """The person annotations of a COCO keypoint file, per image and in file order:
    {image_id: {'keypoints' (g, 17, 3) float64, 'area' (g,) float64, 'bbox' (g, 4) float64, 'iscrowd' (g,) uint8, 'num_keypoints' (g,)
    int64}}.  Every image of the file's `images` list has an entry (g may be 0)."""
    return {image_id: annotation_arrays(anns) for image_id, anns in person_annotations(annotation_file)[1].items()}


def person_annotations(annotation_file):
    """The parsing load_ground_truth and data.load_annotations share: (the file's `images` list, {image_id: its person annotation
    dicts in file order}); every image of the list has an entry."""
    with open(annotation_file) as f:
        data = json.load(f)
    rows = {im['id']: [] for im in data.get('images', [])}
    for ann in data.get('annotations', []):
        if ann.get('category_id', 1) == 1:
            rows.setdefault(ann['image_id'], []).append(ann)
    return data.get('images', []), rows


def annotation_arrays(anns):
    """One image's person annotation dicts -> the arrays of load_ground_truth's entry."""
    kp = np.array([a['keypoints'] for a in anns], np.float64).reshape(len(anns), K, 3)
    return {
        'keypoints': kp,
        'area': np.array([a['area'] for a in anns], np.float64),
        'bbox': np.array([a['bbox'] for a in anns], np.float64).reshape(len(anns), 4),
        'iscrowd': np.array([a.get('iscrowd', 0) for a in anns], np.uint8),
        'num_keypoints': np.array([a.get('num_keypoints', int((k[:, 2] > 0).sum())) for a, k in zip(anns, kp)], np.int64),
    }


def _device():
    if not torch.cuda.is_available():
        raise _lib.OgError('cocoeval: the OKS and matching kernels need a HIP device (offsetguided_amd has no CPU path)')
    return torch.device('cuda', torch.cuda.current_device())


def _sigmas(sigmas):
    s = np.ascontiguousarray(sigmas, np.float64)
    if s.shape != (K,):
        raise ValueError(f'sigmas: expected {K} values, got shape {s.shape}')
    return s


class _Pack:
    """Arrays laid out in one pinned host buffer (16-byte aligned sections, every one at least 16 bytes so that no device pointer is
    null) and copied to the device in one transfer."""

    def __init__(self, arrays):
        self.offsets, total = [], 0
        for arr in arrays:
            self.offsets.append(total)
            total += max(16, -(-arr.nbytes // 16) * 16)
        self.host = torch.zeros(total, dtype=torch.uint8).pin_memory()
        view = self.host.numpy()
        for arr, off in zip(arrays, self.offsets):
            view[off:off + arr.nbytes] = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        self.dev = None

    def to(self, device):
        self.dev = self.host.to(device, non_blocking=True)
        base = self.dev.data_ptr()
        return [C.c_void_p(base + off) for off in self.offsets]


def _launch_oks(lib, dev, ptrs, sigmas, n_images, n_dets, n_gts, n_pairs):
    """ptrs: device pointers of (dets, gts, gt_area, gt_bbox, det_off, gt_off, pair_off) -> oks, a (max(n_pairs, 2),) double tensor."""
    oks = torch.empty(max(n_pairs, 2), dtype=torch.float64, device=dev)
    _lib.check(lib.og_oks_matrix_f64(*ptrs, sigmas.ctypes.data_as(C.c_void_p), n_images, n_dets, n_gts, n_pairs, _lib.ptr(oks),
                                     _lib.stream_ptr(dev)), lib)
    return oks


def oks_matrix(dets, gts, area, bbox, sigmas=COCO_PERSON_SIGMAS):
    """OKS of one image's detections (d, 17, 3) against its ground truths (g, 17, 3) with `area` (g,) and `bbox` (g, 4) [x, y, w, h]:
    a (d, g) float64 tensor on the device (og_oks_matrix_f64).  d is at most 64."""
    dev = _device()
    dets = np.asarray(dets, np.float64).reshape(-1, K, 3)
    gts = np.asarray(gts, np.float64).reshape(-1, K, 3)
    area, bbox = np.asarray(area, np.float64).reshape(-1), np.asarray(bbox, np.float64).reshape(-1, 4)
    d, g = len(dets), len(gts)
    if len(area) != g or len(bbox) != g:
        raise ValueError(f'oks_matrix: {g} ground truths, {len(area)} areas, {len(bbox)} boxes')
    if d > 64:
        raise ValueError(f'oks_matrix: at most 64 detections per image, got {d}')
    pack = _Pack([dets, gts, area, bbox, np.array([0, d], np.int32), np.array([0, g], np.int32), np.array([0, d * g], np.int64)])
    oks = _launch_oks(_lib.load(), dev, pack.to(dev), _sigmas(sigmas), 1, d, g, d * g)
    return oks[:d * g].reshape(d, g)


class KeypointEval:
    """COCOeval(gt, dt, iouType='keypoints') on the device.  ground_truth: load_ground_truth()'s dict (an image id without an entry
    has no ground truth).  After evaluate(): precision (T, R, A), recall (T, A), stats (10), and for tests oks (the packed OKS values),
    dt_match (A, T, D), dt_ignore (A, T, D), gt_ignore_a (A, G) and the offset tables det_off / gt_off / pair_off."""

    def __init__(self, ground_truth, sigmas=COCO_PERSON_SIGMAS):
        self.ground_truth = ground_truth
        self.sigmas = _sigmas(sigmas)
        self.iou_thrs, self.rec_thrs, self.area_ranges, self.max_dets = IOU_THRS, REC_THRS, AREA_RANGES, MAX_DETS
        self.precision = self.recall = self.stats = None
        self._oks_dev = self._oks = None

    @property
    def oks(self):
        """The packed OKS values (image i's d_i x g_i block at pair_off[i]) as a numpy array; copied from the device on first use."""
        if self._oks is None and self._oks_dev is not None:
            self._oks = self._oks_dev[:int(self.pair_off[-1])].cpu().numpy()
        return self._oks

    def _pack(self, results, image_ids):
        by_image = {}
        for r in results:
            by_image.setdefault(r['image_id'], []).append(r)
        ids = list(dict.fromkeys(image_ids))
        dets, scores, gt_rows = [], [], []
        det_off, gt_off = [0], [0]
        for image_id in ids:
            rs = by_image.get(image_id, [])
            sc = np.array([r['score'] for r in rs], np.float64)
            order = np.argsort(-sc, kind='mergesort')[:self.max_dets]
            dets += [rs[j]['keypoints'] for j in order]
            scores.append(sc[order])
            gt = self.ground_truth.get(image_id)
            if gt is not None and len(gt['area']):
                gt_rows.append(gt)
            det_off.append(det_off[-1] + len(order))
            gt_off.append(gt_off[-1] + (len(gt['area']) if gt is not None else 0))
        dets = np.array(dets, np.float64).reshape(-1, K, 3)
        cat = lambda key, shape, dtype: (np.concatenate([np.asarray(g[key], dtype).reshape((-1,) + shape) for g in gt_rows])    # noqa: E731
                                         if gt_rows else np.zeros((0,) + shape, dtype))
        gts, area, bbox = cat('keypoints', (K, 3), np.float64), cat('area', (), np.float64), cat('bbox', (4,), np.float64)
        crowd = (cat('iscrowd', (), np.int64) != 0).astype(np.uint8)
        ignore = ((crowd != 0) | (cat('num_keypoints', (), np.int64) == 0)).astype(np.uint8)
        det_area = ((dets[:, :, 0].max(1) - dets[:, :, 0].min(1)) * (dets[:, :, 1].max(1) - dets[:, :, 1].min(1))
                    if len(dets) else np.zeros(0))
        det_off, gt_off = np.array(det_off, np.int32), np.array(gt_off, np.int32)
        pair_off = np.concatenate(([0], np.cumsum(np.diff(det_off).astype(np.int64) * np.diff(gt_off)))).astype(np.int64)
        self.image_ids, self.scores = ids, np.concatenate(scores) if scores else np.zeros(0)
        self.det_off, self.gt_off, self.pair_off = det_off, gt_off, pair_off
        return [dets, gts, area, bbox, det_off, gt_off, pair_off, ignore, crowd, det_area]

    def evaluate(self, results, image_ids):
        """results, image_ids: what evaluate.run_images returns.  Only the images named in image_ids are scored (params.imgIds), in that
        order, a repeated id once.  One pinned buffer, one H2D copy, og_oks_matrix_f64 + og_oks_match_i32, one D2H copy, then numpy.
        -> self."""
        dev = _device()
        lib = _lib.load()
        arrays = self._pack(results, image_ids)
        n_images, n_dets, n_gts, n_pairs = len(self.image_ids), int(self.det_off[-1]), int(self.gt_off[-1]), int(self.pair_off[-1])
        A, T = len(self.area_ranges), len(self.iou_thrs)
        self._oks = None
        if n_images == 0:
            self._oks_dev = None
            self.dt_match, self.dt_ignore = np.zeros((A, T, 0), np.int32), np.zeros((A, T, 0), np.uint8)
            self.gt_ignore_a = np.zeros((A, 0), np.uint8)
            return self._accumulate()
        pack = _Pack(arrays)
        p = pack.to(dev)
        st = _lib.stream_ptr(dev)
        self._oks_dev = _launch_oks(lib, dev, p[:7], self.sigmas, n_images, n_dets, n_gts, n_pairs)
        # the three outputs in one device buffer (dt_match first: int32 alignment), so that one copy brings them back
        n_m, n_i, n_g = 4 * A * T * n_dets, A * T * n_dets, A * n_gts
        out = torch.zeros(max(n_m + n_i + n_g, 16), dtype=torch.uint8, device=dev)
        ws_bytes = lib.og_oks_match_workspace_bytes(n_gts, A, T)
        ws = _lib.workspace(dev, ws_bytes, tag='oks_match')
        ranges, thrs = np.ascontiguousarray(self.area_ranges, np.float64), np.ascontiguousarray(self.iou_thrs, np.float64)
        base = out.data_ptr()
        _lib.check(lib.og_oks_match_i32(_lib.ptr(self._oks_dev), p[4], p[5], p[6], p[2], p[7], p[8], p[9],
                                        ranges.ctypes.data_as(C.c_void_p), A, thrs.ctypes.data_as(C.c_void_p), T, n_images, n_dets, n_gts,
                                        n_pairs, C.c_void_p(base), C.c_void_p(base + n_m), C.c_void_p(base + n_m + n_i), _lib.ptr(ws),
                                        ws_bytes, st), lib)
        host = out.cpu().numpy()               # (waits for the stream: the pinned input buffer may go after this)
        self.dt_match = host[:n_m].view(np.int32).reshape(A, T, n_dets).copy()
        self.dt_ignore = host[n_m:n_m + n_i].reshape(A, T, n_dets).copy()
        self.gt_ignore_a = host[n_m + n_i:n_m + n_i + n_g].reshape(A, n_gts).copy()
        return self._accumulate()

    def _accumulate(self):
        """COCOeval.accumulate for one category and one maxDets, then the ten summary figures."""
        A, T, R = len(self.area_ranges), len(self.iou_thrs), len(self.rec_thrs)
        self.precision, self.recall = -np.ones((T, R, A)), -np.ones((T, A))
        # an image with neither detections nor ground truth contributes nothing (evaluateImg returns None): it has no entries anyway
        order = np.argsort(-self.scores, kind='mergesort')
        nd = len(order)
        eps = np.spacing(1)
        for a in range(A):
            npig = int(np.count_nonzero(self.gt_ignore_a[a] == 0))
            if npig == 0:
                continue
            for t in range(T):
                dtm, dtig = self.dt_match[a, t][order], self.dt_ignore[a, t][order]
                tp = np.cumsum((dtm != 0) & (dtig == 0)).astype(np.float64)
                fp = np.cumsum((dtm == 0) & (dtig == 0)).astype(np.float64)
                rc = tp / npig
                pr = tp / (fp + tp + eps)
                self.recall[t, a] = rc[-1] if nd else 0.0
                pr = np.maximum.accumulate(pr[::-1])[::-1]            # non-increasing from the right
                inds = np.searchsorted(rc, self.rec_thrs, side='left')
                q = np.zeros(R)
                ok = inds < nd
                q[ok] = pr[inds[ok]]
                self.precision[t, :, a] = q
        self.stats = np.array([self._figure(*row) for row in SUMMARY])
        return self

    def _figure(self, ap, iou_thr, a):
        s = self.precision[:, :, a] if ap else self.recall[:, a]
        if iou_thr is not None:
            s = s[np.where(iou_thr == self.iou_thrs)[0]]
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    def summarize(self):
        """Print COCOeval's ten keypoint lines; -> stats."""
        if self.stats is None:
            raise RuntimeError('KeypointEval.summarize: call evaluate() first')
        for (ap, iou_thr, a), value in zip(SUMMARY, self.stats):
            iou = ('{:0.2f}:{:0.2f}'.format(self.iou_thrs[0], self.iou_thrs[-1]) if iou_thr is None else '{:0.2f}'.format(iou_thr))
            print(' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'.format(
                'Average Precision' if ap else 'Average Recall', '(AP)' if ap else '(AR)', iou, AREA_NAMES[a], self.max_dets, value))
        return self.stats
