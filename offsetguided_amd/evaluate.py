"""Inference harness with the reference evaluate.py surface (evaluate_cli :49-122, run_images
:125-300, validation :303-328), MI355X-native underneath:

  images -> models.InferenceEngine (fp16 NHWC: the reference's apex-O2 arithmetic, HIP graph) -> decoder.PostProcess.submit (HIP kernels,
  batch i+1's backbone is queued before batch i's poses are collected) -> annotations_inverse ->
  COCO-style result dicts.

COCO data loading is not part of this path: `run_images` takes any iterable of (images, annos, metas)
batches (the reference's collate format, data/factory.py:23-35) and falls back to synthetic batches.
`validation` (and `--score` on the command line) scores the results against args.annotation_file: with
pycocotools when it imports, otherwise -- or with scorer='native' -- with the package's own COCO keypoint
scorer (cocoeval.KeypointEval: OKS and matching as HIP kernels, csrc/oks.hip), which needs no pycocotools.
"""
import argparse
import json
import logging
import os
import time

import numpy as np
import torch

from . import _lib, decoder, models
from .decoder import multiscale
from .utils import AverageMeter

LOG = logging.getLogger(__name__)

ANNOTATIONS_VAL = 'data/link2COCO2017/annotations/person_keypoints_val2017.json'
IMAGE_DIR_VAL = 'data/link2COCO2017/val2017'
ANNOTATIONS_TESTDEV = 'data/link2COCO2017/annotations_trainval_info/image_info_test-dev2017.json'
ANNOTATIONS_TEST = 'data/link2COCO2017/annotations_trainval_info/image_info_test2017.json'
IMAGE_DIR_TEST = 'data/link2COCO2017/test2017/'


def evaluate_cli(argv=None):
    """Same flags as the reference (apex flags are accepted and ignored: bf16 is built in)."""
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    g = parser.add_argument_group('logging')
    g.add_argument('--debug', default=False, action='store_true')
    g.add_argument('-q', '--quiet', default=False, action='store_true')
    models.net_cli(parser)
    decoder.decoder_cli(parser)
    parser.add_argument('--dump-name', default='hourglass104_mi355x', type=str, help='detection file name')
    parser.add_argument('--dataset', choices=('val', 'test', 'test-dev'), default='val')
    parser.add_argument('--batch-size', default=8, type=int)
    parser.add_argument('--long-edge', default=640, type=int, help='long edge of input images')
    parser.add_argument('--fixed-height', action='store_true', default=False)
    parser.add_argument('--flip-test', action='store_true', default=False, help='flip augmentation during testing')
    parser.add_argument('--cat-flip-offset', action='store_true', default=False)
    parser.add_argument('--scored-off', action='store_true', default=False,
                        help='heatmap-weighted refinement of the guiding offsets (generate_poses(scored_off=True); beyond the '
                             'reference command line, which never passes the switch)')
    parser.add_argument('--test-scales', default=[1.0], type=float, nargs='+', metavar='S',
                        help='multi-scale test (beyond the reference): input scales relative to --long-edge whose head outputs are '
                             'averaged on the grid of scale 1 (which must be in the list) and decoded once')
    parser.add_argument('--score', action='store_true', default=False,
                        help='score the results against the annotation file (validation(): COCO keypoint AP / AR; pycocotools when '
                             'it imports, the native scorer cocoeval.KeypointEval otherwise)')
    parser.add_argument('--annotation-file', default=None, type=str,
                        help="COCO keypoint annotations --score reads (default: the --dataset's own file)")
    parser.add_argument('--image-dir', default=None, type=str,
                        help="read the images from this directory (data.CocoKeypoints on the annotation file when it exists, data.ImageList "
                             "of the directory's files otherwise) instead of the synthetic stand-in; decoded by PIL, rescaled, padded and "
                             'normalised on the device')
    parser.add_argument('--loader-workers', default=8, type=int)
    parser.add_argument('--all-images', default=False, action='store_true')
    parser.add_argument('--resume', '-r', action='store_true', default=False, help='load --checkpoint-whole')
    parser.add_argument('--use-ema', action='store_true', default=False,
                        help="with --resume: load the averaged weights of the checkpoint (its ema_state_dict, written by train_dist "
                             '--ema-decay) instead of the raw ones; a checkpoint without them is an error')
    parser.add_argument('--checkpoint-path', '-p', default='link2checkpoints_storage')
    parser.add_argument('--show-detected-poses', action='store_true', default=False,
                        help="paint every batch's poses over the network-input images on the device (visualization.draw_poses) and "
                             'write the first image of each batch to <show-dir>/<dump-name>.poses.<batch>.ppm')
    parser.add_argument('--show-dir', default='.', type=str, help='directory of the --show-* images')
    parser.add_argument('--range-report', default=None, type=str, metavar='FILE',
                        help="count on the device what the engine's 16-bit type does to every layer -- folded weights that overflow, "
                             'flush to zero or go subnormal; activations that are inf, NaN or subnormal over the images actually run '
                             '(engines built with probe=True: a diagnostic mode that reads every activation a second time) -- and '
                             'write the report as JSON to FILE')
    parser.add_argument('--show-hmp-idx', default=None, type=int, metavar='N',
                        help='paint heat-map channel N of the decoded maps over the first image of each batch, raw and after NMS '
                             '(visualization.draw_heatmap): <show-dir>/<dump-name>.hmpN.<batch>.ppm and .hmpN_nms.<batch>.ppm')
    parser.add_argument('--show-limb-idx', default=None, type=int, metavar='N',
                        help='paint the guiding offsets of limb type N as arrows over the (whitened) first image of each batch '
                             '(visualization.draw_offsets): <show-dir>/<dump-name>.limbN.<batch>.ppm')
    parser.add_argument('--show-all-limbs', action='store_true', default=False,
                        help='paint every candidate limb the pairing produced (within --dist-max) over the first image of each batch '
                             '(visualization.draw_limbs): <show-dir>/<dump-name>.limbs.<batch>.ppm')
    g = parser.add_argument_group('apex configuration (accepted for command-line compatibility, unused)')
    g.add_argument('--local_rank', default=0, type=int)
    g.add_argument('--opt-level', type=str, default='O2')
    g.add_argument('--keep-batchnorm-fp32', type=str, default=None)
    g.add_argument('--loss-scale', type=str, default=None)
    g.add_argument('--channels-last', default=False, action='store_true')
    g.add_argument('--print-freq', '-f', default=10, type=int, metavar='N')
    args = parser.parse_args(argv)
    if args.use_ema and not args.resume:
        parser.error('--use-ema loads the averaged weights of a checkpoint: add --resume')
    try:
        validate_test_scales(args.test_scales, args.fixed_height, args.cat_flip_offset)
        validate_views(args)
    except ValueError as e:
        parser.error(str(e))
    args.raw_image_dir = args.image_dir       # only an explicit --image-dir makes run_images read files
    default_dir, annotation_file = {
        'val': (IMAGE_DIR_VAL, ANNOTATIONS_VAL), 'test': (IMAGE_DIR_TEST, ANNOTATIONS_TEST),
        'test-dev': (IMAGE_DIR_TEST, ANNOTATIONS_TESTDEV)}[args.dataset]
    args.image_dir = args.image_dir or default_dir
    args.annotation_file = args.annotation_file or annotation_file
    if args.dataset in ('test', 'test-dev'):
        args.all_images = True
    return args


def validate_test_scales(scales, fixed_height=False, cat_flip_offset=False):
    """--test-scales: positive, no repeats, 1.0 present (its grid and metas are the ones decoded and mapped back); more than one scale
    is not served with --fixed-height or --cat-flip-offset (decoder/multiscale.py).  Raises ValueError."""
    scales = [float(s) for s in scales]
    if not scales:
        raise ValueError('--test-scales: at least one scale')
    if any(not s > 0 for s in scales):
        raise ValueError(f'--test-scales: every scale must be > 0, got {scales}')
    if len(set(scales)) != len(scales):
        raise ValueError(f'--test-scales: duplicate scales in {scales}')
    if 1.0 not in scales:
        raise ValueError(f'--test-scales: 1.0 must be one of the scales (the base grid), got {scales}')
    if len(scales) > 1 and fixed_height:
        raise ValueError('--test-scales with more than one scale is not implemented with --fixed-height')
    if len(scales) > 1 and cat_flip_offset:
        raise ValueError('--test-scales with more than one scale is not implemented with --cat-flip-offset')
    return scales


def validate_views(args):
    """--show-hmp-idx / --show-limb-idx / --show-all-limbs: the views take 2-component offsets (no --cat-flip-offset), and an index
    must name a heat-map channel / a limb type of the heads.  Raises ValueError.  -> whether any view is asked for."""
    hmp_idx, limb_idx = getattr(args, 'show_hmp_idx', None), getattr(args, 'show_limb_idx', None)
    if hmp_idx is None and limb_idx is None and not getattr(args, 'show_all_limbs', False):
        return False
    if getattr(args, 'cat_flip_offset', False):
        raise ValueError('--show-hmp-idx / --show-limb-idx / --show-all-limbs are not served with --cat-flip-offset (the views take '
                         '2-component offsets)')
    cfg = {}
    for name, stride in zip(args.headnets, args.strides):
        cfg.update(decoder.factory.parse_heads(name, stride))
    if hmp_idx is not None and not 0 <= hmp_idx < len(cfg['keypoints']):
        raise ValueError(f"--show-hmp-idx: {hmp_idx} outside the {len(cfg['keypoints'])} heat-map channels")
    if limb_idx is not None and not 0 <= limb_idx < len(cfg['skeleton']):
        raise ValueError(f"--show-limb-idx: {limb_idx} outside the {len(cfg['skeleton'])} limb types")
    return True


def decoded_maps(proc, features, flip_test):
    """(hm (N, C, h, w), off (N, 2L, h, w)): the stride-4 maps PostProcess.generate_limbs(features, flip_test) decodes -- the head
    outputs of the decoded stack, with flip_test what flip_augment merges from [images | mirrored images]."""
    hm = features[proc.hmp_index][0][proc.feat_stage]
    off = features[proc.omp_index][0][proc.feat_stage]
    if flip_test:
        hm, _, off, _, _ = proc.flip_augment(hm, [], off, [], False, 2)
    return hm, off


def annotations_inverse(keypoints, meta):
    """Poses from network-input coordinates back to the original image (transforms/preprocess.py:33-63):
    un-pad (offset), un-scale, keypoint scales / sqrt(sx*sy)."""
    kp = np.array(keypoints, copy=True)
    kp[:, :, 0] += meta['offset'][0]
    kp[:, :, 1] += meta['offset'][1]
    kp[:, :, 0] /= meta['scale'][0]
    kp[:, :, 1] /= meta['scale'][1]
    kp[:, :, 3] /= np.sqrt(np.prod(meta['scale']))
    if meta.get('hflip'):
        raise Exception('this should not happen. please have a check here, not implemented actually!')
    return kp


def poses_to_results(image_poses, image_meta, result_keypoints, result_image_ids):
    """Append one image's COCO keypoint results (evaluate.py:227-265); returns the inverse-mapped poses."""
    subset = annotations_inverse(image_poses, image_meta)
    image_id = image_meta['image_id']
    result_image_ids.append(image_id)
    subset[:, :, :2] = np.around(subset[:, :, :2], 2)
    # (vectorised: the reference's loop over persons x keypoints costs 0.3 ms per image at 40 poses -- 2.4 ms of host time per batch of 8,
    # which made the loop host-bound on crowded images; same values, same types: float x / y, int flag, sequential float sum of the scores)
    if len(subset):
        sub = subset.astype(float)
        n_kp = sub.shape[1]
        flags = ((sub[:, :, 0] > 0) | (sub[:, :, 1] > 0)).astype(int).tolist()
        trip = np.concatenate((sub[:, :, :2], np.zeros(sub.shape[:2] + (1,))), axis=2).reshape(len(sub), 3 * n_kp).tolist()
        # the reference's sum(v) / len(v) (evaluate.py:252) as explicit left-to-right float64 adds, column by column -- what Python's sum()
        # does up to 3.11 (from 3.12 on sum() of floats is Neumaier-compensated: the last ulp of a score may then differ from a reference
        # run under that interpreter; this box and the reference's pins run 3.10 / 3.7)
        total = sub[:, 0, 2].copy()
        for j in range(1, n_kp):
            total += sub[:, j, 2]
        scores = (total / n_kp).tolist()
        for triples, flag, score in zip(trip, flags, scores):
            triples[2::3] = flag
            result_keypoints.append({'image_id': image_id, 'category_id': 1, 'keypoints': triples, 'score': score})
    if not len(subset):
        result_keypoints.append({'image_id': image_id, 'category_id': 1, 'keypoints': np.zeros((17 * 3,)).tolist(),
                                 'score': 0.01})
    return subset


def synthetic_loader(n_batches, batch_size, size, device, seed=0):
    """Stand-in for DataLoader(CocoKeypoints): random normalised images + identity metas."""
    g = torch.Generator(device).manual_seed(seed)
    for b in range(n_batches):
        images = torch.randn(batch_size, 3, size, size, device=device, generator=g)
        metas = [{'image_id': b * batch_size + i, 'offset': np.array([0.0, 0.0]), 'scale': np.array([1.0, 1.0]),
                  'hflip': False} for i in range(batch_size)]
        yield images, [None] * batch_size, metas


def image_dir_loader(args):
    """--image-dir: batches of raw (h, w, 3) uint8 images for run_images' device input chain -- data.CocoKeypoints when the annotation
    file exists (the reference's id filtering, --all-images for every image), data.ImageList of the directory's files otherwise (image
    ids = positions in the sorted listing)."""
    from . import data
    if getattr(args, 'annotation_file', None) and os.path.exists(args.annotation_file):
        dataset = data.CocoKeypoints(args.raw_image_dir, args.annotation_file, all_images=getattr(args, 'all_images', False))
    else:
        names = sorted(f for f in os.listdir(args.raw_image_dir) if f.lower().endswith(('.jpg', '.jpeg', '.png', '.bmp', '.ppm')))
        dataset = data.ImageList([os.path.join(args.raw_image_dir, f) for f in names])
    return data.raw_batches(dataset, args.batch_size)


ENGINE_CACHE = 8     # input shapes run_images keeps engines for (--fixed-height: one per padded width, a handful on COCO; an engine
                     # holds its activations + graph, ~0.1 GB per image of 640x640, the weights are shared)
# Batches in flight: batch i runs whole (backbone graph + decoder) on HIP stream i % IN_FLIGHT with that lane's PostProcess; the head
# and tail of one forward (stem, final layers, heads, decoder: few workgroups) then run beside the bulk of the next.  A shape whose
# batches follow each other gets a second engine (captured graph + activations; the weights are shared, models/engine.py:_shared_layers)
# so that two of them can run at once.  Measured on bench.py's loop: 2 = +1.6...2.1 %, 3 = nothing more.
IN_FLIGHT = 2


def run_images(args, data_loader=None, model=None, n_synthetic_batches=4, stats=None):
    """The hot loop of evaluate.py:207-298.  Returns (result_keypoints, result_image_ids).
    stats: an optional dict that receives `host_enqueue_s` (per batch: host time to queue the input chain, the forward and the decoder --
    no wait in it), `engines_built`, `torch_conv_calls` (0: every engine is strict, models/engine.py), `test_scales` and
    `engines_per_shape` (input shape 'NxCxHxW' -> engines kept for it), with args.show_detected_poses `pose_images` and with
    args.show_hmp_idx / show_limb_idx / show_all_limbs `view_images` (the files written).
    args.range_report (--range-report FILE): the engines are built with probe=True, and at the end their probe rows, summed by probe
    name over engines, shapes and lanes, go with the first engine's weight_report() to FILE as JSON and to stats['range']
    (range_summary below).  Without it no call is added.
    args.test_scales (--test-scales, default [1.0]): more than one scale runs the multi-scale test (enqueue_multi_scale below)."""
    if not torch.cuda.is_available():
        raise RuntimeError('run_images needs a HIP device (offsetguided_amd has no CPU path)')
    dev = torch.device('cuda', torch.cuda.current_device())
    result_keypoints, result_image_ids = [], []
    if model is None:
        model, _ = models.model_factory(args)
        if args.resume:
            model, *_ = models.load_model(model, args.checkpoint_whole, optimizer=None, resume_optimizer=False,
                                          drop_layers=False, load_amp=False, **({'use_ema': True} if getattr(args, 'use_ema', False) else {}))
    processors = [decoder.decoder_factory(args) for _ in range(IN_FLIGHT)]
    lanes = _lib.lane_streams(dev, IN_FLIGHT) if IN_FLIGHT > 1 else [torch.cuda.current_stream(dev)]
    if data_loader is None and getattr(args, 'raw_image_dir', None):
        data_loader = image_dir_loader(args)
    if data_loader is None:
        data_loader = synthetic_loader(n_synthetic_batches, args.batch_size, args.long_edge, dev)
    feeder = DeviceFeeder(dev)
    # engines (scratch + captured graph) per input shape, those of the ENGINE_CACHE most recently used shapes kept (--fixed-height:
    # one shape per width); the folded / tiled weights are shared between them (models/engine.py:_shared_layers); a ragged last
    # batch is padded instead of getting an engine of its own.  A shape has one engine until two batches of it follow each other
    # closer than IN_FLIGHT apart: then the one still busy is left alone and another is built (at most IN_FLIGHT per shape)
    import collections
    engines = collections.OrderedDict()                      # shape -> [[engine, index of the last batch it ran, event behind that batch], ...]
    batch_time, end, last_print, pending = AverageMeter(), time.time(), -1, collections.deque()
    full_batch = None
    first_engine = [None]
    range_file = getattr(args, 'range_report', None)
    range_parts, range_images = [], [0]           # [(probe points, probe rows on the host)] of the engines that have gone; images forwarded

    # --show-detected-poses (evaluate.py:267-284): a batch's handle also carries (batch index, uint8 copy of the network-input batch);
    # once its poses are on the host they are painted over that copy on the device, in network-input coordinates (before
    # annotations_inverse), and the first image -- the reference shows batch_poses[0] -- is written as a PPM.  Off: nothing below runs
    show = bool(getattr(args, 'show_detected_poses', False))
    # --show-hmp-idx / --show-all-limbs / --show-limb-idx (demo_batch.py:215-317): the handle carries paint_views' canvases
    views = validate_views(args)
    hmp_idx, limb_idx, all_limbs = (getattr(args, k, None) for k in ('show_hmp_idx', 'show_limb_idx', 'show_all_limbs'))
    if show or views:
        from . import visualization
        show_dir = getattr(args, 'show_dir', '.')
        os.makedirs(show_dir, exist_ok=True)

    def canvas_of(images, normalised):
        """(n, 3, H, W) network-input batch -> (n, H, W, 3) uint8 RGB: the pixels the input chain normalised, or, for a tensor batch
        (synthetic_loader's random floats: no image behind it), a black canvas of the batch's size."""
        if not normalised:
            return torch.zeros((images.shape[0],) + tuple(images.shape[2:]) + (3,), dtype=torch.uint8, device=dev)
        return visualization.denormalise_u8(images)

    def paint_views(batch_idx, proc, features, flip_test, canvas):
        """Queued on the lane's stream right after submit (the engine outputs are read before a later batch overwrites them): the
        views of the FIRST image (canvas (1, H, W, 3) uint8) of the maps the decoder decodes -> (batch index, [(name, image)], event)."""
        hm, off = decoded_maps(proc, features, flip_test)
        hm, off = hm[:1], off[:1]
        out = []
        if hmp_idx is not None:
            for nms in (False, True):
                out.append((f'hmp{hmp_idx}' + ('_nms' if nms else ''), visualization.draw_heatmap(canvas.clone(), hm, hmp_idx, nms=nms)))
        if all_limbs:
            limbs = proc.generate_limbs(features, flip_test=flip_test, scored_off=scored_off)
            out.append(('limbs', visualization.draw_limbs(canvas.clone(), limbs[:1], dist_max=args.dist_max)))
        if limb_idx is not None:
            faded = (canvas >> 1) + 128       # white blended over the image with alpha 0.5: imshow(image, alpha=0.5), show.py:61
            out.append((f'limb{limb_idx}', visualization.draw_offsets(faded, hm, off, limb_idx, proc.skeleton)))
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(dev))
        return batch_idx, out, done

    def collect(handle):
        poses, metas = handle[:2]
        batch_poses = poses.result()
        if len(handle) > 3 and handle[3] is not None:
            batch_idx, painted, done = handle[3]
            done.synchronize()
            for name, image in painted:
                path = os.path.join(show_dir, f'{args.dump_name}.{name}.{batch_idx}.ppm')
                visualization.save_ppm(path, image[0])
                if stats is not None:
                    stats.setdefault('view_images', []).append(path)
        if len(handle) > 2 and handle[2] is not None:
            batch_idx, canvas = handle[2]
            visualization.draw_poses(canvas, list(batch_poses[:canvas.shape[0]]), processors[0].skeleton)
            path = os.path.join(show_dir, f'{args.dump_name}.poses.{batch_idx}.ppm')
            visualization.save_ppm(path, canvas[0])
            if stats is not None:
                stats.setdefault('pose_images', []).append(path)
        for image_poses, image_meta in zip(batch_poses, metas):   # zip drops the padded images of a ragged batch
            poses_to_results(image_poses, image_meta, result_keypoints, result_image_ids)

    preprocess, packer = [None], [None]

    def ahead(loader):
        """The loader one batch ahead; a batch of raw images is packed into pinned memory on a worker thread meanwhile (host
        memcpys: the reference does this part in DataLoader workers, evaluate.py:170-178)."""
        from concurrent.futures import ThreadPoolExecutor

        def prepare(batch):
            images = batch[0]
            if not isinstance(images, (list, tuple)):
                return batch, None
            if preprocess[0] is None:
                from .transforms import EvalPreprocess
                preprocess[0] = EvalPreprocess(args.long_edge, device=dev, fixed_height=args.fixed_height)
                packer[0] = ThreadPoolExecutor(max_workers=1, thread_name_prefix='og-pack')
            imgs = list(images)
            return (imgs,) + tuple(batch[1:]), packer[0].submit(preprocess[0].pack, imgs)

        it = iter(loader)
        try:
            nxt = prepare(next(it))
        except StopIteration:
            return
        while nxt is not None:
            cur = nxt
            try:
                nxt = prepare(next(it))
            except StopIteration:
                nxt = None
            yield cur

    def engine_slot(shape, batch_idx):
        """[engine, index of the last batch it ran, event behind that batch] for an input shape (built or reused, see above)."""
        of_shape = engines.pop(shape, None)
        if of_shape is None:
            if len(engines) >= ENGINE_CACHE:
                while pending:               # the batches in flight still read the outputs of the engines that go
                    collect(pending.popleft())
                for gone in engines.popitem(last=False)[1]:
                    if range_file:
                        range_parts.append((gone[0]._probe_points, gone[0].probe_stats.cpu()))
            of_shape = []
        engines[shape] = of_shape          # most recently used last
        slot = min(of_shape, key=lambda e: e[1], default=None)           # the engine of this shape that has rested longest
        if slot is None or (batch_idx - slot[1] < len(lanes) and len(of_shape) < len(lanes)):
            slot = [models.InferenceEngine(model, shape[0], shape[2], shape[3], device=dev,
                                           feat_stage=args.feat_stage, like=first_engine[0], **({'probe': True} if range_file else {})),
                    -len(lanes), None]
            first_engine[0] = first_engine[0] or slot[0]      # the module's weights do not change inside one call
            of_shape.append(slot)
            if stats is not None:
                stats['engines_built'] = stats.get('engines_built', 0) + 1
                stats.setdefault('_engines', []).append(slot[0])
        return slot

    # multi-scale test (--test-scales with more than one scale; decoder/multiscale.py): per batch and scale the input chain
    # (EvalPreprocess.multi_scale: one H2D copy, one launch per scale), the engine of that scale's shape, then one og_scale_accumulate_f32
    # launch per scale (og_scale_accumulate_heads_f32 with a keypoint-scale / jitter head) into the lane's base-grid accumulators and
    # one submit of the averaged maps.  [1.0] runs the code above unchanged.
    scored_off = bool(getattr(args, 'scored_off', False))
    scales = validate_test_scales(getattr(args, 'test_scales', [1.0]), getattr(args, 'fixed_height', False),
                                  getattr(args, 'cat_flip_offset', False))
    multi = len(scales) > 1
    if multi and len(scales) > ENGINE_CACHE:
        raise ValueError(f'--test-scales: at most {ENGINE_CACHE} scales (the engines of one batch must all stay cached)')
    base = scales.index(1.0)
    accumulators = [None] * len(lanes)

    def enqueue_multi_scale(batch_idx, images, metas, packed):
        nonlocal full_batch
        if packed is None:
            raise ValueError('--test-scales with more than one scale needs batches of raw (h, w, 3) uint8 images: a tensor batch '
                             'cannot be rescaled')
        per_scale = preprocess[0].multi_scale(images, scales, image_ids=[m['image_id'] for m in metas], packed=packed.result())
        base_metas = per_scale[base][1]
        n = len(base_metas)
        full_batch = full_batch or n
        lane = batch_idx % len(lanes)
        cur = torch.cuda.current_stream(dev)
        inputs, tables = [], []
        base_hw = tuple(s_ // 4 for s_ in per_scale[base][0].shape[2:])
        shown = ((batch_idx, canvas_of(per_scale[base][0], True)) if show else None,)   # the scale-1 batch is the one painted
        first = canvas_of(per_scale[base][0][:1], True) if views else None
        for x, metas_s in per_scale:
            aff = decoder.scale_affines(base_metas, metas_s, base_hw, tuple(s_ // 4 for s_ in x.shape[2:]))
            if n < full_batch:         # last batch of the dataset: filled up to the engine's batch, results are dropped
                x = torch.cat((x, x[-1:].expand(full_batch - n, -1, -1, -1)))
                aff = np.concatenate((aff, np.repeat(aff[-1:], full_batch - n, axis=0)))
            if args.flip_test:
                x = torch.cat((x, torch.flip(x, [-1])))
            inputs.append(x)
            tables.append(aff)
        aff_dev = torch.from_numpy(np.stack(tables)).pin_memory().to(dev, non_blocking=True)
        slots = []
        for x in inputs:
            slot = engine_slot(tuple(x.shape), batch_idx)
            slot[1] = batch_idx          # taken: a second scale of the same padded size gets another engine, or runs after this one
            slots.append(slot)
        if lanes[lane] is not cur:
            lanes[lane].wait_stream(cur)                 # the input chain, the flips and the affine tables ran / were copied on `cur`
            for x in inputs:
                x.record_stream(lanes[lane])
            aff_dev.record_stream(lanes[lane])
        proc = processors[lane]
        inv = float(np.float32(1.0) / np.float32(len(scales)))
        with torch.cuda.stream(lanes[lane]):
            has_scl, has_jit = slots[0][0].scale is not None, slots[0][0].jitter is not None   # forward_raw: (hm, off[, scale][, jitter])
            if accumulators[lane] is None or tuple(accumulators[lane][0].shape[2:]) != base_hw:
                new = lambda ch: torch.empty((full_batch, ch) + base_hw, dtype=torch.float32, device=dev)  # noqa: E731
                accumulators[lane] = (new(len(proc.keypoints)), new(2 * len(proc.skeleton)))
                if has_scl or has_jit:
                    accumulators[lane] += (new(len(proc.keypoints)) if has_scl else None, new(2) if has_jit else None)
            for slot in slots:
                if slot[2] is not None:
                    lanes[lane].wait_event(slot[2])      # the engine's last batch (maybe on another lane): its merge has read the outputs
            for s, (x, slot) in enumerate(zip(inputs, slots)):
                # scale by scale: forward, then its merge, then the engine's event -- two scales of one padded size may share an engine,
                # whose graph outputs the second forward overwrites (stream order: after the first merge has read them)
                hm, off, *rest = slot[0].forward_raw(x)
                range_images[0] += x.shape[0]
                scl = rest.pop(0) if has_scl else None
                jit = rest.pop(0) if has_jit else None
                mode = multiscale.MODE_WRITE if s == 0 else (multiscale.MODE_ADD_SCALE if s == len(inputs) - 1 else multiscale.MODE_ADD)
                multiscale.accumulate_scale(hm, off, aff_dev[s], accumulators[lane], mode, inv, args.flip_test, proc.keypoints,
                                            proc.skeleton, scl, jit)
                slot[2] = torch.cuda.Event()
                slot[2].record(lanes[lane])
            # the accumulators are read by K1 on this lane before the lane's next batch writes them (stream order)
            feats = multiscale.merged_features(accumulators[lane], slot[0].n_stacks)
            handle = (proc.submit(feats, flip_test=False, scored_off=scored_off), base_metas) + shown
            if views:
                first.record_stream(lanes[lane])
                handle += (paint_views(batch_idx, proc, feats, False, first),)
            return handle

    try:
        for batch_idx, ((images, _, metas), packed) in enumerate(ahead(data_loader)):
            t_host = time.perf_counter()
            if multi:
                handle = enqueue_multi_scale(batch_idx, images, metas, packed)
            else:
                if packed is not None:
                    # raw (h, w, 3) uint8 RGB images of any size: the input chain of evaluate.py:157-168 runs on the device
                    # (RescaleLongAbsolute + CenterPad, or with --fixed-height RescaleHighAbsolute + RightDownPad of :150-156, then
                    # ToTensor + Normalize; pinned staging packed a batch ahead, one H2D copy); metas are derived here
                    images, metas = preprocess[0](images, image_ids=[m['image_id'] for m in metas], packed=packed.result())
                images = feeder(images)
                shown = ((batch_idx, canvas_of(images, packed is not None)) if show else None,)
                first = canvas_of(images[:1], packed is not None) if views else None
                full_batch = full_batch or images.shape[0]
                if images.shape[0] < full_batch:   # last batch of the dataset: fill up to the engine's batch, results are dropped
                    images = torch.cat((images, images[-1:].expand(full_batch - images.shape[0], -1, -1, -1)))
                if args.flip_test:
                    images = torch.cat((images, torch.flip(images, [-1])))
                lane = batch_idx % len(lanes)
                slot = engine_slot(tuple(images.shape), batch_idx)
                cur = torch.cuda.current_stream(dev)
                if lanes[lane] is not cur:
                    lanes[lane].wait_stream(cur)                 # the input chain (H2D copy, rescale / pad / normalize, flip) ran on `cur`
                    images.record_stream(lanes[lane])
                if slot[2] is not None:
                    lanes[lane].wait_event(slot[2])              # the engine's last batch (maybe on another lane): its decoder has read the outputs
                with torch.cuda.stream(lanes[lane]):
                    outputs = slot[0](images)
                    range_images[0] += images.shape[0]
                    handle = (processors[lane].submit(outputs, flip_test=args.flip_test, cat_flip_offs=args.cat_flip_offset,
                                                      scored_off=scored_off), metas) + shown
                    if views:      # before the engine's event: the views read its outputs
                        first.record_stream(lanes[lane])
                        handle += (paint_views(batch_idx, processors[lane], outputs, args.flip_test, first),)
                    slot[1], slot[2] = batch_idx, torch.cuda.Event()
                    slot[2].record(lanes[lane])
            pending.append(handle)
            if stats is not None:
                stats.setdefault('host_enqueue_s', []).append(time.perf_counter() - t_host)
            while len(pending) > len(lanes):                 # the oldest batch: its poses are on the host by now (or soon)
                collect(pending.popleft())
            if batch_idx % args.print_freq == 0:
                torch.cuda.synchronize()
                now = time.time()
                per_batch = (now - end) / (batch_idx - last_print)   # batches since the last print (1 at the first), not print_freq
                end, last_print = now, batch_idx
                if batch_idx > 0:                                    # the first batch builds the engine: not a speed sample
                    batch_time.update(per_batch)
                print('==================> [{0}]\tTime {1:.3f} ({2:.3f})\tSpeed {3:.3f} ({4:.3f})'.format(
                    batch_idx, per_batch, batch_time.avg or per_batch, args.batch_size / per_batch,
                    args.batch_size / (batch_time.avg or per_batch)))
        while pending:
            collect(pending.popleft())
        if range_file:
            torch.cuda.synchronize(dev)
            range_parts += [(e[0]._probe_points, e[0].probe_stats.cpu()) for of in engines.values() for e in of]
            report = range_summary(first_engine[0], range_parts, range_images[0])
            with open(range_file, 'w') as f:
                json.dump(report, f, indent=1)
            print(report['summary']['verdict'])
            if stats is not None:
                stats['range'] = report
    finally:
        # also on an exception (engine build failure, OgError, the --fixed-height assertion): the worker must not outlive the
        # call holding pinned staging buffers, and a pack still queued must not write one while the caller handles the error
        if packer[0] is not None:
            packer[0].shutdown(wait=True, cancel_futures=True)
        if stats is not None:
            stats['torch_conv_calls'] = sum(len(e.torch_conv_calls) for e in stats.pop('_engines', []))
            stats['test_scales'] = list(scales)
            stats['engines_per_shape'] = {'x'.join(str(v) for v in shape): len(of) for shape, of in engines.items()}
    return result_keypoints, result_image_ids


def range_summary(engine, parts, images):
    """The --range-report dict: {dtype, images, weights, activations, summary}.  parts: [(probe points, (points, 9) int64 rows)] of
    every engine that ran; rows of one probe name are combined over engines, shapes and lanes (counts summed, max / min combined) and
    listed in the first engine's issue order.  images: the images forwarded (the flipped copies of --flip-test and the padding of a
    ragged last batch included: every probe's n is images x its elements per image).  weights: engine.weight_report()."""
    from .models import range_report
    merged, order = {}, []
    for points, rows in parts:
        for (name, route, shape, riders), row in zip(points, rows):
            if name not in merged:
                order.append(name)
                merged[name] = {'name': name, 'route': route, 'with': list(riders), 'shapes': [], 'rows': []}
            entry = merged[name]
            if list(shape) not in entry['shapes']:
                entry['shapes'].append(list(shape))
            entry['rows'].append(row.reshape(1, -1))
    activations = []
    for name in order:
        entry = merged[name]
        words = range_report.decode(range_report.combine(entry.pop('rows')))[0]
        activations.append({**entry, **{k: words[k] for k in ('n', 'nan', 'inf', 'sub', 'zero', 'max', 'min')}})
    weights = engine.weight_report()
    bad = next((a for a in activations if a['inf'] + a['nan'] > 0), None)
    top = max(activations, key=lambda a: a['max'], default=None)
    over = [w['name'] for w in weights if w['folded']['over'] > 0]
    flush = [w['name'] for w in weights if w['folded']['flush'] > 0]
    dtype = str(engine.dtype).replace('torch.', '')
    summary = {'first_nonfinite_activation': {k: bad[k] for k in ('name', 'route', 'inf', 'nan')} if bad else None,
               'weights_over': over, 'weights_flush': flush,
               'max_activation': {'name': top['name'], 'value': top['max']} if top else None}
    summary['verdict'] = (f'range report ({dtype}, {images} images): '
                          + (f"first non-finite activation at {bad['name']} ({bad['inf']} inf, {bad['nan']} NaN)" if bad else
                             'no non-finite activation')
                          + f'; {len(over)} layers with overflowing and {len(flush)} with flushed folded weights'
                          + (f"; largest activation {top['max']:.6g} at {top['name']}" if top else ''))
    return {'dtype': dtype, 'images': images, 'weights': weights, 'activations': activations, 'summary': summary}


class DeviceFeeder:
    """Host batch -> device through two pinned staging buffers (the data loader's tensors are pageable: a direct
    `.to(device, non_blocking=True)` from them is a synchronous staged copy).  The copy of batch i+1 is queued on its own
    stream while batch i computes; a batch that already lives on the device passes through."""

    def __init__(self, device):
        self.device = device
        self.stream = _lib.dedicated_stream(device, ('feeder',))
        self.slots, self.turn = [None, None], 0

    def __call__(self, images):
        if images.is_cuda:
            return images
        slot = self.slots[self.turn]
        if slot is None or slot[0].shape != images.shape or slot[0].dtype != images.dtype:
            slot = self.slots[self.turn] = [torch.empty(images.shape, dtype=images.dtype).pin_memory(), None]
        if slot[1] is not None:
            slot[1].synchronize()                # the copy that last used this staging buffer has left the host
        slot[0].copy_(images)
        with torch.cuda.stream(self.stream):
            out = slot[0].to(self.device, non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record(self.stream)
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        out.record_stream(torch.cuda.current_stream(self.device))
        self.turn ^= 1
        return out


def validation(args, data_loader=None, scorer=None):
    """run_images + COCO keypoint evaluation (evaluate.py:303-328).  scorer: 'pycocotools' (the reference's COCOeval; ImportError
    without the package), 'native' (cocoeval.KeypointEval on cocoeval.load_ground_truth(args.annotation_file): needs no pycocotools)
    or None: pycocotools when it imports, native otherwise.  The results JSON is written either way.  -> the COCOeval, or with the
    native scorer the KeypointEval (.stats, .precision, .recall)."""
    if scorer not in (None, 'pycocotools', 'native'):
        raise ValueError(f"validation: scorer must be 'pycocotools', 'native' or None, got {scorer!r}")
    if scorer is None:
        try:
            import pycocotools.cocoeval  # noqa: F401
            scorer = 'pycocotools'
        except ImportError:
            scorer = 'native'
    if scorer == 'native':
        from . import cocoeval
        if not torch.cuda.is_available():
            raise _lib.OgError('validation: the native scorer needs a HIP device (offsetguided_amd has no CPU path)')
        res_file = 'data/link2COCO2017/results/person_keypoints_%s_%s_results.json' % (args.dataset, args.dump_name)
        os.makedirs(os.path.dirname(res_file), exist_ok=True)
        ground_truth = cocoeval.load_ground_truth(args.annotation_file)
        results, ids = run_images(args, data_loader)
        json.dump(results, open(res_file, 'w'))
        keypoint_eval = cocoeval.KeypointEval(ground_truth).evaluate(results, ids)
        keypoint_eval.summarize()
        return keypoint_eval
    try:
        from pycocotools.coco import COCO
        from pycocotools.cocoeval import COCOeval
    except ImportError as e:
        raise ImportError('validation() needs pycocotools; run_images() does not') from e
    res_file = 'data/link2COCO2017/results/person_keypoints_%s_%s_results.json' % (args.dataset, args.dump_name)
    os.makedirs(os.path.dirname(res_file), exist_ok=True)
    coco_gt = COCO(args.annotation_file)
    results, ids = run_images(args, data_loader)
    json.dump(results, open(res_file, 'w'))
    coco_eval = COCOeval(coco_gt, coco_gt.loadRes(res_file), iouType='keypoints')
    coco_eval.params.imgIds = ids
    coco_eval.evaluate()
    coco_eval.accumulate()
    coco_eval.summarize()
    return coco_eval


if __name__ == '__main__':
    logging.basicConfig(level=logging.INFO)
    a = evaluate_cli()
    if a.score:
        validation(a)
    else:
        kps, ids = run_images(a)
        print(f'{len(ids)} images, {len(kps)} detections')
