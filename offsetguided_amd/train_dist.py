"""Data-parallel training step (reference train_dist.py:108-387), MI355X-native:

  apex AMP O1 + dynamic loss scaling      -> torch.autocast(bfloat16) (no scaler needed); --opt-level O1: torch.autocast(float16) and
    (amp.scale_loss, :336)                    optim.DeviceLossScaler, whose unscale / overflow skip / scale update run inside the step
  apex DistributedDataParallel            -> torch DDP over RCCL/xGMI: 25 MB gradient buckets whose
    (delay_allreduce=True: one flat            all-reduce overlaps the rest of backward (xGMI links are
     all-reduce after backward)                point-to-point, so overlap matters more than on NVSwitch)
  apex SyncBatchNorm                      -> torch.nn.SyncBatchNorm (optional, --no-sync-bn)
  apex FusedAdam                          -> torch.optim.Adam(fused=True); --device-step: optim.DeviceAdam / DeviceSGD (csrc/optim.hip),
    loss.item() batch drop (:322)             gradient clipping and the batch drop as one device-side scale: no host wait in the step
  (no weight average in the reference)    -> --ema-decay D: optim.ModelEma, averaged inside the --device-step update launch; the
                                              checkpoint carries it (`ema_state_dict`), evaluate --use-ema scores it
  mask/gather losses                      -> fused HIP loss kernels (models/losses.py, csrc/losses.hip)

One process per GPU (`python -m torch.distributed.run --nproc-per-node N -m offsetguided_amd.train_dist`);
without COCO on disk the loop runs on synthetic encoder-style targets (GT heatmaps, patch offsets with
inf outside the patches, instance scales, mask_miss).  --augment: the pool holds raw uint8 images and un-augmented annotations,
and every step warps a new random crop on the device (transforms.DeviceAugment = the reference's WarpAffineTransforms).
"""
import argparse
import os
import random
import time

import numpy as np
import torch

from . import _lib, encoder, models, optim, sharding, synth, transforms
from .config import coco_data as cd
from .utils import AverageMeter, adjust_learning_rate, boolean_string


def train_cli(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    models.net_cli(p)
    p.add_argument('--resume', '-r', action='store_true', default=False)
    p.add_argument('--drop-optim-state', dest='resume_optimizer', action='store_false', default=True,
                   help='do not resume the optimizer from the checkpoint')
    p.add_argument('--drop-layers', action='store_true', default=False,
                   help='drop the offset convolutions of the checkpoint (--resume, or a --checkpoint-whole start)')
    p.add_argument('--recount-epoch', action='store_true', default=False, help='restart the epoch counter at 0 after --resume')
    p.add_argument('--freeze', action='store_true', default=False, help='freeze the layers of the BaseNet, i.e. the backbone')
    p.add_argument('--epochs', default=100, type=int)
    p.add_argument('--warmup', action='store_true', default=False, help='warm-up learning rate')
    p.add_argument('--checkpoint-path', '-p', default='link2checkpoints_storage')
    p.add_argument('--batch-size', default=8, type=int, help='per-GPU batch size')
    p.add_argument('--square-length', default=512, type=int, help='training crop size')
    p.add_argument('--steps-per-epoch', default=20, type=int, help='synthetic-data epoch length')
    p.add_argument('--no-sync-bn', dest='sync_bn', action='store_false', default=True)
    p.add_argument('--print-freq', '-f', default=10, type=int)
    p.add_argument('--bench', action='store_true', default=False,
                   help='BASELINE configs[4] measurement: time --bench-steps training steps (after --bench-warmup) on synthetic '
                        'annotations and print ONE JSON line (step ms, images/s over all ranks, gradient all-reduce bus GB/s); '
                        'no checkpoint is written')
    p.add_argument('--bench-steps', default=20, type=int)
    p.add_argument('--bench-warmup', default=5, type=int)
    p.add_argument('--grad-compress', default='bf16', choices=['none', 'bf16'],
                   help='DDP gradient all-reduce payload: fp32 (750.9 MB) or bf16-compressed (375.5 MB)')
    g = p.add_argument_group('training parameters for warp affine (data/factory.py:84-104)')
    g.add_argument('--augment', action='store_true', default=False,
                   help='augment on the device: raw uint8 images + annotations in the pool, a new random WarpAffineTransforms crop '
                        '(flip, rotate, scale, stretch, translate) of every batch in every step')
    g.add_argument('--train-annotations', default=None, type=str, metavar='FILE',
                   help='train on a COCO keypoint annotation file (data.CocoKeypoints; with --train-image-dir, implies --augment): '
                        'mask_miss is rasterised on the device from the polygons and RLEs and carried through the warp into the losses')
    g.add_argument('--train-image-dir', default=None, type=str, metavar='DIR', help="directory of that file's images")
    g.add_argument('--flip-prob', default=0.5, type=float, help='the probability to flip the input image')
    g.add_argument('--max-rotate', default=45, type=float, help='upper bound of the image rotation during augmentation')
    g.add_argument('--min-scale', default=0.5, type=float, help='lower bound of the relative image scale during augmentation')
    g.add_argument('--max-scale', default=2.0, type=float, help='upper bound of the relative image scale during augmentation')
    g.add_argument('--min-stretch', default=0.95, type=float, help='lower bound of the relative image length stretch')
    g.add_argument('--max-stretch', default=1.05, type=float, help='upper bound of the relative image length stretch')
    g.add_argument('--max-translate', default=150, type=int, help='upper bound of shifting the image during augmentation')
    g = p.add_argument_group('photometric augmentation behind the warp, with --augment (data/factory.py:250-265; all off by default)')
    g.add_argument('--color-tint-prob', default=0., type=float,
                   help='probability of ColorTint (hue +-10, saturation +-40, value +-30 in 8-bit HSV); the reference trains with 0.2')
    g.add_argument('--gray-prob', default=0., type=float, help='probability of Gray (the reference never composes it)')
    g.add_argument('--jpeg-prob', default=0., type=float,
                   help='probability of a JpegCompression round trip; 0.1 in the reference, where the step is commented out')
    g.add_argument('--jpeg-quality', default=50, type=int, help='quality of that round trip, 1...100 (the reference: 50)')
    g.add_argument('--annotation-jitter-prob', default=0., type=float,
                   help='probability of AnnotationJitter (+-0.5 px on every keypoint); 0.1 in the reference, where the step is commented out')
    g = p.add_argument_group('optimizer configuration')
    g.add_argument('--optimizer', type=str, default='adam', choices=['sgd', 'adam'])
    g.add_argument('--learning-rate', type=float, default=2.5e-4, help='learning rate for world size 1')
    g.add_argument('--momentum', default=0.9, type=float)
    g.add_argument('--weight-decay', '--wd', default=0, type=float)
    g.add_argument('--device-step', action='store_true', default=False,
                   help='step with the HIP multi-tensor optimizer (optim.DeviceAdam / DeviceSGD): the exploding-batch drop and the '
                        'gradient clipping are one device-side scale, losses stay on the device between --print-freq lines')
    g.add_argument('--max-grad-norm', default=float('inf'), type=float,
                   help='clip the norm of all gradients to this value, as torch.nn.utils.clip_grad_norm_ does (with --device-step)')
    g.add_argument('--ema-decay', default=None, type=float, metavar='D',
                   help='keep an exponential moving average of the weights with decay D, 0 <= D < 1 (optim.ModelEma; with '
                        '--device-step: the update launch averages what it steps); every checkpoint carries it as ema_state_dict')
    g.add_argument('--ema-warmup', default=True, type=boolean_string,
                   help='with --ema-decay: the decay of update t is min(D, (1 + t) / (10 + t))')
    g = p.add_argument_group('apex configuration (train_dist.py:77-82)')
    g.add_argument('--opt-level', type=str, default=None, choices=['O0', 'O1', 'O2', 'O3'],
                   help='O0: fp32, no autocast; O1: fp16 autocast with a device-side loss scaler (optim.DeviceLossScaler, needs '
                        '--device-step); not given: bf16 autocast, no scaler.  O2 / O3 are not implemented.  With --grad-compress bf16 '
                        'the DDP hook rounds the SCALED gradients to bf16: bf16 has fp32\'s exponent range, so the scale costs no range '
                        'and the rounding is the same relative one as without a scaler -- the two flags combine')
    g.add_argument('--loss-scale', type=str, default=None, metavar="{dynamic,NUMBER}",
                   help='with --opt-level O1: dynamic loss scaling (not given, or "dynamic") or a static scale')
    g.add_argument('--drop-amp-state', dest='load_amp', action='store_false', default=True,
                   help="do not resume the loss scaler from the checkpoint's amp entry")
    args = p.parse_args(argv)
    if args.opt_level in ('O2', 'O3'):
        p.error(f'--opt-level {args.opt_level} is not implemented: it needs fp16 model copies with fp32 master weights (O0 and O1 are)')
    if args.opt_level == 'O1' and not args.device_step:
        p.error('--opt-level O1 unscales and skips overflow steps inside the device-side step: add --device-step')
    if args.loss_scale is not None:
        if args.opt_level != 'O1':
            p.error('--loss-scale belongs to --opt-level O1')
        if args.loss_scale != 'dynamic':
            try:
                args.loss_scale = float(args.loss_scale)
            except ValueError:
                p.error(f"--loss-scale: 'dynamic' or a number, got {args.loss_scale!r}")
            if not 0 < args.loss_scale < float('inf'):
                p.error('--loss-scale must be positive and finite')
    if args.max_grad_norm != float('inf') and not args.device_step:
        p.error('--max-grad-norm is applied by the device-side step: add --device-step')
    if not args.max_grad_norm > 0:
        p.error('--max-grad-norm must be positive')
    if args.ema_decay is not None:
        if not args.device_step:
            p.error('--ema-decay is averaged by the device-side step: add --device-step')
        if not 0 <= args.ema_decay < 1:
            p.error('--ema-decay must lie in [0, 1)')
    if bool(args.train_annotations) != bool(args.train_image_dir):
        p.error('--train-annotations and --train-image-dir go together')
    if args.train_annotations:
        args.augment = True
    return args


def synthetic_targets(seed, batch, size, device, *, background=False, jitter=False, scale=False):
    """Encoder-style training targets (encoder/heatmap.py, encoder/offset.py conventions) for one batch:
    annos = [(gt_hmp, gt_bghmp, gt_jomp, mask_miss), (gt_off, gt_scale, gt_ps, mask_miss)].  The optional maps are None
    unless asked for: background = 1 - max over the keypoint channels; jitter (N,2,h,w) sub-cell offsets round the peaks,
    inf elsewhere; scale (N,17,h,w) keypoint scales round each channel's peaks, NaN elsewhere."""
    hm, off = synth.synth_batch(seed, batch, size, size, hm_noise=0.0, off_noise=0.0)
    off = np.where(off == 0.0, np.inf, off).astype(np.float32)          # offsets exist in the patches only
    h = size // 4
    rng = synth.HashRng(seed + 17)
    ps = rng.uniform(batch * h * h, 40.0, 300.0).reshape(batch, 1, h, h).astype(np.float32)
    mask = torch.ones(batch, 1, h, h, dtype=torch.bool, device=device)
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    hm = np.clip(hm, 0, 1).astype(np.float32)
    bg = jit = sc = None
    if background:
        bg = t(1.0 - hm.max(axis=1, keepdims=True))
    if jitter:
        jit = rng.uniform(batch * 2 * h * h, -0.5, 0.5).reshape(batch, 2, h, h).astype(np.float32)
        jit = t(np.where(hm.max(axis=1, keepdims=True) >= 0.25, jit, np.float32(np.inf)))
    if scale:
        sc = rng.uniform(batch * hm.shape[1] * h * h, 1.0, 12.0).reshape(hm.shape).astype(np.float32)
        sc = t(np.where(hm >= 0.25, sc, np.float32(np.nan)))
    return [(t(hm), bg, jit, mask), (t(off), sc, t(ps), mask)]


def synthetic_annotations(seed, batch, size, width=None):
    """Annotation-style input of the encoders: joints (N,P,17,4) fp32 [x, y, v, scale] padded to P persons, and the
    person count per image (transforms/annotations.py:46-50 layout; the scale column plays the keypoint scale).  Scenes are
    size x size, or size rows x width columns."""
    scenes = [synth.make_scene(synth.HashRng(seed * 1000003 + i), size, width or size) for i in range(batch)]
    p_max = max(xy.shape[0] for xy, _, _ in scenes)
    joints = np.zeros((batch, p_max, 17, 4), np.float32)
    for i, (xy, vis, _) in enumerate(scenes):
        p = xy.shape[0]
        joints[i, :p, :, :2] = xy
        joints[i, :p, :, 2] = vis * 2.0
        extent = (xy[..., 1].max(1) - xy[..., 1].min(1)).astype(np.float32)            # person height in pixels
        joints[i, :p, :, 3] = (extent[:, None] * np.asarray(cd.COCO_PERSON_SIGMAS, np.float32)[None]).astype(np.float32)
    return joints, np.array([xy.shape[0] for xy, _, _ in scenes], np.int32)


def synthetic_raw_images(seed, joints, n_persons, height, width):
    """Raw uint8 (height, width, 3) images for synthetic annotations: flat limbs of the annotated skeletons on noise."""
    images = []
    for i in range(joints.shape[0]):
        rs = np.random.RandomState(seed * 1009 + i)
        im = rs.randint(64, 192, (height, width, 3)).astype(np.uint8)
        for p in range(int(n_persons[i])):
            colour = rs.randint(0, 256, 3).astype(np.uint8)
            for a, b in cd.COCO_PERSON_SKELETON:
                ja, jb = joints[i, p, a], joints[i, p, b]
                if ja[2] > 0 and jb[2] > 0:
                    t = np.linspace(0.0, 1.0, int(max(abs(jb[0] - ja[0]), abs(jb[1] - ja[1]))) + 2)[:, None]
                    xy = np.rint(ja[None, :2] * (1 - t) + jb[None, :2] * t).astype(np.int64)
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            im[np.clip(xy[:, 1] + dy, 0, height - 1), np.clip(xy[:, 0] + dx, 0, width - 1)] = colour
        images.append(im)
    return images


def augmented_batch(augment, entry, rng, events=None):
    """One training batch from a pool entry of raw images + annotations: a new random crop (transforms.DeviceAugment) -> (images,
    (joints, n_persons)) on the device.  events: a list that receives a (start, end) pair of HIP timing events round the augment calls.
    An entry with a fifth element (annotations.MaskTables, from a COCO file) has its mask_miss built on the device (data.device_masks)
    and warped with the images: -> (images, (joints, n_persons, mask (N,S,S) uint8))."""
    raws, joints, n_persons, n_persons_dev = entry[:4]
    stream = torch.cuda.current_stream(augment.device)
    if events is not None:
        start, end = _lib.TimingEvent(), _lib.TimingEvent()
        start.record(stream)
    if len(entry) > 4:
        from . import data
        images, joints_dev, mask, _ = augment(raws, joints, n_persons, data.device_masks(entry[4], augment.device, mask_all=False), rng=rng)
    else:
        images, joints_dev, _, _ = augment(raws, joints, n_persons, rng=rng)
    if events is not None:
        end.record(stream)
        events.append((start, end))
    if len(entry) > 4:
        return images.contiguous(memory_format=torch.channels_last), (joints_dev, n_persons_dev, mask)
    return images.contiguous(memory_format=torch.channels_last), (joints_dev, n_persons_dev)


def coco_pool(args, rank, world, dev):
    """The pool of --train-annotations: this rank's share of data.CocoKeypoints in batches of --batch-size (a ragged last batch is
    dropped), every entry (raw images, joints, n_persons, n_persons on the device, mask tables) -- what augmented_batch takes.  The
    images are decoded once and stay on the host; crop, mask_miss and targets are made on the device in every step."""
    from . import data
    dataset = data.CocoKeypoints(args.train_image_dir, args.train_annotations)
    indices = list(range(rank, len(dataset), world))
    pool = []
    for first in range(0, len(indices) - args.batch_size + 1, args.batch_size):
        raws, joints, n_persons, tables, _ = data.collate_raw([dataset[i] for i in indices[first:first + args.batch_size]])
        pool.append((raws, joints, n_persons, torch.from_numpy(n_persons).to(dev), tables))
    if not pool:
        raise ValueError(f'--train-annotations: {len(indices)} images for rank {rank}, fewer than one batch of {args.batch_size}')
    return pool


def encode_targets(encoders, joints, n_persons, mask_miss=None):
    """Device-side ground truth (offsetguided_amd.encoder = reference encoder/): the same annos layout as
    synthetic_targets, produced from annotations by the HIP encoder kernels inside the step.  mask_miss: the warped (N,S,S) uint8
    mask of the crops (0 = not labelled), shrunk to each head's stride by its encoder (og_shrink_mask_miss_u8); None = all labelled."""
    if mask_miss is None:
        hm, bg, jit, mask = encoders[0].encode_batch(joints, n_persons)
        off, sc, ps, _ = encoders[1].encode_batch(joints, n_persons)
    else:
        hm, bg, jit, mask = encoders[0].encode_batch(joints, n_persons, mask_miss)
        off, sc, ps, omask = encoders[1].encode_batch(joints, n_persons, mask_miss)
        return [(hm, bg if bg.numel() else None, jit if jit.numel() else None, mask), (off, sc if sc.numel() else None, ps, omask)]
    return [(hm, bg if bg.numel() else None, jit if jit.numel() else None, mask), (off, sc if sc.numel() else None, ps, mask)]


def amp_setup(args, dev, use_cuda):
    """--opt-level -> (autocast dtype or None, loss scaler or None).  Not given: the bf16 autocast of every run so far, no scaler."""
    level = getattr(args, 'opt_level', None)
    if level is None:
        return (torch.bfloat16 if use_cuda else None), None
    if level == 'O0':
        return None, None
    loss_scale = getattr(args, 'loss_scale', None)
    return torch.float16, optim.DeviceLossScaler('dynamic' if loss_scale is None else loss_scale, device=dev)


def train_step(model, criterion, optimizer, images, annos, lambdas, autocast_dtype=torch.bfloat16):
    """One optimisation step (train_dist.py:304-342).  Returns (loss, per-head losses)."""
    optimizer.zero_grad(set_to_none=True)
    dev_type = 'cuda' if images.is_cuda else 'cpu'
    with torch.autocast(dev_type, dtype=autocast_dtype, enabled=autocast_dtype is not None):
        outputs = model(images)
    multi_losses = []
    for out, lossfun, anno in zip(outputs, criterion, annos):
        out32 = tuple([o.float() if isinstance(o, torch.Tensor) else o for o in part] for part in out)
        multi_losses += list(lossfun(out32, *anno))
    assert len(multi_losses) <= len(lambdas), 'lambdas is incomplete'
    loss = sum(lam * l for lam, l in zip(lambdas, multi_losses))
    if loss.item() > 1e8:  # gradient explosion: drop the batch (train_dist.py:322-325)
        loss = loss * 0.0
    loss.backward()
    optimizer.step()
    return loss.detach(), [float(l.detach()) if torch.is_tensor(l) else float(l) for l in multi_losses]


def train_step_device(model, criterion, optimizer, images, annos, lambdas, autocast_dtype=torch.bfloat16, max_grad_norm=float('inf'),
                      world=1, scaler=None, ema=None):
    """train_step for optim.DeviceAdam / DeviceSGD: nothing is read back.  backward() runs on the real loss; the step multiplies the
    gradients by the device-side scale -- 0 for a batch whose loss exceeds 1e8 (train_dist.py:322-325) or whose gradients are not
    finite, the clip_grad_norm_ coefficient of --max-grad-norm otherwise.  Under DDP the gradients are all-reduced when backward()
    returns, so every rank takes the same norm; the loss the drop looks at is the largest over the ranks, so every rank drops the same
    batches.  scaler (optim.DeviceLossScaler, --opt-level O1): backward() runs on scaler.scale(loss); the step unscales, and a step
    whose gradients overflowed is skipped and moves the loss scale; the drop still looks at the unscaled loss.  Under DDP an inf or
    NaN in any rank's gradients is non-finite on every rank after the all-reduce, so every rank takes the same decision and keeps the
    same loss scale without another collective.  ema (optim.ModelEma, --ema-decay): the step averages the weights it writes.  Returns (loss, per-head losses) as device tensors."""
    optimizer.zero_grad(set_to_none=True)
    dev_type = 'cuda' if images.is_cuda else 'cpu'
    with torch.autocast(dev_type, dtype=autocast_dtype, enabled=autocast_dtype is not None):
        outputs = model(images)
    multi_losses = []
    for out, lossfun, anno in zip(outputs, criterion, annos):
        out32 = tuple([o.float() if isinstance(o, torch.Tensor) else o for o in part] for part in out)
        multi_losses += list(lossfun(out32, *anno))
    assert len(multi_losses) <= len(lambdas), 'lambdas is incomplete'
    loss = sum(lam * l for lam, l in zip(lambdas, multi_losses))
    (loss if scaler is None else scaler.scale(loss)).backward()
    loss = loss.detach()
    guard = loss
    if world > 1:
        guard = loss.clone()
        torch.distributed.all_reduce(guard, op=torch.distributed.ReduceOp.MAX)
    extra = {} if ema is None else {'ema': ema}
    if scaler is None:
        optimizer.step(loss=guard, max_grad_norm=max_grad_norm, **extra)
    else:
        optimizer.step(loss=guard, max_grad_norm=max_grad_norm, scaler=scaler, **extra)
    return loss, [l.detach() if torch.is_tensor(l) else l for l in multi_losses]


def freeze_backbone(model):
    """--freeze (train_dist.py:202-206): the BaseNet's parameters take no gradient; call before the optimizer is made."""
    for name, param in model.named_parameters():
        if 'basenet' in name:
            param.requires_grad = False
    return model


def make_optimizer(args, model, world, use_cuda):
    """The optimizer of a run over the parameters that take a gradient (train_dist.py:208-222)."""
    params = [p for p in model.parameters() if p.requires_grad]
    lr = args.learning_rate * world
    if getattr(args, 'device_step', False):
        if args.optimizer == 'adam':
            return optim.DeviceAdam(params, lr=lr, weight_decay=args.weight_decay)
        return optim.DeviceSGD(params, lr=lr, momentum=args.momentum, weight_decay=args.weight_decay)
    if args.optimizer == 'adam':
        return torch.optim.Adam(params, lr=lr, weight_decay=args.weight_decay, fused=use_cuda)
    return torch.optim.SGD(params, lr=lr, momentum=args.momentum, weight_decay=args.weight_decay)


def make_ema(args, model):
    """--ema-decay -> optim.ModelEma over the model as it stands (on its device, in its memory format), or None."""
    decay = getattr(args, 'ema_decay', None)
    return None if decay is None else optim.ModelEma(model, decay=decay, warmup=getattr(args, 'ema_warmup', True))


def load_checkpoint(args, model, optimizer, use_cuda, scaler=None, ema=None):
    """--resume (train_dist.py:230-236, :267-268): weights, optimizer state unless --drop-optim-state, and the epoch the LR schedule
    is at unless --recount-epoch.  Without --resume, --checkpoint-whole initialises the weights only (fine-tuning, as
    evaluate.py:189-191 loads it); a path that does not exist is an error (load_model raises FileNotFoundError), never a silent
    random init.  scaler: resumed from the checkpoint's `amp` entry (train_dist.py:234-236) unless --drop-amp-state; a checkpoint
    without one leaves it as made.  ema (optim.ModelEma bound to model): resumed from the checkpoint's `ema_state_dict`; a checkpoint
    without one, --drop-optim-state and a --checkpoint-whole start begin the average at the loaded weights.  -> (model, optimizer, start_epoch, start_loss or None)."""
    drop_layers = getattr(args, 'drop_layers', False)
    if args.resume:
        if not args.checkpoint_whole:
            raise ValueError('--resume needs --checkpoint-whole <file>')
        model, optimizer, start_epoch, start_loss, amp_state = models.load_model(
            model, args.checkpoint_whole, optimizer=optimizer, resume_optimizer=getattr(args, 'resume_optimizer', True),
            drop_layers=drop_layers, optimizer2cuda=use_cuda, load_amp=scaler is not None and getattr(args, 'load_amp', True),
            **({} if ema is None else {'ema': ema}))
        if scaler is not None:
            optim.load_amp_state(scaler, amp_state)
        if ema is not None and not getattr(args, 'resume_optimizer', True):
            ema.reset()
        return model, optimizer, 0 if getattr(args, 'recount_epoch', False) else start_epoch, start_loss
    if args.checkpoint_whole:
        model, *_ = models.load_model(model, args.checkpoint_whole, optimizer=None, resume_optimizer=False, drop_layers=drop_layers)
        if ema is not None:
            ema.reset()
    return model, optimizer, 0, None


def describe_losses(args):
    """The heads and loss choices of a run, for the --bench line: the default is 'focal-L2 hmp + L1 offset losses'."""
    short = lambda name: {'focal_l2_loss': 'focal-L2', 'l2_loss': 'L2', 'offset_l1_loss': 'L1', 'vector_l1_loss': 'vector-L1',  # noqa: E731
                          'offset_laplace_loss': 'laplace', 'offset_instance_l1_loss': 'instance-L1', 'scale_l1_loss': 'L1'}[name]
    parts = [f'{short(args.hmp_loss)} hmp']
    if args.include_background:
        parts.append(f'{short(args.hmp_loss)} background')
    if args.include_jitter_offset:
        parts.append(f'{short(args.jitter_offset_loss)} jitter')
    parts.append(f'{short(args.offset_loss)} offset' + (' (spread head)' if args.include_spread else ''))
    if args.include_scale:
        parts.append(f'{short(args.scale_loss)} scale')
    return ' + '.join(parts) + ' losses' + (', sqrt' if args.sqrt_re else '') + ('' if args.fused_losses else ', torch-formulated')


def bench_steps(args, model, criterion, optimizer, pool, encoders, dev, rank, world, augment=None, rng=None, amp=None, ema=None):
    """BASELINE configs[4]: step time of the DDP training step (fused HIP losses, device-side GT encoding, bf16 autocast)
    and the gradient all-reduce's bus bandwidth.  The all-reduce overlaps backward inside the step, so its bandwidth is
    measured on its own: the same payload (one flat buffer of the gradients' size, the bucketed hook's dtype) reduced
    back to back over RCCL; bus GB/s = bytes x 2 (N - 1) / N / time (ring convention).  `exposed_comm_ms` = step time
    minus the same step under no_sync().  amp: amp_setup's pair; None = bf16 autocast, no scaler.  ema: make_ema's."""
    import contextlib
    import json
    use_cuda = dev.type == 'cuda'
    dist = torch.distributed

    augment_events = []
    device_step = getattr(args, 'device_step', False)
    autocast_dtype, scaler = amp if amp is not None else (torch.bfloat16 if use_cuda else None, None)

    def run(n, first, sync_grads=True):
        ctx = contextlib.nullcontext() if (sync_grads or world == 1) else model.no_sync()
        with ctx:
            for step in range(first, first + n):
                if augment is not None:
                    images, annos = augmented_batch(augment, pool[step % len(pool)], rng, augment_events)
                else:
                    images, annos = pool[step % len(pool)]
                if encoders is not None:
                    annos = encode_targets(encoders, *annos)
                if ema is not None:
                    train_step_device(model, criterion, optimizer, images, annos, args.lambdas, autocast_dtype, args.max_grad_norm,
                                      world, scaler, ema)
                elif device_step:
                    train_step_device(model, criterion, optimizer, images, annos, args.lambdas, autocast_dtype, args.max_grad_norm,
                                      world, scaler)
                else:
                    train_step(model, criterion, optimizer, images, annos, args.lambdas, autocast_dtype)

    def timed(n, first, **kw):
        sharding.barrier(dev if use_cuda else None)
        t0 = time.perf_counter()
        run(n, first, **kw)
        sharding.barrier(dev if use_cuda else None)
        return sharding.max_over_ranks(time.perf_counter() - t0, dev if use_cuda else None) / n

    model.train()
    run(max(args.bench_warmup, 1), 0)
    del augment_events[:]
    step_s = timed(args.bench_steps, args.bench_warmup)
    extra = {}
    if device_step:
        extra['optimizer'] = 'device'
        extra['dropped_steps'] = int(optimizer.dropped_steps)
    if scaler is not None:
        extra['amp'] = 'fp16'
        extra['loss_scale'] = float(scaler.loss_scale)
        extra['overflow_steps'] = int(scaler.overflow_steps)
    if ema is not None:
        extra['ema'] = ema.decay
    if augment is not None:
        torch.cuda.synchronize(dev)               # the events are complete before they are read
        us =[a.elapsed_time(b) * 1e3 for a, b in augment_events]
        extra['augment_us'] = round(sum(us) / len(us), 1)
        extra['photo_probs'] = {'color_tint': args.color_tint_prob, 'gray': args.gray_prob, 'jpeg': args.jpeg_prob,
                                'jpeg_quality': args.jpeg_quality, 'annotation_jitter': args.annotation_jitter_prob}
    nosync_s = timed(max(args.bench_steps // 2, 1), 0, sync_grads=False) if world > 1 else step_s
    n_params = sum(p.numel() for p in model.parameters() if p.requires_grad)
    payload_dtype = torch.bfloat16 if (args.grad_compress == 'bf16' and use_cuda) else torch.float32
    nbytes = n_params * (2 if payload_dtype == torch.bfloat16 else 4)
    comm_ms = bus = None
    if world > 1:
        flat = torch.zeros(n_params, dtype=payload_dtype, device=dev)
        for _ in range(2):
            dist.all_reduce(flat)
        sharding.barrier(dev if use_cuda else None)
        t0 = time.perf_counter()
        reps = 5
        for _ in range(reps):
            dist.all_reduce(flat)
        sharding.barrier(dev if use_cuda else None)
        comm_s = sharding.max_over_ranks(time.perf_counter() - t0, dev if use_cuda else None) / reps
        comm_ms, bus = round(comm_s * 1e3, 3), round(nbytes * 2 * (world - 1) / world / comm_s / 1e9, 1)
    group = sharding.describe_group(dev if use_cuda else None)   # every rank takes part in the gather
    autocast_name = 'bf16 autocast' if amp is None else {torch.bfloat16: 'bf16 autocast', torch.float16: 'fp16 autocast + loss scaler',
                                                        None: 'fp32, no autocast'}[autocast_dtype]
    if rank == 0:
        print(json.dumps({
            'rccl': group,
            'metric': 'training images/sec (DDP step: forward + fused losses + backward + all-reduce + fused Adam)',
            'value': round(world * args.batch_size / step_s, 2), 'unit': 'images/sec', 'n_gpus': world,
            'steps': args.bench_steps, 'warmup': args.bench_warmup, 'ms_per_step': round(step_s * 1e3, 2),
            'config': {'workload': f'train_dist DDP, {args.square_length}x{args.square_length} crops, bs{args.batch_size}/GPU, '
                                   f'{autocast_name}, {describe_losses(args)} (BASELINE configs[4])',
                       'sync_bn': bool(args.sync_bn and world > 1), 'grad_payload': str(payload_dtype).replace('torch.', '')},
            'grad_allreduce': {'bytes': nbytes, 'ms': comm_ms, 'bus_GBps': bus,
                               'exposed_comm_ms': round(max(step_s - nosync_s, 0.0) * 1e3, 2) if world > 1 else 0.0},
            'data': ('COCO annotations: mask_miss rasterised, images augmented and targets encoded on the device'
                     if getattr(args, 'train_annotations', None) else 'synthetic raw images, augmented and encoded on the device')
                    if augment is not None else 'synthetic annotations, GT encoded on the device', **extra}))
    if dist.is_initialized():
        dist.destroy_process_group()


def main(argv=None):
    args = train_cli(argv)
    rank, local_rank, world = sharding.env_rank()
    use_cuda = torch.cuda.is_available()
    dev = torch.device('cuda', local_rank) if use_cuda else torch.device('cpu')
    if use_cuda:
        torch.cuda.set_device(dev)
        torch.backends.cudnn.benchmark = True
    sharding.init(device=dev if use_cuda else None)
    model, criterion = models.model_factory(args)
    model = model.to(dev)
    if use_cuda:
        model = model.to(memory_format=torch.channels_last)
    if world > 1 and args.sync_bn:
        model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)
    if args.freeze:
        freeze_backbone(model)
    optimizer = make_optimizer(args, model, world, use_cuda)
    autocast_dtype, scaler = amp_setup(args, dev, use_cuda)
    # continue a run (train_dist.py:219-233): weights, optimizer state and the epoch the LR schedule is at.  Before the DDP
    # wrap, so every rank loads the same state and the first broadcast has nothing to fix.
    ema = make_ema(args, model)
    if ema is None:
        model, optimizer, start_epoch, start_loss = load_checkpoint(args, model, optimizer, use_cuda, scaler)
    else:
        model, optimizer, start_epoch, start_loss = load_checkpoint(args, model, optimizer, use_cuda, scaler, ema)
    if args.resume and rank == 0:
        print(f'resumed {args.checkpoint_whole}: next epoch {start_epoch}, last train loss {start_loss:.4f}')
    if world > 1:
        model = torch.nn.parallel.DistributedDataParallel(model, device_ids=[local_rank] if use_cuda else None,
                                                          bucket_cap_mb=25, gradient_as_bucket_view=True)
        if args.grad_compress == 'bf16' and use_cuda:   # 375.5 MB instead of 750.9 MB over xGMI per step
            from torch.distributed.algorithms.ddp_comm_hooks import default_hooks
            model.register_comm_hook(None, default_hooks.bf16_compress_hook)
    os.makedirs(args.checkpoint_path, exist_ok=True)
    # a small rotating pool of synthetic batches per rank (generating targets on the host every step
    # would measure numpy, not the training step)
    # On the GPU the pool holds ANNOTATIONS and the targets are encoded on the device inside every step
    # (the reference's numpy encoder manages 17 samples/s per dataloader worker, data/factory.py:284).
    pool, encoders, augment, aug_rng = [], None, None, random.Random(1000 * rank + 7)
    if args.augment and not use_cuda:
        raise _lib.OgError('--augment warps on the device: it needs a GPU (offsetguided_amd has no CPU path)')
    if use_cuda:
        encoder.HeatMaps.include_jitter_offset = args.include_jitter_offset
        encoder.HeatMaps.include_background = args.include_background
        encoder.OffsetMaps.include_scale = args.include_scale
        encoders = encoder.factory_heads(['hmp', 'omp'], args.square_length, [4, 4], dev)
    if args.augment:
        # raw uint8 images on 640 x 480 canvases and their un-augmented annotations; every step draws a new crop of its entry
        photo = transforms.PhotoParams(tint_prob=args.color_tint_prob, gray_prob=args.gray_prob, jpeg_prob=args.jpeg_prob,
                                       jpeg_quality=args.jpeg_quality, jitter_prob=args.annotation_jitter_prob)
        augment = transforms.DeviceAugment(args.square_length, args, device=dev, photo_params=photo,
                                           np_rng=np.random.RandomState(1000 * rank + 11))
        if args.train_annotations:
            pool = coco_pool(args, rank, world, dev)
        for i in range(0 if args.train_annotations else 4):
            joints, n_persons = synthetic_annotations(1000 * rank + i, args.batch_size, 480, 640)
            pool.append((synthetic_raw_images(1000 * rank + i, joints, n_persons, 480, 640), joints, n_persons,
                         torch.from_numpy(n_persons).to(dev)))
    for i in range(0 if args.augment else 4):
        imgs = torch.randn(args.batch_size, 3, args.square_length, args.square_length, device=dev)
        if use_cuda:
            imgs = imgs.contiguous(memory_format=torch.channels_last)
            joints, n_persons = synthetic_annotations(1000 * rank + i, args.batch_size, args.square_length)
            pool.append((imgs, (torch.from_numpy(joints).to(dev), torch.from_numpy(n_persons).to(dev))))
        else:
            pool.append((imgs, synthetic_targets(1000 * rank + i, args.batch_size, args.square_length, dev,
                                                 background=args.include_background, jitter=args.include_jitter_offset,
                                                 scale=args.include_scale)))
    if args.bench:
        return bench_steps(args, model, criterion, optimizer, pool, encoders, dev, rank, world, augment, aug_rng,
                           None if args.opt_level is None else (autocast_dtype, scaler), **({} if ema is None else {'ema': ema}))
    batch_time = AverageMeter()   # over the whole run: the first steps (MIOpen find, allocator warm-up) do not bias an epoch
    # --epochs MORE epochs after a resume, as the reference counts them (train_dist.py:269)
    for epoch in range(start_epoch, start_epoch + args.epochs):
        model.train()
        losses, end, last_print = AverageMeter(), time.time(), -1
        for step in range(args.steps_per_epoch):
            adjust_learning_rate(args.learning_rate, world, optimizer, epoch, step, args.steps_per_epoch, args.warmup)
            if augment is not None:
                images, annos = augmented_batch(augment, pool[step % len(pool)], aug_rng)
            else:
                images, annos = pool[step % len(pool)]
            if encoders is not None:
                annos = encode_targets(encoders, *annos)
            if ema is not None:
                loss, _ = train_step_device(model, criterion, optimizer, images, annos, args.lambdas, autocast_dtype,
                                            args.max_grad_norm, world, scaler, ema)
            elif args.device_step:
                loss, _ = train_step_device(model, criterion, optimizer, images, annos, args.lambdas, autocast_dtype,
                                            args.max_grad_norm, world, scaler)
            else:
                loss, _ = train_step(model, criterion, optimizer, images, annos, args.lambdas, autocast_dtype)
            if step % args.print_freq == 0:
                if world > 1:  # averaged over ranks for logging only (train_dist.py:346-348, :458-466)
                    torch.distributed.all_reduce(loss)
                    loss = loss / world
                if use_cuda:
                    torch.cuda.synchronize()
                now = time.time()
                per_step = (now - end) / (step - last_print)   # steps since the last print (1 at step 0), not print_freq
                end, last_print = now, step
                if epoch > start_epoch or step > 0:            # the very first step is warm-up: not a speed sample
                    batch_time.update(per_step)
                losses.update(float(loss))
                if rank == 0:
                    print(f'epoch {epoch} [{step}/{args.steps_per_epoch}] loss {losses.val:.4f} ({losses.avg:.4f}) '
                          f'speed {world * args.batch_size / per_step:.1f} img/s'
                          + (f' grad norm {float(optimizer.last_grad_norm):.4g} dropped {int(optimizer.dropped_steps)}'
                             if args.device_step else '')
                          + (f' loss scale {float(scaler.loss_scale):g} overflows {int(scaler.overflow_steps)}'
                             if scaler is not None else ''))
        if rank == 0:
            models.save_model(os.path.join(args.checkpoint_path, f'PoseNet_{epoch}_epoch.pth'), epoch, losses.avg, model,
                              optimizer, amp_state=optim.amp_state_dict(scaler) if scaler is not None else None,
                              **({} if ema is None else {'ema_state': ema.state_dict()}))
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
