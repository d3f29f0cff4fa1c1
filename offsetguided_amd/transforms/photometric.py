"""The photometric and annotation-noise steps of the reference's training chain (data/factory.py:250-265) as parameter-drawing classes:
RandomApply (transforms/random.py), ColorTint, Gray, JpegCompression (transforms/image.py) and AnnotationJitter
(transforms/annotations.py:89-111), with the reference's names and defaults.  As with WarpAffineTransforms the parameters are drawn
here, with the reference's generators in the reference's order; the pixels and keypoints move in DeviceAugment (csrc/photometric.h
behind the warp, csrc/jpeg_sim.hip, the jitter of csrc/augment.hip).

Draw order of DeviceAugment, per image, after all matrices() draws of the batch: one `rng.uniform(0, 1)` gate each for jitter, jpeg,
tint, gray in this order -- a gate is drawn ONLY IF its probability is > 0, so that PhotoParams() leaves the random stream, the launches
and the outputs exactly as they are without it --, a step applied iff not (u > p) (RandomApply); a passed jitter gate draws
torch.rand(K, 2) per person in use (the CPU generator), a passed tint gate draws np_rng.randint(21) - 10, randint(81) - 40,
randint(61) - 30 at once.  On the device the order is the reference's: warp, [jitter], [jpeg], [tint], [gray], normalise."""
import random

import numpy as np
import torch

MODE_TINT, MODE_GRAY = 1, 2


class RandomApply:
    """draw() -> None (skipped) or the transform's own draw; the gate is the reference's `random.uniform(0, 1) > probability`."""

    def __init__(self, transform, probability):
        self.transform, self.probability = transform, probability

    def draw(self, rng=random, **kw):
        if rng.uniform(0, 1) > self.probability:
            return None
        return self.transform.draw(**kw)


class ColorTint:
    """draw() -> (dh, ds, dv) added to H in [0, 180), S and V in [0, 255] of the 8-bit HSV image, each clamped."""

    def draw(self, np_rng=np.random, **kw):
        return int(np_rng.randint(20 + 1)) - 10, int(np_rng.randint(80 + 1)) - 40, int(np_rng.randint(60 + 1)) - 30


class Gray:
    def draw(self, **kw):
        return True


class JpegCompression:
    def __init__(self, quality=50):
        self.quality = quality

    def draw(self, **kw):
        return self.quality


class AnnotationJitter:
    """draw(persons, keypoints) -> (persons, keypoints, 2) fp32 uniform noise u, one torch.rand(keypoints, 2) per person as the
    reference draws it; the device adds epsilon * ((u - 0.5 + shift) * 2) to x and y."""

    def __init__(self, shift=0, epsilon=0.5):
        self.shift, self.epsilon = shift, epsilon

    def draw(self, persons=0, keypoints=17, **kw):
        rows = [torch.rand(keypoints, 2) for _ in range(persons)]
        return torch.stack(rows).numpy() if rows else np.zeros((0, keypoints, 2), np.float32)


class PhotoParams:
    """Probabilities of the four steps (all off by default; the reference trains with tint 0.2 and keeps jitter 0.1 and jpeg 0.1
    commented out) and their fixed parameters."""

    def __init__(self, tint_prob=0, gray_prob=0, jpeg_prob=0, jpeg_quality=50, jitter_prob=0, jitter_epsilon=0.5, jitter_shift=0):
        self.tint_prob, self.gray_prob, self.jpeg_prob, self.jpeg_quality = tint_prob, gray_prob, jpeg_prob, jpeg_quality
        self.jitter_prob, self.jitter_epsilon, self.jitter_shift = jitter_prob, jitter_epsilon, jitter_shift

    def steps(self):
        """(name, RandomApply) in draw order, the steps with probability 0 left out."""
        every = (('jitter', AnnotationJitter(self.jitter_shift, self.jitter_epsilon), self.jitter_prob),
                 ('jpeg', JpegCompression(self.jpeg_quality), self.jpeg_prob),
                 ('tint', ColorTint(), self.tint_prob), ('gray', Gray(), self.gray_prob))
        return [(name, RandomApply(t, p)) for name, t, p in every if p > 0]


def draw_photo(params, n_persons, keypoints, rng=random, np_rng=None):
    """One dict per image {'jitter': noise or None, 'jpeg': quality or None, 'tint': (dh, ds, dv) or None, 'gray': True or None}."""
    np_rng = np.random if np_rng is None else np_rng
    steps = params.steps()
    out = []
    for n in n_persons:
        drawn = {'jitter': None, 'jpeg': None, 'tint': None, 'gray': None}
        for name, step in steps:
            drawn[name] = step.draw(rng, np_rng=np_rng, persons=int(n), keypoints=keypoints)
        out.append(drawn)
    return out


def photo_table(photo):
    """The (n, 4) int32 descriptor table {mode, dh, ds, dv} of the device epilogue for draw_photo's dicts."""
    table = np.zeros((len(photo), 4), np.int32)
    for i, d in enumerate(photo):
        if d['tint'] is not None:
            table[i] = (MODE_TINT,) + tuple(d['tint'])
        if d['gray']:
            table[i, 0] |= MODE_GRAY
    return table
