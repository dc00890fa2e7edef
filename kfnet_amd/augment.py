"""Augmenting a training batch on the device: the reference's data_augmentation (KFNet/train.py:168-193) and
image_augmentation (KFNet/util.py:66-136), with one parameter set per batch as there.  DESIGN.md 6c holds the definitions.

    p = draw(seed, step)                          the parameters of update number `step`: a function of (seed, step) alone
    d = descriptor(p, B, H, W, label_stride)      kfn_augment_desc: every derived constant in fp64, rounded once to fp32
    frames, labels = Augmenter(B, H, W)(frames_u8, labels, p)

The draws are numpy's, not TensorFlow's random stream: the distributions are the reference's, the numbers are not.  There
is no fallback: a missing entry point or an unsupported shape raises.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from .staging import check_size, current_stream, stage

TRANSLATE, ENLARGE, SHRINK = 0, 1, 2
MAX_ANGLE = 30.0              # degrees, KFNet/util.py:92,110
MAX_BOX_ORIGIN = 0.2          # :97-98
MIN_RATIO = 0.8               # :99,115
MAX_DELTA = 20.0              # KFNet/train.py:178
CONTRAST = (0.8, 1.2)         # :179
BRANCHES = (0.1, 0.55)        # KFNet/util.py:134


class AugmentParams(object):
    """mode (TRANSLATE / ENLARGE / SHRINK), angle in degrees, the box origin (x1, y1) and its side `ratio` as fractions of
    the image (ENLARGE), the shrink `ratio` (SHRINK), the brightness `delta` in grey levels and the contrast `factor`.
    delta = 0 and factor = 1 switch the colour adjustment off."""
    __slots__ = ('mode', 'angle', 'x1', 'y1', 'ratio', 'delta', 'factor')

    def __init__(self, mode=TRANSLATE, angle=0.0, x1=0.0, y1=0.0, ratio=1.0, delta=0.0, factor=1.0):
        if mode not in (TRANSLATE, ENLARGE, SHRINK):
            raise ValueError('unknown augmentation mode %r' % (mode,))
        self.mode, self.angle, self.x1, self.y1 = int(mode), float(angle), float(x1), float(y1)
        self.ratio, self.delta, self.factor = float(ratio), float(delta), float(factor)

    def __repr__(self):
        return 'AugmentParams(%s)' % ', '.join('%s=%r' % (k, getattr(self, k)) for k in self.__slots__)


def draw(seed, step):
    """The parameters of update number `step` (from 0).  u = default_rng([seed, step]).random(7) in the fixed order branch,
    angle, x1, y1, ratio, brightness, contrast: like train.batch_indices a function of its arguments alone, so a resumed run
    continues the same stream."""
    u = np.random.default_rng([int(seed), int(step)]).random(7)
    mode = TRANSLATE if u[0] < BRANCHES[0] else ENLARGE if u[0] < BRANCHES[1] else SHRINK
    x1, y1 = MAX_BOX_ORIGIN * u[2], MAX_BOX_ORIGIN * u[3]
    if mode == ENLARGE:
        ratio = MIN_RATIO + u[4] * (1.0 - max(x1, y1) - MIN_RATIO)
    else:
        ratio = MIN_RATIO + (1.0 - MIN_RATIO) * u[4]
    return AugmentParams(mode, -MAX_ANGLE + 2.0 * MAX_ANGLE * u[1], x1, y1, ratio, -MAX_DELTA + 2.0 * MAX_DELTA * u[5],
                         CONTRAST[0] + (CONTRAST[1] - CONTRAST[0]) * u[6])


def descriptor(params, B, H, W, label_stride=8):
    """kfn_augment_desc of `params` for a batch [B,H,W]: the one place where the constants of DESIGN.md 6c are derived, in
    fp64, each rounded to fp32 once (ctypes does the rounding)."""
    p = params
    d = _lib.AugmentDesc(B=B, H=H, W=W, label_stride=label_stride, mode=p.mode)
    d.has_colour = int(p.delta != 0.0 or p.factor != 1.0)
    d.delta, d.factor = p.delta, p.factor
    d.rot = (C.c_float * 6)(1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    if p.mode == TRANSLATE:
        return d
    d.has_rotation = int(p.angle != 0.0)
    if d.has_rotation:       # tf.contrib.image.angles_to_projective_transforms
        a = math.radians(p.angle)
        c, s = math.cos(a), math.sin(a)
        xo = ((W - 1) - (c * (W - 1) - s * (H - 1))) / 2.0
        yo = ((H - 1) - (s * (W - 1) + c * (H - 1))) / 2.0
        d.rot = (C.c_float * 6)(c, -s, xo, s, c, yo)
    if p.mode == ENLARGE:    # crop_and_resize of the box (y1, x1, y1 + ratio, x1 + ratio) to the image size
        d.y0, d.dy = p.y1 * (H - 1), p.ratio
        d.x0, d.dx = p.x1 * (W - 1), p.ratio
        return d
    r = np.float32(p.ratio)  # tf.cast(crop_size * ratio, tf.int32): a float32 product, truncated
    d.new_h = max(int(np.float32(H) * r), 1)
    d.new_w = max(int(np.float32(W) * r), 1)
    d.off_y, d.off_x = (H - d.new_h) // 2, (W - d.new_w) // 2
    d.scale_y, d.scale_x = H / d.new_h, W / d.new_w
    return d


class Augmenter(object):
    """kfn_augment_batch with its buffers, for users outside the trainer: aug(frames, labels, params) on uint8 [B,H,W,3]
    and float32 [B,H,W,4] (or labels None) returns device tensors (frames [B,H,W,3] uint8, labels [B,H/s,W/s,4] or None) that
    the next call overwrites."""

    def __init__(self, B, H, W, label_stride=8, device='cuda:0'):
        import torch
        if B < 1:
            raise ValueError('batch must be >= 1')
        check_size(H, W, 'the height and width of an augmented batch')
        if label_stride not in (1, 8):
            raise ValueError('label_stride must be 1 or 8')
        self.lib = _lib.load()
        self.torch, self.device = torch, torch.device(device)
        self.shape, self.label_stride = (B, H, W), label_stride
        with torch.cuda.device(self.device):
            self.frames_in = torch.zeros((B, H, W, 3), dtype=torch.uint8, device=self.device)
            self.frames_out = self.labels_in = None        # made on first use: the trainer brings its own frames
            self.labels_out = torch.zeros((B, H // label_stride, W // label_stride, 4), dtype=torch.float32, device=self.device)
            self.sums = torch.zeros((B, 4), dtype=torch.int32, device=self.device)

    def launch(self, params, frames_in, labels_in, frames_out, labels_out, stream):
        """The call itself, on device tensors (labels both None for frames only)."""
        B, H, W = self.shape
        d = descriptor(params, B, H, W, self.label_stride)
        _lib.check(self.lib.kfn_augment_batch(C.byref(d), frames_in.data_ptr(), None if labels_in is None else labels_in.data_ptr(),
                                              frames_out.data_ptr(), None if labels_out is None else labels_out.data_ptr(),
                                              self.sums.data_ptr(), stream), 'kfn_augment_batch')

    def pixel_map(self, params, camera, out, stream):
        """kfn_augment_pixel_map: the normalised pixel map of `camera` (a kfnet_amd.labels.DepthCamera) carried through the
        augmentation of `params` (KFNet/train.py:181-187, channels 7-8 of the bundle), into the device tensor out
        [H/s,W/s,2] float32.  One parameter set serves the batch, so one map serves every frame."""
        from .reproj import camera_constants
        B, H, W = self.shape
        s = self.label_stride
        if tuple(out.shape) != (H // s, W // s, 2) or out.dtype != self.torch.float32:
            raise ValueError('the pixel map must be float32 [%d,%d,2], got %s' % (H // s, W // s, tuple(out.shape)))
        d = descriptor(params, B, H, W, s)
        u, v, inv_fx, inv_fy = camera_constants(camera)
        _lib.check(self.lib.kfn_augment_pixel_map(C.byref(d), u, v, inv_fx, inv_fy, out.data_ptr(), stream), 'kfn_augment_pixel_map')

    def stage(self, frames_u8, labels):
        """Copies a batch into the staging buffers; returns (frames, labels or None) on the device."""
        torch = self.torch
        B, H, W = self.shape
        stage(self.frames_in, frames_u8, torch.uint8, (B, H, W, 3), 'frames')
        if labels is None:
            return self.frames_in, None
        # labels of any float type are converted, and the buffer is made only for labels that pass: torch's own copy
        lb = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(labels, dtype=np.float32))
        if tuple(lb.shape) != (B, H, W, 4):
            raise ValueError('augmentation needs full-resolution labels float32 [%d,%d,%d,4], got %s: interpolating an '
                             'already sub-sampled label is a different function' % (B, H, W, tuple(lb.shape)))
        if self.labels_in is None:
            self.labels_in = torch.zeros((B, H, W, 4), dtype=torch.float32, device=self.device)
        self.labels_in.copy_(lb.to(torch.float32), non_blocking=True)
        return self.frames_in, self.labels_in

    def __call__(self, frames_u8, labels, params):
        with self.torch.cuda.device(self.device):
            fin, lin = self.stage(frames_u8, labels)
            if self.frames_out is None:
                self.frames_out = self.torch.zeros_like(self.frames_in)
            lout = None if lin is None else self.labels_out
            self.launch(params, fin, lin, self.frames_out, lout, current_stream(self.device))
        return self.frames_out, lout
