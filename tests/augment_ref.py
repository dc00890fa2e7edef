"""Two restatements of the augmentation of DESIGN.md 6c (kfnet_amd/augment.py, kfnet_amd/csrc/kfn_augment.hip), in numpy:

    augment64   fp64, built as the reference builds it, in passes: colour, rotate (NEAREST, fill 0), then resample.
    augment32   float32, fused like the kernel and in its operation order, from kfnet_amd.augment.descriptor: what the device
                must equal bit for bit.

numpy rounds every float32 operation and fuses nothing, so augment32's arrays are the kernel's registers."""
import math

import numpy as np

from kfnet_amd.augment import ENLARGE, SHRINK, TRANSLATE, descriptor

F = np.float32
AMBIGUITY = 1e-3        # a rotation source coordinate this close to a half-integer may round either way


def shrink_size(size, ratio):
    """tf.cast(size * ratio, tf.int32): the float32 product, truncated; at least 1."""
    return max(int(F(size) * F(ratio)), 1)


def round_half_away(s):
    t = np.trunc(s)
    return t + np.where(np.abs(s - t) >= 0.5, np.sign(s), 0).astype(s.dtype)      # s - t is exact


# ---- fp64, in passes -----------------------------------------------------------------------------------------------------
def colour64(frames, delta, factor):
    """random_brightness's + delta, then adjust_contrast about each frame's per-channel mean.  [B,H,W,3] -> fp64."""
    x = frames.astype(np.float64) + delta
    mean = x.mean(axis=(1, 2), keepdims=True)
    return (x - mean) * factor + mean


def rotation_sources64(angle, H, W):
    """(sx, sy) [H,W]: the source coordinates output pixel (x, y) of tf.contrib.image.rotate reads."""
    a = math.radians(angle)
    c, s = math.cos(a), math.sin(a)
    xo = ((W - 1) - (c * (W - 1) - s * (H - 1))) / 2.0
    yo = ((H - 1) - (s * (W - 1) + c * (H - 1))) / 2.0
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    return c * x - s * y + xo, s * x + c * y + yo


def rotate64(img, angle):
    """img [B,H,W,C] -> (rotated [B,H,W,C], ambiguous [H,W]): NEAREST, fill 0."""
    B, H, W, _ = img.shape
    sx, sy = rotation_sources64(angle, H, W)
    qx, qy = round_half_away(sx), round_half_away(sy)
    inside = (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
    qx, qy = np.where(inside, qx, 0).astype(int), np.where(inside, qy, 0).astype(int)
    out = np.where(inside[None, :, :, None], img[:, qy, qx], 0.0)
    amb = (np.abs(sx - np.floor(sx) - 0.5) < AMBIGUITY) | (np.abs(sy - np.floor(sy) - 0.5) < AMBIGUITY)
    return out, amb


def axis64(params, size, which):
    """(ok, lo, hi, frac) per output line of one axis, fp64."""
    i = np.arange(size)
    if params.mode == ENLARGE:
        inn = (params.y1 if which == 'y' else params.x1) * (size - 1) + i * params.ratio
        ok = (inn >= 0) & (inn <= size - 1)
        lo, hi = np.floor(inn), np.ceil(inn)
    else:
        new = shrink_size(size, params.ratio)
        ii = i - (size - new) // 2
        ok = (ii >= 0) & (ii < new)
        inn = ii * (size / new)
        lo = np.floor(inn)
        hi = np.minimum(lo + 1, size - 1)
    frac = inn - lo
    lo, hi = np.where(ok, lo, 0).astype(int), np.where(ok, hi, 0).astype(int)
    return ok, lo, hi, np.where(ok, frac, 0.0)


def resample64(img, params, amb=None):
    """The bilinear pass on the rotated image; returns (values [B,H,W,C], the output pixels with an ambiguous tap [H,W])."""
    B, H, W, _ = img.shape
    oy, t, b, ly = axis64(params, H, 'y')
    ox, l, r, lx = axis64(params, W, 'x')
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    T, Bm = img[:, t], img[:, b]
    top = T[:, :, l] + (T[:, :, r] - T[:, :, l]) * lx
    bot = Bm[:, :, l] + (Bm[:, :, r] - Bm[:, :, l]) * lx
    ok = oy[:, None] & ox[None, :]
    out = np.where(ok[None, :, :, None], top + (bot - top) * ly, 0.0)
    touched = np.zeros((H, W), bool)
    if amb is not None:
        touched = ok & (amb[t][:, l] | amb[t][:, r] | amb[b][:, l] | amb[b][:, r])
    return out, touched


def augment64(frames, labels, params):
    """(frame values before rounding [B,H,W,3], label channels before the mask threshold [B,H,W,4] or None, the output
    pixels that read an ambiguous rotation source [H,W]) in fp64."""
    B, H, W, _ = frames.shape
    col = colour64(frames, params.delta, params.factor) if (params.delta != 0.0 or params.factor != 1.0) else frames.astype(np.float64)
    lab = None if labels is None else labels.astype(np.float64)
    if params.mode == TRANSLATE:
        return col, lab, np.zeros((H, W), bool)
    col, amb = rotate64(col, params.angle)
    col, touched = resample64(col, params, amb)
    if lab is not None:
        lab = resample64(rotate64(lab, params.angle)[0], params)[0]
    return col, lab, touched


def finish_frames(values):
    return np.clip(np.rint(values), 0, 255).astype(np.uint8)


def finish_labels(values):
    out = values.copy()
    out[..., 3] = (values[..., 3] >= 1.0)
    return out


# ---- float32, fused ------------------------------------------------------------------------------------------------------
def _axis32(mode, idx, size, o0, d, new_n, off, scale):
    if mode == ENLARGE:
        inn = F(o0) + idx.astype(F) * F(d)
        ok = (inn >= F(0)) & (inn <= F(size - 1))
        fl = np.floor(inn)
        lo, hi = fl.astype(np.int64), np.ceil(inn).astype(np.int64)
    else:
        ii = idx - off
        ok = (ii >= 0) & (ii < new_n)
        inn = ii.astype(F) * F(scale)
        fl = np.floor(inn)
        lo = np.clip(fl.astype(np.int64), 0, size - 1)
        hi = np.minimum(lo + 1, size - 1)
    frac = inn - fl
    assert inn.dtype == F and frac.dtype == F
    return ok, np.where(ok, lo, 0), np.where(ok, hi, 0), np.where(ok, frac, F(0))


def _gather32(src, d, rows, cols):
    """src [B,H,W,C] float32 (already colour-adjusted for frames) at output pixels rows x cols -> (values float32
    [B,len(rows),len(cols),C], ok [len(rows),len(cols)], the source pixel lists of the four taps for the bound)."""
    B, H, W, _ = src.shape
    assert src.dtype == F
    if d.mode == TRANSLATE:
        return src[:, rows][:, :, cols], None
    oy, t, b, ly = _axis32(d.mode, rows, H, d.y0, d.dy, d.new_h, d.off_y, d.scale_y)
    ox, l, r, lx = _axis32(d.mode, cols, W, d.x0, d.dx, d.new_w, d.off_x, d.scale_x)
    ok = oy[:, None] & ox[None, :]
    rot = np.array(d.rot[:], dtype=F)

    def tap(y, x):
        yy, xx = np.broadcast_arrays(y[:, None], x[None, :])
        if d.has_rotation:
            fx, fy = xx.astype(F), yy.astype(F)
            sx = (rot[0] * fx + rot[1] * fy) + rot[2]
            sy = (rot[3] * fx + rot[4] * fy) + rot[5]
            assert sx.dtype == F and sy.dtype == F
            rx, ry = round_half_away(sx), round_half_away(sy)
            inside = (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
            xx, yy = np.where(inside, rx, 0).astype(np.int64), np.where(inside, ry, 0).astype(np.int64)
        else:
            inside = np.ones(yy.shape, bool)
        return np.where((inside & ok)[None, :, :, None], src[:, yy, xx], F(0))
    tl, tr, bl, br = tap(t, l), tap(t, r), tap(b, l), tap(b, r)
    lx, ly = lx[None, None, :, None], ly[None, :, None, None]
    top = tl + (tr - tl) * lx
    bot = bl + (br - bl) * lx
    val = top + (bot - top) * ly
    assert val.dtype == F
    return np.where(ok[None, :, :, None], val, F(0)), (tl, tr, bl, br)


def channel_sums(frames):
    """[B,4] exact integer sums, the fourth word 0."""
    s = np.zeros((frames.shape[0], 4), np.uint32)
    s[:, :3] = frames.astype(np.uint64).sum(axis=(1, 2))
    return s


def colour32(frames, d):
    x = frames.astype(F)
    if not d.has_colour:
        return x
    B, H, W, _ = frames.shape
    delta, factor = F(d.delta), F(d.factor)
    sums = channel_sums(frames)[:, :3].astype(np.float64)
    mean = (sums / np.float64(H * W) + np.float64(delta)).astype(F)[:, None, None, :]
    out = ((x + delta) - mean) * factor + mean
    assert out.dtype == F
    return out


def augment32(frames, labels, params, label_stride=1, raw=False):
    """(frames uint8 [B,H,W,3], labels float32 [B,H/s,W/s,4] or None); raw: the float32 values before the frame's rounding
    and the mask's threshold, and the taps of the frames (for the bound of test_augment_host)."""
    B, H, W, _ = frames.shape
    d = descriptor(params, B, H, W, label_stride)
    fv, taps = _gather32(colour32(frames, d), d, np.arange(H), np.arange(W))
    lv = None
    if labels is not None:
        s = label_stride
        lv, _ = _gather32(np.ascontiguousarray(labels, dtype=F), d, np.arange(0, H, s), np.arange(0, W, s))
    if raw:
        return fv, lv, taps
    return finish_frames(fv), None if lv is None else finish_labels(lv)


def make_batch(B, H, W, seed):
    """Frames with smooth and noisy parts and saturated patches; labels with a 0/1 mask that has fractional cells."""
    rng = np.random.default_rng([seed, B, H, W])
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    base = 128 + 100 * np.sin(0.21 * x + 0.1 * seed)[..., None] * np.cos(0.17 * y)[..., None] * np.array([1.0, 0.7, -0.8])
    frames = np.clip(base[None] + rng.integers(-40, 41, size=(B, H, W, 3)), 0, 255).astype(np.uint8)
    frames[:, :H // 4, :W // 4] = 255
    frames[:, -(H // 4):, -(W // 4):] = 0
    labels = rng.normal(size=(B, H, W, 4)).astype(F)
    labels[..., 3] = (rng.uniform(size=(B, H, W)) < 0.8)
    labels[:, ::3, ::5, 3] = 0.5
    return frames, labels
