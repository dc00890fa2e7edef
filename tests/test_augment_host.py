"""CPU tests of the training augmentation (kfnet_amd/augment.py): the fp64 restatement of tests/augment_ref.py
on cases known by hand and against torch's grid_sample, the float32 restatement -- what the kernel must equal bit for bit,
tests/test_gpu_augment.py -- against the fp64 one within a derived bound, the draws, the new exports' argument checks and
the command line's refusals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import augment_ref as R
from kfnet_amd import _lib
from kfnet_amd.augment import ENLARGE, SHRINK, TRANSLATE, AugmentParams, descriptor, draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the inputs of the comparisons between implementations: sizes, angles (degrees), and the box / the shrink ratio
SIZES = [(48, 64), (40, 56), (480, 640)]
ANGLES = [17.0, -29.0, 3.5]
BOX = (0.13, 0.07, 0.83)
MAX_LEFT_OUT = 0.03


# -- 1. the fp64 restatement on cases known by hand ----------------------------------------------------------------------------
def _image(H, W, C=2, seed=0):
    return np.random.default_rng(seed).normal(size=(1, H, W, C))


def test_angle_zero_with_the_whole_image_as_the_box_is_the_identity():
    img = _image(16, 24)
    rot, amb = R.rotate64(img, 0.0)
    assert np.array_equal(rot, img) and not amb.any()
    out, _ = R.resample64(rot, AugmentParams(ENLARGE, 0.0, 0.0, 0.0, 1.0))
    assert np.array_equal(out, img)


def test_ninety_degrees_on_a_square_is_rot90():
    """rotate's output pixel (x, y) reads source (cos a x - sin a y + xo, sin a x + cos a y + yo): at a = 90 degrees on 16x16
    that is (15 - y, x), so out[y, x] = img[x, 15 - y]: the first output row is the last source column, np.rot90 with k = 1
    (counter-clockwise as the array is printed).  cos 90 is 6e-17, far inside the rounding to the nearest pixel."""
    img = _image(16, 16)
    rot, _ = R.rotate64(img, 90.0)
    assert np.array_equal(rot[0, 0], img[0, :, 15]) and np.array_equal(rot[0, :, 0], img[0, 0, ::-1])
    assert np.array_equal(rot[0], np.rot90(img[0], k=1, axes=(0, 1)))
    assert not np.array_equal(rot[0], np.rot90(img[0], k=-1, axes=(0, 1)))
    back, _ = R.rotate64(rot, -90.0)
    assert np.array_equal(back, img)


def test_shrink_ratio_one_is_the_identity_and_an_odd_pad_puts_the_extra_row_at_the_bottom():
    img = _image(16, 24)
    out, _ = R.resample64(img, AugmentParams(SHRINK, 0.0, ratio=1.0))
    assert np.array_equal(out, img)
    # 16 rows to 15: one row of padding, off = 0, so the zero row is the LAST one; 24 columns to int(24 * 15.5/16) = 23: the last
    ratio = 15.5 / 16
    assert R.shrink_size(16, ratio) == 15 and R.shrink_size(24, ratio) == 23
    ones = np.ones((1, 16, 24, 1))
    out, _ = R.resample64(ones, AugmentParams(SHRINK, 0.0, ratio=ratio))
    assert np.all(out[0, :15, :23] == 1.0) and np.all(out[0, 15] == 0.0) and np.all(out[0, :, 23] == 0.0)
    # 16 rows to 13: three rows of padding, one above and two below
    ratio = 13.5 / 16
    out, _ = R.resample64(ones, AugmentParams(SHRINK, 0.0, ratio=ratio))
    assert R.shrink_size(16, ratio) == 13
    assert np.all(out[0, 0] == 0.0) and np.all(out[0, 1:14, 3:22] == 1.0) and np.all(out[0, 14:] == 0.0)


def test_fill_pixels_are_not_colour_adjusted_and_the_mask_threshold_is_at_one():
    frames, labels = R.make_batch(1, 16, 24, 1)
    p = AugmentParams(ENLARGE, 30.0, 0.0, 0.0, 1.0, delta=15.0, factor=1.2)
    f, l = R.augment32(frames, labels, p)
    assert f[0, 0, 0].tolist() == [0, 0, 0] and f[0, -1, -1].tolist() == [0, 0, 0]      # rotated-in corners
    assert set(np.unique(l[..., 3])) == {0.0, 1.0}
    fv, lv, _ = R.augment32(frames, labels, p, raw=True)
    assert np.array_equal(l[..., 3] == 1.0, lv[..., 3] >= 1.0) and ((lv[..., 3] > 0) & (lv[..., 3] < 1)).any()
    assert np.array_equal(l[..., :3], lv[..., :3])                                       # xyz stay as interpolated


# -- 2. the fp64 restatement against an independent implementation -----------------------------------------------------------------
def _grid_sample_pipeline(img, p):
    """rotate (nearest) then resample (bilinear) with torch.nn.functional.grid_sample, align_corners=True, fp64."""
    import torch
    import torch.nn.functional as Fn
    B, H, W, Cc = img.shape
    x = torch.from_numpy(img).permute(0, 3, 1, 2)

    def sample(t, sx, sy, mode):
        g = torch.stack([2.0 * torch.from_numpy(sx) / (W - 1) - 1.0, 2.0 * torch.from_numpy(sy) / (H - 1) - 1.0], dim=-1)
        return Fn.grid_sample(t, g[None].expand(B, -1, -1, -1), mode=mode, padding_mode='zeros', align_corners=True)
    sx, sy = R.rotation_sources64(p.angle, H, W)
    rot = sample(x, sx, sy, 'nearest')
    i, j = np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64)
    if p.mode == ENLARGE:
        iy, ix = p.y1 * (H - 1) + i * p.ratio, p.x1 * (W - 1) + j * p.ratio
        oky, okx = (iy >= 0) & (iy <= H - 1), (ix >= 0) & (ix <= W - 1)
    else:
        nh, nw = R.shrink_size(H, p.ratio), R.shrink_size(W, p.ratio)
        ii, jj = i - (H - nh) // 2, j - (W - nw) // 2
        iy, ix = ii * (H / nh), jj * (W / nw)
        oky, okx = (ii >= 0) & (ii < nh), (jj >= 0) & (jj < nw)
    gy, gx = np.meshgrid(iy, ix, indexing='ij')
    out = sample(rot, gx, gy, 'bilinear').permute(0, 2, 3, 1).numpy()
    return np.where((oky[:, None] & okx[None, :])[None, :, :, None], out, 0.0)


@pytest.mark.parametrize('size', SIZES, ids=['%dx%d' % s for s in SIZES])
def test_fp64_restatement_against_grid_sample(size):
    H, W = size
    img = _image(H, W, C=3, seed=H)
    for angle in ANGLES:
        for p in (AugmentParams(ENLARGE, angle, *BOX), AugmentParams(SHRINK, angle, ratio=0.87)):
            rot, amb = R.rotate64(img, p.angle)
            got, left_out = R.resample64(rot, p, amb)
            want = _grid_sample_pipeline(img, p)
            share = float(left_out.mean())
            err = float(np.abs(got - want)[:, ~left_out].max())
            print('%dx%d angle %5.1f mode %d: max err %.3g, left out %.2f %%' % (H, W, angle, p.mode, err, 100 * share))
            assert share < MAX_LEFT_OUT
            assert err <= 1e-9          # unit-variance data; the two differ by fp64 rounding of the sample positions
            assert np.abs(want).max() > 1.0


# -- 3. the float32 restatement against the fp64 one ---------------------------------------------------------------------------
def _bound(taps32, values64_taps, size, largest):
    """Bound on |float32 value - fp64 value| of one output pixel, from DESIGN.md 6c's operation list.

    Index arithmetic.  in = o0 + f32(i) d (enlarge) or f32(ii) scale (shrink) has at most four roundings -- the constants o0
    and d / scale (half an ulp each, the second one multiplied by i < size), the product and the sum -- all on numbers below
    size: |in32 - in| <= 4 ulp(size) =: E, ulp(size) = 2^-23 * 2^floor(log2 size).  floor() then either agrees, and the weight
    frac = in - floor(in) (exact) is off by E, or in32 and in straddle an integer n, where the fp64 cell [n-1, n] has weight
    1 - e and the float32 cell [n, n+1] weight e', e + e' <= E: both values are within weight * (difference of their own cell's
    taps) of the tap at n.  Either way the error from one axis is at most E times the largest tap difference over the cells of
    BOTH restatements; the two axes add.  The rotation's own fp32 error moves a tap only where its source coordinate is within
    ~1e-4 of a half-integer, and those pixels are left out (AMBIGUITY = 1e-3).

    Values.  A colour-adjusted tap is four rounded operations on numbers below `largest` plus the rounded mean: 5 ulp; the two
    lerps add three operations each on numbers below 2 * largest: 12 ulp(largest) more.  Taken as 32 * 2^-24 * largest."""
    E = 4.0 * 2.0 ** -23 * 2.0 ** np.floor(np.log2(size))
    def spread(t):
        tl, tr, bl, br = [np.asarray(a, np.float64) for a in t]
        dx = np.maximum(np.abs(tr - tl), np.abs(br - bl))
        dy = np.maximum(np.abs(bl - tl), np.abs(br - tr))
        return dx + dy
    return E * (spread(taps32) + spread(values64_taps)) + 32.0 * 2.0 ** -24 * largest


def _taps64(img, p):
    oy, t, b, _ = R.axis64(p, img.shape[1], 'y')
    ox, l, r, _ = R.axis64(p, img.shape[2], 'x')
    T, Bm = img[:, t], img[:, b]
    return T[:, :, l], T[:, :, r], Bm[:, :, l], Bm[:, :, r]


@pytest.mark.parametrize('size', SIZES, ids=['%dx%d' % s for s in SIZES])
def test_float32_restatement_against_fp64_within_the_derived_bound(size):
    H, W = size
    frames, labels = R.make_batch(1, H, W, 2)
    for angle in ANGLES:
        for p in (AugmentParams(ENLARGE, angle, *BOX, delta=-12.5, factor=1.15), AugmentParams(SHRINK, angle, ratio=0.87, delta=7.0, factor=0.85),
                  AugmentParams(ENLARGE, angle, *BOX)):
            f64, l64, left_out = R.augment64(frames, labels, p)
            f32, l32, ftaps = R.augment32(frames, labels, p, raw=True)
            share = float(left_out.mean())
            assert share < MAX_LEFT_OUT
            col = R.colour64(frames, p.delta, p.factor) if (p.delta or p.factor != 1.0) else frames.astype(np.float64)
            keep = ~left_out
            worst = 0.0
            for got, want, src, taps32 in ((f32, f64, col, ftaps), (l32, l64, labels.astype(np.float64), None)):
                rot = R.rotate64(src, p.angle)[0]
                if taps32 is None:
                    d = descriptor(p, 1, H, W, 1)
                    taps32 = R._gather32(np.ascontiguousarray(labels, dtype=np.float32), d, np.arange(H), np.arange(W))[1]
                bound = _bound(taps32, _taps64(rot, p), max(H, W), max(float(np.abs(src).max()), 255.0))
                ratio = (np.abs(got.astype(np.float64) - want) / bound)[:, keep]
                worst = max(worst, float(ratio.max()))
            # the rounded frames: a grey level apart at most, and only where the value sits within the bound of a tie
            a, b = R.finish_frames(f32), R.finish_frames(f64)
            assert int(np.abs(a.astype(int) - b.astype(int))[:, keep].max()) <= 1
            print('%dx%d angle %5.1f mode %d colour %d: worst error / bound %.3f, left out %.2f %%' %
                  (H, W, angle, p.mode, int(p.delta != 0), worst, 100 * share))
            assert worst <= 1.0


def test_translate_mode_is_colour_only_and_labels_are_sub_sampled():
    frames, labels = R.make_batch(2, 16, 24, 3)
    f, l = R.augment32(frames, labels, AugmentParams(TRANSLATE, 25.0, 0.1, 0.1, 0.85), label_stride=8)
    assert np.array_equal(f, frames)
    want = labels[:, ::8, ::8].copy()
    want[..., 3] = want[..., 3] >= 1.0
    assert np.array_equal(l, want)
    p = AugmentParams(TRANSLATE, delta=10.0, factor=1.1)
    f, _ = R.augment32(frames, None, p)
    f64, _, _ = R.augment64(frames, None, p)
    assert int(np.abs(f.astype(int) - R.finish_frames(f64).astype(int)).max()) <= 1 and not np.array_equal(f, frames)


def test_descriptor_rounds_fp64_constants_once():
    p = AugmentParams(ENLARGE, 17.0, 0.13, 0.07, 0.83, delta=-3.3, factor=1.07)
    d = descriptor(p, 3, 48, 64, 8)
    a = np.radians(17.0)
    assert d.struct_size == C.sizeof(_lib.AugmentDesc) == 26 * 4
    assert (d.B, d.H, d.W, d.label_stride, d.mode, d.has_rotation, d.has_colour) == (3, 48, 64, 8, 1, 1, 1)
    xo = (63 - (np.cos(a) * 63 - np.sin(a) * 47)) / 2
    yo = (47 - (np.sin(a) * 63 + np.cos(a) * 47)) / 2
    want = [np.cos(a), -np.sin(a), xo, np.sin(a), np.cos(a), yo]
    assert [np.float32(v) for v in d.rot[:]] == [np.float32(v) for v in want]
    assert (np.float32(d.y0), np.float32(d.dy), np.float32(d.x0)) == (np.float32(0.07 * 47), np.float32(0.83), np.float32(0.13 * 63))
    s = descriptor(AugmentParams(SHRINK, -5.0, ratio=0.9), 1, 40, 56)
    assert (s.new_h, s.new_w, s.off_y, s.off_x) == (36, 50, 2, 3) and not s.has_colour
    assert np.float32(s.scale_y) == np.float32(40 / 36) and np.float32(s.scale_x) == np.float32(56 / 50)
    t = descriptor(AugmentParams(TRANSLATE, 20.0), 1, 8, 8)
    assert t.mode == 0 and not t.has_rotation and list(t.rot[:]) == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    assert not descriptor(AugmentParams(ENLARGE, 0.0, 0.0, 0.0, 1.0), 1, 8, 8).has_rotation
    with pytest.raises(ValueError):
        AugmentParams(3)


# -- 5. draws, exports, command line -------------------------------------------------------------------------------------------
def test_draws_depend_on_seed_and_step_alone_and_stay_inside_the_reference_ranges():
    modes = np.zeros(3)
    for step in range(10000):
        p = draw(4, step)
        modes[p.mode] += 1
        assert -30.0 <= p.angle <= 30.0 and 0.0 <= p.x1 <= 0.2 and 0.0 <= p.y1 <= 0.2
        assert -20.0 <= p.delta <= 20.0 and 0.8 <= p.factor <= 1.2
        if p.mode == ENLARGE:
            assert 0.8 <= p.ratio <= 1.0 - max(p.x1, p.y1) + 1e-15        # the box stays inside the image
        else:
            assert 0.8 <= p.ratio <= 1.0
    share = modes / modes.sum()
    print('branch shares', share)
    # binomial standard deviations at n = 10000: 0.003, 0.005, 0.005; five of them
    assert abs(share[0] - 0.10) < 0.015 and abs(share[1] - 0.45) < 0.025 and abs(share[2] - 0.45) < 0.025
    a, b = draw(4, 77), draw(4, 77)
    assert repr(a) == repr(b)
    draw(4, 78)
    assert repr(draw(4, 77)) == repr(a)                                   # no hidden state
    assert repr(draw(5, 77)) != repr(a) and repr(draw(4, 78)) != repr(a)
    u = np.random.default_rng([4, 77]).random(7)
    assert a.angle == -30.0 + 60.0 * u[1] and a.delta == -20.0 + 40.0 * u[5] and a.factor == 0.8 + (1.2 - 0.8) * u[6]


def test_augment_entry_points_are_exported_and_check_their_arguments_without_a_device():
    lib = _lib.load()
    assert lib.kfn_abi_version() == 13
    for name in ('kfn_frame_channel_sums', 'kfn_augment_batch'):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    ARG = -1
    a = np.zeros(4096, np.float32)
    b = np.zeros(4096, np.float32)
    buf, out = a.ctypes.data, b.ctypes.data
    assert buf % 16 == 0 and out % 16 == 0

    def call(p=AugmentParams(ENLARGE, 10.0, 0.1, 0.1, 0.85, delta=1.0), size=(1, 8, 8), stride=8, fin=buf, lin=buf, fout=out, lout=out,
             sums=out, **fields):
        d = descriptor(p, size[0], size[1], size[2], stride)
        for k, v in fields.items():
            setattr(d, k, v)
        return lib.kfn_augment_batch(C.byref(d), fin, lin, fout, lout, sums, None)
    for size in ((1, 8, 12), (1, 12, 8), (1, 0, 8), (1, 4, 8), (0, 8, 8), (1, 8, 7)):
        assert call(size=size) == ARG, size
        assert b'multiples of 8' in lib.kfn_last_error()
        assert lib.kfn_frame_channel_sums(buf, size[0], size[1], size[2], out, None) == ARG, size
    for stride in (0, 2, 4, 16):
        assert call(stride=stride) == ARG, stride
        assert b'label_stride' in lib.kfn_last_error()
    assert call(fout=buf) == ARG and b'in place' in lib.kfn_last_error()
    assert call(fin=None) == ARG and call(fout=None) == ARG
    assert call(lin=None) == ARG and call(lout=None) == ARG            # one label pointer without the other
    assert call(sums=None) == ARG and b'sums' in lib.kfn_last_error()  # colour needs the sums
    assert call(struct_size=8) == ARG and call(struct_size=C.sizeof(_lib.AugmentDesc) + 4) == ARG
    assert b'struct_size' in lib.kfn_last_error()
    assert call(mode=3) == ARG
    assert call(p=AugmentParams(SHRINK, 0.0, ratio=0.9), new_h=9) == ARG and call(p=AugmentParams(SHRINK, 0.0, ratio=0.9), off_x=5) == ARG
    assert lib.kfn_augment_batch(None, buf, buf, out, out, out, None) == ARG
    assert lib.kfn_frame_channel_sums(None, 1, 8, 8, out, None) == ARG and lib.kfn_frame_channel_sums(buf, 1, 8, 8, None, None) == ARG
    assert lib.kfn_frame_channel_sums(buf + 4, 1, 8, 8, out, None) == ARG
    assert not a.any() and not b.any()                                 # nothing was written


def _cli(*args):
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    return subprocess.run([sys.executable, '-m', 'kfnet_amd.SCoordNet.train'] + list(args), cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def test_command_line_has_the_flags_and_refuses_augment_without_full_labels(tmp_path):
    from kfnet_amd.SCoordNet.train import build_parser
    r = _cli('--help')
    assert r.returncode == 0 and '--augment' in r.stdout and '--augment_seed' in r.stdout
    a = build_parser().parse_args([])
    assert a.augment is False and a.augment_seed is None
    a = build_parser().parse_args(['--augment', '--augment_seed', '9'])
    assert a.augment is True and a.augment_seed == 9
    common = ['--scene', 'fire', '--model_folder', str(tmp_path / 'm'), '--input_folder', str(tmp_path), '--height', '64', '--width', '96',
              '--augment']
    (tmp_path / 'image_list.txt').write_text(str(tmp_path / 'a.png') + '\n')
    (tmp_path / 'transform.txt').write_text('1 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 0 1\n')
    r = _cli(*common)
    assert r.returncode == 1 and 'label_list.txt' in r.stderr
    (tmp_path / 'label_list.txt').write_text(str(tmp_path / 'a.bin') + '\n')
    np.zeros((8, 12, 4), np.float32).tofile(str(tmp_path / 'a.bin'))              # a grid-sized label
    r = _cli(*common)
    assert r.returncode == 1 and 'full-resolution' in r.stderr
    r = _cli(*(common[:-1] + ['--augment', '--height', '60']))
    assert r.returncode == 1 and 'multiples of 8' in r.stderr


def test_trainer_step_signature_takes_augment():
    import inspect
    from kfnet_amd.train import SCoordNetTrainer
    sig = inspect.signature(SCoordNetTrainer.step)
    assert list(sig.parameters) == ['self', 'frames_u8', 'labels', 'augment'] and sig.parameters['augment'].default is None
