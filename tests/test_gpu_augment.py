"""The training augmentation on the device (kfnet_amd/csrc/kfn_augment.hip): kfn_augment_batch equals the
float32 restatement of tests/augment_ref.py bit for bit -- frames and labels, every pixel -- kfn_frame_channel_sums equals
numpy's integer sums, and SCoordNetTrainer.step(..., augment=p) equals a trainer fed the restatement's frames and labels.
tests/test_augment_host.py ties the restatement to fp64 and to torch's grid_sample."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import augment_ref as R
from gpu_util import dev, stream, sync
from kfnet_amd import _lib
from kfnet_amd.augment import ENLARGE, SHRINK, TRANSLATE, AugmentParams, descriptor, draw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256
# (B, H, W): one grid pixel; ragged waves and several frames; one full-size frame
SHAPES = [(1, 8, 8), (3, 16, 24), (3, 40, 56), (3, 72, 104), (1, 480, 640)]
COLOUR = dict(delta=-13.25, factor=1.17)


def geometries(H):
    """The modes' cases; the last shrink ratio gives new_h = H - 1: an odd pad."""
    return [('translate', dict(mode=TRANSLATE, angle=12.0)),
            ('enlarge +30', dict(mode=ENLARGE, angle=30.0, x1=0.05, y1=0.11, ratio=0.84)),
            ('enlarge -30', dict(mode=ENLARGE, angle=-30.0, x1=0.17, y1=0.02, ratio=0.81)),
            ('enlarge 0', dict(mode=ENLARGE, angle=0.0, x1=0.13, y1=0.07, ratio=0.83)),
            ('enlarge box 0.2', dict(mode=ENLARGE, angle=8.0, x1=0.2, y1=0.2, ratio=0.8)),
            ('shrink 0.8', dict(mode=SHRINK, angle=-21.0, ratio=0.8)),
            ('shrink odd pad', dict(mode=SHRINK, angle=14.0, ratio=(H - 0.5) / H))]


def run_augment(frames, labels, params, label_stride):
    """kfn_augment_batch on fresh buffers with guard bytes behind both outputs; returns (frames, labels or None, sums)."""
    import torch
    lib = _lib.load()
    B, H, W, _ = frames.shape
    s = label_stride
    d = descriptor(params, B, H, W, s)
    fin = dev(frames)
    lin = None if labels is None else dev(labels)
    fout = torch.full((B * H * W * 3 + GUARD,), 77, dtype=torch.uint8, device='cuda')
    n_lab = B * (H // s) * (W // s) * 4
    lout = None if labels is None else torch.full((n_lab + GUARD,), -5.0, device='cuda')
    sums = torch.full((B * 4 + GUARD,), -1, dtype=torch.int32, device='cuda')
    _lib.check(lib.kfn_augment_batch(C.byref(d), fin.data_ptr(), None if lin is None else lin.data_ptr(), fout.data_ptr(),
                                     None if lout is None else lout.data_ptr(), sums.data_ptr(), stream()), 'kfn_augment_batch')
    sync()
    fh = fout.cpu().numpy()
    assert np.all(fh[-GUARD:] == 77), 'wrote past frames_out'
    sh = sums.cpu().numpy()
    assert np.all(sh[B * 4:] == -1), 'wrote past the sums'
    lh = None
    if lout is not None:
        lh = lout.cpu().numpy()
        assert np.all(lh[-GUARD:] == -5.0), 'wrote past labels_out'
        lh = lh[:n_lab].reshape(B, H // s, W // s, 4)
    assert np.array_equal(fin.cpu().numpy(), frames), 'the input frames changed'
    return fh[:-GUARD].reshape(B, H, W, 3), lh, sh[:B * 4].reshape(B, 4).view(np.uint32)


@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%dx%d' % s for s in SHAPES])
def test_augment_batch_equals_the_float32_restatement_bit_for_bit(shape):
    B, H, W = shape
    frames, labels = R.make_batch(B, H, W, 5)
    for name, geo in geometries(H):
        for colour in (False, True):
            p = AugmentParams(**dict(geo, **(COLOUR if colour else {})))
            if colour:       # the labels do not depend on the colour parameters: one restatement per geometry
                want_f, _ = R.augment32(frames, None, p)
            else:
                want_f, want_l = R.augment32(frames, labels, p, label_stride=1)
            got_f, got_l, sums = run_augment(frames, labels, p, 1)
            what = '%s, colour %s' % (name, colour)
            bad = int((got_f != want_f).sum())
            print('%dx%dx%d %s: %d frame bytes differ, %d label floats differ, %.1f %% of the frame is fill' %
                  (B, H, W, what, bad, int((got_l.view(np.uint32) != want_l.view(np.uint32)).sum()), 100 * float((want_f == 0).all(-1).mean())))
            assert np.array_equal(got_f, want_f), what
            assert np.array_equal(got_l.view(np.uint32), want_l.view(np.uint32)), what
            if colour:
                assert np.array_equal(sums, R.channel_sums(frames)), what
            # the label stride: the grid the loss reads equals the full-resolution output sub-sampled, and frames do not depend on labels
            grid_f, grid_l, _ = run_augment(frames, labels, p, 8)
            assert np.array_equal(grid_f, want_f) and np.array_equal(grid_l.view(np.uint32), want_l[:, ::8, ::8].view(np.uint32)), what
            if B > 1 or colour:
                only_f, none_l, _ = run_augment(frames, None, p, 8)
                assert none_l is None and np.array_equal(only_f, want_f), what
    # the cases do what their names say: rotated-in corners are fill, the identity case changes nothing
    f, l, _ = run_augment(frames, labels, AugmentParams(ENLARGE, 0.0, 0.0, 0.0, 1.0), 1)
    assert np.array_equal(f, frames) and np.array_equal(l[..., :3], labels[..., :3])
    if H >= 16:
        f, _, _ = run_augment(frames, None, AugmentParams(ENLARGE, 30.0, 0.0, 0.0, 1.0, **COLOUR), 8)
        assert not f[:, 0, 0].any() and not f[:, -1, -1].any() and f[:, H // 2, W // 2].any()


def test_channel_sums_are_exact():
    import torch
    lib = _lib.load()
    rng = np.random.default_rng(8)
    cases = [rng.integers(0, 256, size=(3, 8, 8, 3)).astype(np.uint8), rng.integers(0, 256, size=(2, 40, 56, 3)).astype(np.uint8),
             rng.integers(0, 256, size=(3, 72, 104, 3)).astype(np.uint8), np.full((1, 480, 640, 3), 255, np.uint8)]
    cases[2][1, :, :, 1] = 255          # channels apart: a phase slip between the three sums would show
    cases[2][1, :, :, 2] = 0
    for img in cases:
        B, H, W, _ = img.shape
        out = torch.full((B * 4 + 16,), -1, dtype=torch.int32, device='cuda')
        d = dev(img)
        _lib.check(lib.kfn_frame_channel_sums(d.data_ptr(), B, H, W, out.data_ptr(), stream()), 'kfn_frame_channel_sums')
        sync()
        got = out.cpu().numpy()
        assert np.all(got[B * 4:] == -1)
        assert np.array_equal(got[:B * 4].reshape(B, 4).view(np.uint32), R.channel_sums(img)), img.shape
    assert R.channel_sums(cases[3])[0, 0] == 480 * 640 * 255


def test_launches_are_identical_under_a_concurrent_copy_stream():
    import torch
    B, H, W = 4, 480, 640
    frames, labels = R.make_batch(B, H, W, 6)
    p = AugmentParams(ENLARGE, -23.0, 0.09, 0.14, 0.82, **COLOUR)
    lib = _lib.load()
    d = descriptor(p, B, H, W, 8)
    fin, lin = dev(frames), dev(labels)
    side = torch.cuda.Stream()
    big_a = torch.randn(32 << 20, device='cuda')
    big_b = torch.empty_like(big_a)
    outs = []
    for load in (False, True, True):
        fout = torch.zeros((B, H, W, 3), dtype=torch.uint8, device='cuda')
        lout = torch.zeros((B, H // 8, W // 8, 4), device='cuda')
        sums = torch.zeros((B, 4), dtype=torch.int32, device='cuda')
        torch.cuda.synchronize()
        if load:
            with torch.cuda.stream(side):
                for _ in range(4):
                    big_b.copy_(big_a)
        _lib.check(lib.kfn_augment_batch(C.byref(d), fin.data_ptr(), lin.data_ptr(), fout.data_ptr(), lout.data_ptr(), sums.data_ptr(),
                                         stream()), 'kfn_augment_batch')
        torch.cuda.synchronize()
        outs.append((fout, lout, sums))
    for fout, lout, sums in outs[1:]:
        assert torch.equal(fout, outs[0][0]) and torch.equal(lout, outs[0][1]) and torch.equal(sums, outs[0][2])
    assert np.array_equal(outs[0][2].cpu().numpy().view(np.uint32), R.channel_sums(frames))


def test_augmenter_wraps_the_call():
    from kfnet_amd.augment import Augmenter
    frames, labels = R.make_batch(2, 40, 56, 7)
    p = draw(3, 11)
    aug = Augmenter(2, 40, 56, label_stride=8)
    f, l = aug(frames, labels, p)
    want_f, want_l = R.augment32(frames, labels, p, label_stride=8)
    assert np.array_equal(f.cpu().numpy(), want_f) and np.array_equal(l.cpu().numpy().view(np.uint32), want_l.view(np.uint32))
    f, l = aug(dev(frames), None, p)
    assert l is None and np.array_equal(f.cpu().numpy(), want_f)
    with pytest.raises(ValueError):
        aug(frames, labels[:, ::8, ::8], p)
    with pytest.raises(ValueError):
        Augmenter(2, 40, 60)


# -- the trainer ---------------------------------------------------------------------------------------------------------------
SIZE = (64, 96)


def _training_inputs(count=4):
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    from kfnet_amd.train import synthetic_labels
    from kfnet_amd.weights import initial_weights
    return (synthetic_sequence(count, SIZE[0], SIZE[1]), synthetic_labels(count, SIZE), synthetic_transform().astype(np.float32),
            initial_weights(2))


def test_trainer_step_with_augment_equals_a_trainer_fed_the_restatement():
    from kfnet_amd.train import SCoordNetTrainer, StepStats
    frames, labels, M, W = _training_inputs()
    kw = dict(image_size=SIZE, batch=2, transform=M, base_lr=1e-3, stepvalue=3)
    a, b = SCoordNetTrainer(W, **kw), SCoordNetTrainer(W, **kw)
    params = [AugmentParams(ENLARGE, 19.0, 0.06, 0.12, 0.85, delta=9.5, factor=0.9), AugmentParams(SHRINK, -11.0, ratio=0.86, delta=-4.0, factor=1.1)]
    for s, p in enumerate(params):
        idx = [2 * s, 2 * s + 1]
        sa = dict(a.step(frames[idx], labels[idx], augment=p))
        want_f, want_l = R.augment32(frames[idx], labels[idx], p, label_stride=8)
        assert np.array_equal(a.frames.cpu().numpy(), want_f)
        sb = dict(b.step(want_f, want_l))
        print('step %d: %s' % (s, sa))
        assert sorted(sa) == sorted(StepStats.KEYS)
        for k in StepStats.KEYS:
            assert np.float64(sa[k]).tobytes() == np.float64(sb[k]).tobytes(), (s, k, sa[k], sb[k])
        assert 0 < sa['pixels'] < 2 * 8 * 12
    wa, wb = a.weights(), b.weights()
    for k in wa:
        assert np.array_equal(wa[k].view(np.uint32), wb[k].view(np.uint32)), k
        assert not np.array_equal(wa[k], W[k]), k
    with pytest.raises(ValueError):
        a.step(frames[:2], labels[:2, ::8, ::8], augment=params[0])       # grid-sized labels cannot be augmented
    assert a.global_step == 2


def test_trainer_step_without_augment_is_unchanged_after_an_augmented_one():
    """step(frames, labels) gives the same bits whether or not the trainer has augmented a batch before: the augmentation
    leaves nothing behind that the plain path reads."""
    from kfnet_amd.train import SCoordNetTrainer
    frames, labels, M, W = _training_inputs()
    kw = dict(image_size=SIZE, batch=2, transform=M, base_lr=1e-3, stepvalue=3)
    plain, mixed = SCoordNetTrainer(W, **kw), SCoordNetTrainer(W, **kw)
    mixed.step(frames[:2], labels[:2], augment=draw(1, 0))
    mixed.set_weights(W)
    mixed.load_state(plain.state())
    for lab in (labels[2:4], labels[2:4, ::8, ::8]):
        sp, sm = dict(plain.step(frames[2:4], lab)), dict(mixed.step(frames[2:4], lab))
        assert sp == sm
    wp, wm = plain.weights(), mixed.weights()
    for k in wp:
        assert np.array_equal(wp[k].view(np.uint32), wm[k].view(np.uint32)), k


def _cli(args, timeout=900):
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT'):
        env.pop(k, None)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    r = subprocess.run([sys.executable, '-m', 'kfnet_amd.SCoordNet.train'] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_augmented_command_line_run_resumes_to_the_same_snapshot_bytes(tmp_path):
    """--augment --synthetic: 6 steps in one run, and 3 steps + a resumed run of 3 more, write snapshots whose every array has the same
    bytes: the draws are a function of (seed, step).  A run without --augment writes other weights."""
    common = ['--synthetic', '6', '--height', '64', '--width', '96', '--batch', '2', '--scene', 'fire', '--snapshot', '3', '--display', '3',
              '--stepvalue', '4', '--base_lr', '1e-3']
    one, two, plain = tmp_path / 'one', tmp_path / 'two', tmp_path / 'plain'
    _cli(['--model_folder', str(one), '--max_steps', '6', '--augment', '--augment_seed', '5'] + common)
    _cli(['--model_folder', str(two), '--max_steps', '3', '--augment', '--augment_seed', '5'] + common)
    log = _cli(['--model_folder', str(two), '--max_steps', '6', '--augment', '--augment_seed', '5'] + common)
    assert 'current step:  3' in log and 'Adam slots restored' in log and 'step 6/6' in log
    _cli(['--model_folder', str(plain), '--max_steps', '6'] + common)
    def content(path):
        # every array's name, dtype, shape and bytes (the .npz container itself carries the time of writing)
        with np.load(str(path)) as z:
            return {k: (z[k].dtype.str, z[k].shape, z[k].tobytes()) for k in z.files}
    for name in ('kfnet_weights-6.npz', 'kfnet_train_state-6.npz', 'kfnet_weights-3.npz'):
        assert content(one / name) == content(two / name), name
    assert content(one / 'kfnet_weights-6.npz') != content(plain / 'kfnet_weights-6.npz')
