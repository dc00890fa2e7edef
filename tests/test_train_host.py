"""CPU tests of the training path (kfnet_amd/train.py, kfnet_amd/batches.py, kfnet_amd/SCoordNet/train.py; DESIGN.md
"Training"): schedules, label preparation, snapshot naming, initial weights, the new exports' argument checks, the command
line's refusals, the batch sources, and the reference loss of tests/train_ref.py against finite differences."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import train_ref as R
from kfnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kfn_conv2d_grad_weights_workspace_bytes', 'kfn_conv2d_grad_weights', 'kfn_first_conv_u8_grad_weights_workspace_bytes',
       'kfn_first_conv_u8_grad_weights', 'kfn_relu_grad', 'kfn_pack_conv_weights_floats', 'kfn_pack_conv_weights',
       'kfn_coord_loss_grad', 'kfn_adam_step')


def test_learning_rate_is_exponential_decay_with_a_real_exponent():
    from kfnet_amd.train import adam_lr_t, learning_rate
    assert learning_rate(1e-4, 0.5, 80000, 0) == 1e-4
    assert learning_rate(1e-4, 0.5, 80000, 80000) == pytest.approx(5e-5, rel=1e-15)
    assert learning_rate(1e-4, 0.5, 80000, 40000) == pytest.approx(1e-4 * np.sqrt(0.5), rel=1e-15)   # no staircase
    assert learning_rate(1e-4, 0.5, 30000, 1) < 1e-4
    assert adam_lr_t(1e-4, 1) == pytest.approx(1e-4 * np.sqrt(0.001) / 0.1, rel=1e-12)
    assert adam_lr_t(1e-4, 10 ** 6) == pytest.approx(1e-4, rel=1e-9)


def test_batches_are_consecutive_and_wrap_and_shuffle_is_a_seeded_permutation_per_epoch():
    from kfnet_amd.train import batch_indices
    assert batch_indices(0, 4, 10) == [0, 1, 2, 3]
    assert batch_indices(2, 4, 10) == [8, 9, 0, 1]
    assert batch_indices(5, 4, 10) == [0, 1, 2, 3]
    stream = [i for s in range(10) for i in batch_indices(s, 3, 10, shuffle=True, seed=5)]
    for e in range(3):
        assert sorted(stream[10 * e:10 * e + 10]) == list(range(10))      # every epoch visits every frame once
    assert stream[:10] != list(range(10)) and stream[:10] != stream[10:20]
    assert stream == [i for s in range(10) for i in batch_indices(s, 3, 10, shuffle=True, seed=5)]
    assert stream != [i for s in range(10) for i in batch_indices(s, 3, 10, shuffle=True, seed=6)]


def test_labels_are_down_sampled_like_the_metrics_oracle():
    """The loss kernel reads cell (r, c) of a full-resolution label at pixel (8r, 8c); the reference of the GPU tests
    (train_ref.grid_labels) and the command line's reader (KFNet.metrics.read_label_grid) must mean the same cells."""
    from kfnet_amd.KFNet.metrics import read_label_grid
    from kfnet_amd.train import synthetic_labels
    from oracle import kfnet_metrics_oracle as MO
    rng = np.random.default_rng(0)
    lab = rng.normal(size=(2, 64, 96, 4)).astype(np.float32)
    got = R.grid_labels(lab, (8, 12))
    for i in range(2):
        np.testing.assert_array_equal(got[i], MO.resize_nearest(lab[i], (8, 12)))
    np.testing.assert_array_equal(R.grid_labels(got, (8, 12)), got)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'label.bin')
        lab[0].tofile(path)
        np.testing.assert_array_equal(read_label_grid(path, (64, 96), (8, 12)), got[0])
    s = synthetic_labels(3, (8, 12))
    assert s.shape == (3, 8, 12, 4) and s.dtype == np.float32
    assert set(np.unique(s[..., 3])) == {0.0, 1.0} and 0.5 < s[..., 3].mean() < 1.0
    np.testing.assert_array_equal(s[1:], synthetic_labels(2, (8, 12), start=1))


def test_snapshot_names_and_get_snapshot_ignores_the_state_file(tmp_path):
    from kfnet_amd.tools.io import get_snapshot
    from kfnet_amd.train import restore, snapshot_paths
    from kfnet_amd.weights import initial_weights, save_npz
    wp, sp = snapshot_paths(str(tmp_path), 7)
    assert os.path.basename(wp) == 'kfnet_weights-7.npz' and os.path.basename(sp) == 'kfnet_train_state-7.npz'
    W = initial_weights(1)
    save_npz(wp, W)
    np.savez(snapshot_paths(str(tmp_path), 9)[1], global_step=np.int64(9))      # a state file with a HIGHER step
    assert get_snapshot(str(tmp_path)) == (wp, 7)
    got, state, step = restore(str(tmp_path), verbose=False)
    assert step == 7 and state is None and sorted(got) == sorted(W)
    np.savez(sp, global_step=np.int64(7), adam_t=np.int64(7))
    assert restore(str(tmp_path), verbose=False)[1]['adam_t'] == 7
    assert restore(str(tmp_path / 'none'), verbose=False) == (None, None, 0)


def test_initial_weights_are_glorot_uniform_with_zero_biases():
    from kfnet_amd.weights import initial_weights, synthetic_weights, variable_specs
    W = initial_weights(3)
    assert all(k.startswith('ScoreNet/') for k in W) and len(W) == 24
    for name, kind, shape in variable_specs():
        if not name.startswith('ScoreNet/'):
            continue
        k = W[name + '/kernel']
        lim = np.sqrt(6.0 / (shape[0] * shape[1] * (shape[2] + shape[3])))
        assert k.shape == shape and k.dtype == np.float32
        assert np.abs(k).max() <= lim and np.abs(k).max() > 0.8 * lim          # no head scaling: 'prediction' too
        assert not W[name + '/bias'].any()
    np.testing.assert_array_equal(W['ScoreNet/conv3a/kernel'], initial_weights(3)['ScoreNet/conv3a/kernel'])
    assert not np.array_equal(W['ScoreNet/conv3a/kernel'], initial_weights(4)['ScoreNet/conv3a/kernel'])
    assert len(initial_weights(3, scopes=('ScoreNet', 'Temporal'))) == len(synthetic_weights(1))


def test_new_entry_points_are_exported_and_check_their_arguments_without_a_device():
    lib = _lib.load()
    assert lib.kfn_abi_version() == 13
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    ARG = -1
    buf = np.zeros(64, np.float32).ctypes.data
    nb = C.c_size_t()

    def desc(**kw):
        d = dict(N=1, H=9, W=13, Cin=16, ldx=16, Cout=4, cout_pad=32, ldy=4, kh=3, kw=3, stride=1)
        d.update(kw)
        return _lib.ConvDesc(**d)
    d = desc()
    assert lib.kfn_conv2d_grad_weights_workspace_bytes(C.byref(d), C.byref(nb)) == 0 and nb.value >= (9 * 16 + 1) * 4 * 4
    for bad in (dict(Cin=8, ldx=8), dict(kh=5, kw=5), dict(stride=3), dict(transposed=1, stride=2), dict(ldy=2), dict(N=0),
                dict(operand_dtype=1)):
        d = desc(**bad)
        assert lib.kfn_conv2d_grad_weights_workspace_bytes(C.byref(d), C.byref(nb)) == ARG, bad
        assert lib.kfn_conv2d_grad_weights(C.byref(d), buf, buf, buf, buf, buf, None) == ARG, bad
        assert b'kfn_conv2d_grad_weights' in lib.kfn_last_error()
    d = desc()
    assert lib.kfn_conv2d_grad_weights(C.byref(d), None, buf, buf, buf, buf, None) == ARG
    assert lib.kfn_first_conv_u8_grad_weights_workspace_bytes(1, 8, 8, 64, C.byref(nb)) == 0 and nb.value == 28 * 64 * 4
    assert lib.kfn_first_conv_u8_grad_weights_workspace_bytes(1, 8, 8, 24, C.byref(nb)) == ARG
    assert lib.kfn_first_conv_u8_grad_weights(buf, 1, 8, 8, buf, 128, buf, buf, buf, None) == ARG
    assert lib.kfn_first_conv_u8_grad_weights(None, 1, 8, 8, buf, 64, buf, buf, buf, None) == ARG
    assert lib.kfn_relu_grad(buf, 4, buf, 2, 10, 4, None) == ARG
    assert lib.kfn_relu_grad(buf, 4, None, 4, 10, 4, None) == ARG
    n = C.c_size_t()
    assert lib.kfn_pack_conv_weights_floats(1, 1, 128, 4, _lib.PACK_FORWARD, C.byref(n)) == 0 and n.value == 32 * 128
    assert lib.kfn_pack_conv_weights_floats(1, 1, 128, 4, _lib.PACK_INPUT_GRAD_S1, C.byref(n)) == 0 and n.value == 128 * 16
    assert lib.kfn_pack_conv_weights_floats(3, 3, 64, 256, _lib.PACK_INPUT_GRAD_S2, C.byref(n)) == 0 and n.value == 64 * 9 * 256
    assert lib.kfn_pack_conv_weights_floats(3, 3, 64, 256, 7, C.byref(n)) == ARG
    assert lib.kfn_pack_conv_weights(buf, 3, 3, 0, 4, 0, buf, None) == ARG
    ld = _lib.CoordLossDesc(B=1, h=2, w=2, ld_pred=4, ld_dpred=4, label_stride=1, img_stride=8, smooth_weight=50.0,
                            dist_threshold=0.05, min_uncertainty=1e-5)
    assert lib.kfn_coord_loss_grad(C.byref(ld), buf, buf, None, buf, buf, None) == ARG         # smoothness without frames
    assert b'frames' in lib.kfn_last_error()
    ld.smooth_weight = 0.0
    ld.ld_dpred = 3
    assert lib.kfn_coord_loss_grad(C.byref(ld), buf, buf, None, buf, buf, None) == ARG
    ld.ld_dpred, ld.struct_size = 4, 8
    assert lib.kfn_coord_loss_grad(C.byref(ld), buf, buf, None, buf, buf, None) == ARG
    assert lib.kfn_adam_step(buf, buf, buf, buf, 0, 1e-4, 0.9, 0.999, 1e-8, 0.0, None) == ARG
    assert lib.kfn_adam_step(buf, buf, buf, buf, 8, 1e-4, 1.0, 0.999, 1e-8, 0.0, None) == ARG
    assert lib.kfn_adam_step(buf, None, buf, buf, 8, 1e-4, 0.9, 0.999, 1e-8, 0.0, None) == ARG


def _cli(*args):
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    return subprocess.run([sys.executable, '-m', 'kfnet_amd.SCoordNet.train'] + list(args), cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def test_command_line_help_schedule_and_refusals(tmp_path):
    from kfnet_amd.SCoordNet.train import build_parser, format_line, schedule
    r = _cli('--help')
    assert r.returncode == 0
    for flag in ('--input_folder', '--model_folder', '--scene', '--base_lr', '--max_steps', '--display', '--stepvalue',
                 '--snapshot', '--gamma', '--weight_decay', '--shuffle', '--reset_step', '--gpu', '--batch', '--height',
                 '--width', '--seed', '--loss_clip', '--smooth_weight', '--synthetic'):
        assert flag in r.stdout, flag
    a = build_parser().parse_args([])
    assert (a.base_lr, a.display, a.snapshot, a.gamma, a.weight_decay, a.batch, a.loss_clip, a.smooth_weight) == \
        (1e-4, 10, 5000, 0.5, 1e-4, 4, None, 50.0)
    assert schedule('fire') == (30000, 150000) and schedule('heads') == (60000, 300000) and schedule('chess') == (100000, 500000)
    assert schedule('fire', stepvalue=10) == (10, 50) and schedule('fire', max_steps=3) == (30000, 3)
    line = format_line('now', 1, 20, 100, dict(loss=1.5, l_measure=1.25, l_smooth=0.005, a_measure=0.5, pixels=95.0, lr=1e-4), 0.25)
    assert line == ('[now] epoch 1, step 20/100, loss=1.500, l_measure=1.250, l_smooth=0.005, a_measure=0.500, #pixels=95, '
                    'lr = 0.000100 (0.250 sec/step)')
    r = _cli('--scene', 'nowhere', '--model_folder', str(tmp_path))
    assert r.returncode == 1 and 'Invalid scene' in r.stdout
    r = _cli('--scene', 'fire')
    assert r.returncode == 1 and '--model_folder' in r.stderr
    r = _cli('--scene', 'fire', '--model_folder', str(tmp_path), '--synthetic', '4', '--height', '60')
    assert r.returncode == 1 and 'multiples of 8' in r.stderr
    r = _cli('--scene', 'fire', '--model_folder', str(tmp_path), '--input_folder', str(tmp_path / 'missing'))
    assert r.returncode == 1 and 'image_list.txt' in r.stderr
    (tmp_path / 'image_list.txt').write_text('a.png\n')
    r = _cli('--scene', 'fire', '--model_folder', str(tmp_path), '--input_folder', str(tmp_path))
    assert r.returncode == 1 and 'label_list.txt' in r.stderr


def test_trainer_refuses_sizes_that_are_not_multiples_of_8():
    from kfnet_amd.train import SCoordNetTrainer
    with pytest.raises(ValueError):
        SCoordNetTrainer({}, image_size=(60, 96))


def test_reference_loss_gradient_matches_finite_differences():
    import torch
    rng = np.random.default_rng(2)
    B, h, w = 2, 5, 6
    pred0 = rng.normal(size=(B, h, w, 4))
    pred0[..., 3] = rng.uniform(-1.5, 0.5, size=(B, h, w))
    labels = rng.normal(size=(B, h, w, 4)).astype(np.float32)
    labels[..., 3] = (rng.uniform(size=(B, h, w)) < 0.8).astype(np.float32)
    labels[0, 0, 0, 3] = 0.5                                        # mask == 1.0 exactly, nothing else counts
    img = rng.integers(0, 256, size=(B, h, w, 3)).astype(np.float64)
    img[:, :, 3:] = img[:, :, 3:4]                                  # flat regions: weights near 1
    M = np.eye(4)
    M[:3, :3] += 0.1 * rng.normal(size=(3, 3))
    M[:3, 3] = rng.normal(size=3)
    for clip in (None, 0.5):
        def f(p):
            return R.coord_loss(torch.from_numpy(p), labels, img, M, clip, 50.0)[0]
        p = torch.from_numpy(pred0.copy()).requires_grad_(True)
        L, nll, sm, acc, valid = R.coord_loss(p, labels, img, M, clip, 50.0)
        g, = torch.autograd.grad(L, [p])
        g = g.numpy()
        assert valid.item() == float((labels[..., 3] == 1.0).sum() + 1) and sm.item() > 0 and 0.0 <= acc.item() <= 1.0
        assert L.item() == pytest.approx(nll.item() + 50.0 * sm.item(), rel=1e-14)
        eps = 1e-6
        for idx in [(0, 0, 0, 0), (0, 2, 3, 1), (1, 4, 5, 2), (1, 1, 1, 3), (0, 4, 0, 3), (1, 0, 5, 0), (0, 3, 3, 3)]:
            hi, lo = pred0.copy(), pred0.copy()
            hi[idx] += eps
            lo[idx] -= eps
            fd = (float(f(hi)) - float(f(lo))) / (2 * eps)
            assert g[idx] == pytest.approx(fd, rel=1e-5, abs=1e-8), (clip, idx)
        assert np.all(g[labels[..., 3] != 1.0][:, 3] == 0.0)        # masked pixels: no NLL gradient
    # the clip is active somewhere and inactive elsewhere
    p = torch.from_numpy(pred0)
    sig = np.exp(pred0[..., 3:4])
    l = 3 * np.log(sig) + ((pred0[..., :3] - (labels[..., :3].astype(np.float64) @ M[:3, :3].T + M[:3, 3])) ** 2).sum(-1, keepdims=True) / (2 * sig * sig)
    assert (l > 0.5).any() and (l < 0.5).any()


def test_reference_adam_is_the_tensorflow_formula():
    w = np.array([0.5, -0.25, 0.0], np.float32)
    g = np.array([0.1, -0.2, 0.3], np.float32)
    m = np.zeros(3, np.float32)
    v = np.zeros(3, np.float32)
    w1, m1, v1 = R.adam_step(w, m, v, g, 1e-3, 1)
    np.testing.assert_allclose(m1, 0.1 * g, rtol=1e-6)
    np.testing.assert_allclose(v1, 0.001 * g * g, rtol=1e-6)
    np.testing.assert_allclose(w - w1, 1e-3 * np.sign(g), rtol=1e-4)          # the first Adam step is lr * sign(g)
    w2, _, _ = R.adam_step(w, m, v, g * 0, 1e-3, 1, weight_decay=0.5)
    np.testing.assert_allclose(w - w2, 1e-3 * np.sign(w), rtol=1e-4, atol=1e-12)   # the regulariser's gradient is wd * w


def test_inputs_of_the_gpu_loss_tests_keep_clear_of_the_squared_threshold():
    """With numpy alone: every grid tests/test_gpu_train.py runs the loss on beyond one pass satisfies its input condition -- no
    masked pixel whose squared distance lies within 1e-6 of float32(0.05 * 0.05) -- and the clip construction fills both
    branches at the production batch.  The frames carry smoothness weights in both directions (_flatten_upper_half), and the
    seam case has weights of 1 across every frame seam (_seam_inputs asserts what a cross-seam read would add)."""
    import numpy as np
    import test_gpu_train as G
    assert np.float32(G.THR2).view(np.uint32) == 0x3B23D70A
    for grid in G.LOSS_GRIDS:
        pred, labels, frames, M = G._grid_inputs(grid)
        assert pred.shape == grid + (4,) and frames.shape[1:3] == (8 * grid[1], 8 * grid[2])
    assert max(g[0] * g[1] * g[2] for g in G.LOSS_GRIDS) == 19200 and min(g[0] * g[1] * g[2] for g in G.LOSS_GRIDS) == 1024
    G._grid_inputs((4, 60, 80), full_res=True)
    assert G._seam_inputs()[4] > 0
    G._clip_inputs(3)
    G._clip_inputs(7, flat=True, B=4, h=60, w=80)


def test_batch_sources_return_the_frames_and_labels_of_the_indices(tmp_path):
    """The three sources of kfnet_amd.batches have one shape; the synthetic one and the one over label files run without a
    device.  Indices of steps 0-2 at batch 2 of 5 frames: the third batch wraps."""
    from types import SimpleNamespace
    from PIL import Image
    from kfnet_amd.batches import LabelFileSource, SyntheticSource, open_source
    from kfnet_amd.KFNet.metrics import read_label_grid
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    from kfnet_amd.train import batch_indices, synthetic_labels
    H, W, count = 64, 96, 5
    batches = [batch_indices(s, 2, count) for s in range(3)]
    assert batches[2] == [4, 0]
    frames = synthetic_sequence(count, H, W)
    args = SimpleNamespace(height=H, width=W, synthetic=count, depth=False, input_folder=str(tmp_path), batch=2, gpu=0)
    src = open_source(args, False)
    assert isinstance(src, SyntheticSource) and src.count == count
    np.testing.assert_array_equal(src.transform, synthetic_transform())
    for full, hw in ((False, (8, 12)), (True, (H, W))):
        for idx in batches:
            f, l = src.batch(idx, full)
            assert f.dtype == np.uint8 and l.dtype == np.float32
            np.testing.assert_array_equal(f, frames[idx])
            np.testing.assert_array_equal(l, synthetic_labels(count, hw)[idx])

    rng = np.random.default_rng(4)
    labels = rng.normal(size=(count, H, W, 4)).astype(np.float32)
    M = rng.normal(size=(4, 4)).astype(np.float32)
    images, label_files = [], []
    for i in range(count):
        images.append(str(tmp_path / ('image_%d.png' % i)))
        label_files.append(str(tmp_path / ('label_%d.bin' % i)))
        Image.fromarray(frames[i]).save(images[i])
        labels[i].tofile(label_files[i])
    (tmp_path / 'image_list.txt').write_text(''.join(p + '\n' for p in images))
    (tmp_path / 'label_list.txt').write_text(''.join(p + '\n' for p in label_files))
    np.savetxt(str(tmp_path / 'transform.txt'), M)
    args.synthetic = 0
    for full in (False, True):
        src = open_source(args, full)
        assert isinstance(src, LabelFileSource) and src.count == count
        np.testing.assert_array_equal(src.transform, np.loadtxt(str(tmp_path / 'transform.txt'), dtype=np.float32))
        for idx in batches:
            f, l = src.batch(idx, full)
            assert f.dtype == np.uint8 and l.dtype == np.float32
            np.testing.assert_array_equal(f, frames[idx])
            want = np.stack([labels[i] if full else read_label_grid(label_files[i], (H, W), (8, 12)) for i in idx])
            assert l.shape == want.shape and l.tobytes() == want.tobytes()

    labels[0, :8].tofile(label_files[0])                     # a label file of the wrong size, first in the list
    with pytest.raises(ValueError, match='label_0.bin'):
        open_source(args, True)
    src = open_source(args, False)                           # grid-sized reads open only the files of a batch
    for full in (False, True):
        with pytest.raises(ValueError, match='label_0.bin'):
            src.batch(batches[2], full)
        assert src.batch(batches[1], full)[1].shape[0] == 2
    args.depth, args.synthetic = True, count
    with pytest.raises(ValueError, match='--synthetic'):
        open_source(args, False)
