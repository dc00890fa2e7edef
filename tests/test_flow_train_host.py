"""Host side of training OFlowNet (stage 2): the reference of the GPU tests (tests/flow_train_ref.py) against the
oracle's forward and in hand cases of the loss, the sequential-add restatement of the cost volume's transpose against
autograd, the pair list, the loss descriptor, and the new exports."""
import ctypes as C
import os
import re

import numpy as np
import torch

import flow_train_ref as FR
from kfnet_amd import _lib
from kfnet_amd.train_kfnet import group_indices, group_list
from kfnet_amd.weights import synthetic_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kfn_cost_volume_backward', 'kfn_flow_head_backward', 'kfn_l2norm_backward', 'kfn_flow_loss_grad')


# -- the reference -------------------------------------------------------------------------------------------------------------
def test_reference_forward_equals_the_oracle_bit_for_bit_on_a_16x24_pair():
    from oracle.kfnet_oracle_torch import coord_volume, oflow_feat, oflownet, process_model
    rng = np.random.default_rng(0)
    Wnp = synthetic_weights(seed=7)
    frames = rng.integers(0, 256, size=(2, 16, 24, 3)).astype(np.uint8)
    W = FR.tensors(Wnp, torch.float32)
    with torch.no_grad():
        f = FR.l2_normalize(FR.tower(frames, W))
        assert np.array_equal(f.numpy(), oflow_feat(frames, Wnp))
        vol = FR.coord_volume(f[0:1], f[1:2])
        want_vol, offs = coord_volume(f[0:1].numpy(), f[1:2].numpy())
        assert vol.shape == (6, 8, 8, 32) and np.array_equal(vol.numpy(), want_vol)
        assert np.array_equal(offs, FR.OFFSETS.astype(np.float32))
        prob, flow, st = FR.flow_head(*FR.unet(vol, W))
        want_prob, want_st = oflownet(want_vol, Wnp)
        assert np.array_equal(prob.numpy(), want_prob) and np.array_equal(st.numpy(), want_st.reshape(-1))
        last = rng.normal(size=(1, 2, 3, 3)).astype(np.float32)
        tx, ts, want_flow = process_model(want_prob, want_st, offs, last, np.zeros((1, 2, 3, 1), np.float32))
        assert np.array_equal(flow.numpy().reshape(1, 2, 3, 2), want_flow)
        # the process model on a certain last frame IS the loss's warp and uncertainty
        xm, _, _ = FR.warp_labels(flow.reshape(1, 2, 3, 2), np.concatenate([last, np.ones((1, 2, 3, 1), np.float32)], -1).repeat(2, 0))
        assert np.array_equal(xm.numpy(), tx)
        eps2 = torch.tensor(FR.EPS2)
        sm = torch.sqrt(eps2 + torch.maximum(st * st, eps2))
        assert np.array_equal(sm.numpy().reshape(1, 2, 3, 1), ts)
        p2, f2, s2 = FR.forward(frames, W)
        assert np.array_equal(f2.numpy().reshape(-1, 2), flow.numpy()) and np.array_equal(s2.numpy().reshape(-1), st.numpy())


def _labels(rng, P, h, w):
    lab = rng.normal(size=(2 * P, h, w, 4))
    lab[..., 3] = 1.0
    return lab


def test_loss_hand_cases_zero_flow_a_masked_corner_and_a_flow_that_leaves_the_grid():
    rng = np.random.default_rng(1)
    P, h, w = 1, 5, 7
    lab = _labels(rng, P, h, w)
    zero = torch.zeros((P, h, w, 2), dtype=torch.float64)
    xm, va, mb = FR.warp_labels(zero, lab)
    # the corner (x + 1, y + 1) of the last row and column lies outside: those cells are not valid, the others read label a
    assert np.array_equal(va.numpy()[0], np.pad(np.ones((h - 1, w - 1)), ((0, 1), (0, 1))))
    assert np.array_equal(xm.numpy()[0, :-1, :-1], lab[0, :-1, :-1, 0:3]) and mb.min() == 1
    st = torch.full((P, h, w), 0.01, dtype=torch.float64)
    L, acc, valid, lost = FR.flow_loss(zero, st, lab)
    assert valid.item() == (h - 1) * (w - 1) + 1 and lost.item() == h + w - 1
    u = np.sqrt(FR.EPS2 + 1e-4)
    d = ((lab[0, :-1, :-1, 0:3] - lab[1, :-1, :-1, 0:3]) ** 2).sum(-1)
    assert abs(L.item() - (3 * np.log(u) + d / (2 * u * u)).sum() / valid.item()) <= 1e-9 * abs(L.item())
    # a corner with m_a = 0 zeroes the four cells that read it; m_b = 0 zeroes its own
    lab2 = lab.copy()
    lab2[0, 2, 3, 3] = 0.0
    lab2[1, 0, 0, 3] = 2.0                        # only mask == 1 counts
    _, va2, mb2 = FR.warp_labels(zero, lab2)
    gone = np.argwhere(va.numpy()[0] - va2.numpy()[0])
    assert sorted(map(tuple, gone)) == [(1, 2), (1, 3), (2, 2), (2, 3)] and mb2[0, 0, 0] == 0 and mb2.sum() == h * w - 1
    assert FR.flow_loss(zero, st, lab2)[2].item() == valid.item() - 5
    # a flow that leaves the grid: (1, 1) + (-1.5, 0) has floor(px) = -1
    out = zero.clone()
    out[0, 1, 1] = torch.tensor([-1.5, 0.0])
    out[0, 2, 2] = torch.tensor([0.0, 2.25])      # (2, 2 + 2.25): floor 4, corner 5 = h is outside
    out[0, 0, 0] = torch.tensor([0.5, 0.5])       # stays inside
    _, va3, _ = FR.warp_labels(out, lab)
    assert sorted(map(tuple, np.argwhere(va.numpy()[0] - va3.numpy()[0]))) == [(1, 1), (2, 2)]
    # an all-masked batch: L = 0 and no gradient
    lab0 = lab.copy()
    lab0[1::2, ..., 3] = 0.0
    stats, gf, gs = FR.loss_grads(rng.uniform(-1, 1, size=(P, h, w, 2)), np.full((P, h, w), 0.01), lab0)
    assert stats[0] == 0.0 and stats[2] == 1.0 and not gf.any() and not gs.any()


def test_loss_gradient_formulas_of_the_issue_match_autograd():
    rng = np.random.default_rng(2)
    P, h, w = 2, 5, 7
    lab = _labels(rng, P, h, w)
    lab[..., 3] = rng.uniform(size=(2 * P, h, w)) < 0.9
    flow = rng.uniform(-1.5, 1.5, size=(P, h, w, 2))
    st = 10.0 ** rng.uniform(-6, -1, size=(P, h, w))          # below and above the variance floor
    stats, gf, gs = FR.loss_grads(flow, st, lab)
    xm, va, mb = FR.warp_labels(torch.from_numpy(flow), lab)
    M = (va * mb).numpy()
    sm = np.sqrt(FR.EPS2 + np.maximum(st * st, FR.EPS2))
    u = np.maximum(sm, 1e-5)
    d = ((xm.numpy() - lab[1::2, ..., 0:3]) ** 2).sum(-1)
    want = M / stats[2] * (3 / u - d / u ** 3) * (sm > 1e-5) * (st * st > FR.EPS2) * st / sm
    assert np.abs(gs - want).max() <= 1e-12 * np.abs(want).max() and (st * st <= FR.EPS2).any() and M.sum() > 20
    # d_flow against finite differences, with a process noise of centimetres: under the floor 1 / u^2 = 5e9 leaves them no digits
    eps = 1e-6
    st = rng.uniform(0.05, 0.2, size=(P, h, w))
    gf = FR.loss_grads(flow, st, lab)[1]
    tl = torch.from_numpy(st)
    for idx in [(0, 1, 2, 0), (0, 2, 3, 1), (1, 3, 4, 0), (1, 1, 1, 1)]:
        assert M[idx[:3]] == 1 and abs(flow[idx] - np.round(flow[idx])) > 1e-3
        hi, lo = flow.copy(), flow.copy()
        hi[idx] += eps
        lo[idx] -= eps
        fd = (FR.flow_loss(torch.from_numpy(hi), tl, lab)[0].item() - FR.flow_loss(torch.from_numpy(lo), tl, lab)[0].item()) / (2 * eps)
        assert abs(fd - gf[idx]) <= 1e-5 * max(1.0, abs(fd)), (idx, fd, gf[idx])


def test_sequential_cost_volume_transpose_equals_autograd_exactly_on_integers():
    rng = np.random.default_rng(3)
    for (P, h, w, Cc) in ((1, 2, 3, 4), (2, 5, 7, 8), (1, 9, 13, 4)):
        d_vol = rng.integers(-8, 9, size=(P * h * w, 8, 8, Cc)).astype(np.float64)
        fa = torch.zeros((P, h, w, Cc), dtype=torch.float64, requires_grad=True)
        fb = torch.zeros((P, h, w, Cc), dtype=torch.float64, requires_grad=True)
        ga, gb = torch.autograd.grad((FR.coord_volume(fa, fb) * torch.from_numpy(d_vol)).sum(), [fa, fb])
        d_f2, d_f1 = FR.cost_volume_backward(d_vol, (P, h, w))
        assert d_f2.dtype == np.float32 and np.array_equal(d_f2, gb.numpy()) and np.array_equal(d_f1, ga.numpy())


# -- pairs ---------------------------------------------------------------------------------------------------------------------
def test_pair_list_and_its_wrapping_stream():
    g = group_list(4, 1000, group=2)
    assert g == [[0, 1], [1, 0], [1, 2], [2, 1], [2, 3], [3, 2]]
    g = group_list(6, 3, group=2)                 # never across a range of sequence_length frames
    assert g == [[0, 1], [1, 0], [1, 2], [2, 1], [3, 4], [4, 3], [4, 5], [5, 4]]
    assert group_list(1, 1000, group=2) == [] and len(group_list(2000, 1000, group=2)) == 2 * 2 * 999
    assert group_indices(0, 2, g) == [0, 1, 1, 0] and group_indices(3, 2, g) == [4, 5, 5, 4]
    assert group_indices(1, 3, g) == [2, 1, 3, 4, 4, 3] and group_indices(2, 3, g) == [4, 5, 5, 4, 0, 1]
    a = [group_indices(s, 2, g, True, 5) for s in range(8)]
    assert a == [group_indices(s, 2, g, True, 5) for s in reversed(range(8))][::-1]
    assert sorted(tuple(x[i:i + 2]) for x in a[0:4] for i in (0, 2)) == sorted(map(tuple, g))


# -- exports -------------------------------------------------------------------------------------------------------------------
def test_loss_descriptor_matches_the_header_and_its_constants_round_once():
    header = open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()
    body = re.search(r'typedef struct kfn_flow_loss_desc \{(.*?)\} kfn_flow_loss_desc;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [f.strip() for decl in re.findall(r'(?:int32_t|float|double)\s+([^;]+);', body) for f in decl.split(',')]
    assert fields == [f[0] for f in _lib.FlowLossDesc._fields_]
    d = _lib.FlowLossDesc(P=1, h=2, w=3, label_stride=8, dist_threshold=0.05, min_uncertainty=1e-5)
    assert d.struct_size == C.sizeof(_lib.FlowLossDesc) == 48 and _lib.FlowLossDesc.dist_threshold.offset == 32
    # what the library makes of the doubles: one rounding of the double product
    assert np.float32(d.dist_threshold * d.dist_threshold).view(np.uint32) == FR.THR2_BITS == 0x3B23D70A
    assert np.float32(d.min_uncertainty * d.min_uncertainty) == np.float32(FR.EPS2)
    assert np.float32(FR.EPS2).view(np.uint32) != (np.float32(1e-5) * np.float32(1e-5)).view(np.uint32)


def test_new_exports_are_declared_bound_and_check_their_arguments_without_a_device():
    header = open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()
    lib = _lib.load()
    assert lib.kfn_abi_version() == 13 and '#define KFN_ABI_VERSION 13' in header
    for name in NEW:
        assert re.search(r'\bint %s\(' % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert 'ascending' in re.search(r'kfn_cost_volume_backward --(.*?)\*/', header, re.S).group(1)
    ARG = -1
    buf = np.zeros(256, np.float32)
    b = buf.ctypes.data + (-buf.ctypes.data) % 16
    assert lib.kfn_cost_volume_backward(b, b, b, 1, 2, 3, 6, None) == ARG and b'C=6' in lib.kfn_last_error()
    assert lib.kfn_cost_volume_backward(b, None, b, 1, 2, 3, 4, None) == ARG
    assert lib.kfn_cost_volume_backward(b + 4, b, b, 1, 2, 3, 4, None) == ARG and b'misaligned' in lib.kfn_last_error()
    assert lib.kfn_flow_head_backward(b, b, b, b, b, 16, b, 16, 0, None) == ARG
    assert lib.kfn_flow_head_backward(b, b, b, b, b, 3, b, 16, 1, None) == ARG and b'strides' in lib.kfn_last_error()
    assert lib.kfn_flow_head_backward(b, b, b, None, b, 16, b, 16, 1, None) == ARG
    assert lib.kfn_l2norm_backward(b, 32, b, 32, b, 32, 1, 16, None) == ARG and b'32 channels' in lib.kfn_last_error()
    assert lib.kfn_l2norm_backward(b, 32, b, 30, b, 32, 1, 32, None) == ARG
    assert lib.kfn_l2norm_backward(b, 32, b, 32, None, 32, 1, 32, None) == ARG
    d = _lib.FlowLossDesc(P=1, h=2, w=3, label_stride=1, dist_threshold=0.05, min_uncertainty=1e-5)
    assert lib.kfn_flow_loss_grad(C.byref(d), b, b, b, b, b, None, None) == ARG
    d.label_stride = 0
    assert lib.kfn_flow_loss_grad(C.byref(d), b, b, b, b, b, b, None) == ARG and b'label_stride' in lib.kfn_last_error()
    d.label_stride, d.struct_size = 1, 40
    assert lib.kfn_flow_loss_grad(C.byref(d), b, b, b, b, b, b, None) == ARG and b'struct_size' in lib.kfn_last_error()
    d.struct_size, d.min_uncertainty = 48, 0.0
    assert lib.kfn_flow_loss_grad(C.byref(d), b, b, b, b, b, b, None) == ARG and b'thresholds' in lib.kfn_last_error()


# -- the command line --------------------------------------------------------------------------------------------------------------
def _cli(*args):
    import subprocess
    import sys
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    # a refusal must come before any device is touched: hide them all, so that touching one would be a traceback instead
    env['HIP_VISIBLE_DEVICES'] = env['CUDA_VISIBLE_DEVICES'] = ''
    return subprocess.run([sys.executable, '-m', 'kfnet_amd.OFlowNet.train'] + list(args), cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def test_command_line_help_and_refusals_exit_with_status_1_before_any_device(tmp_path):
    r = _cli('--help')
    assert r.returncode == 0 and '--scene' not in r.stdout
    for flag in ('--input_folder', '--model_folder', '--pairs', '--sequence_length', '--synthetic', '--depth', '--shuffle',
                 '--stepvalue', '--max_steps', '--snapshot', '--height', '--width', '--loss_clip'):
        assert flag in r.stdout, flag
    assert 'default 1000' in r.stdout
    base = ['--model_folder', str(tmp_path), '--synthetic', '6', '--height', '64', '--width', '96']
    for args, word in ((base + ['--augment'], '--augment'), (base[2:], '--model_folder'), (base[:-1] + ['100'], 'multiples of 8'),
                       (base[:2] + ['--synthetic', '1'] + base[4:], 'no pair'), (base + ['--pairs', '0'], '--pairs'),
                       (base + ['--sequence_length', '1'], '--sequence_length'),
                       (base[:2] + ['--input_folder', str(tmp_path / 'none')] + base[4:], 'image_list.txt')):
        r = _cli(*args)
        assert r.returncode == 1 and word in r.stderr and 'Traceback' not in r.stderr, (args, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1
    assert os.listdir(str(tmp_path)) == []


def test_parser_defaults_and_the_trainer_refuses_bad_sizes_without_a_device():
    import pytest
    from kfnet_amd.OFlowNet.train import build_parser
    from kfnet_amd.train_flow import OFlowNetTrainer
    a = build_parser().parse_args([])
    assert a.pairs == 4 and a.sequence_length == 1000 and a.stepvalue == 100000 and a.max_steps is None and a.loss_clip is None
    with pytest.raises(ValueError):
        OFlowNetTrainer({}, image_size=(60, 96))
    with pytest.raises(ValueError):
        OFlowNetTrainer({}, image_size=(64, 96), pairs=0)


def test_label_files_without_transform_txt_open_for_stage_2_only(tmp_path):
    import argparse
    from kfnet_amd.batches import open_source
    from PIL import Image
    paths = []
    for i in range(2):
        Image.fromarray(np.zeros((16, 24, 3), np.uint8)).save(str(tmp_path / ('%d.png' % i)))
        np.zeros((16, 24, 4), np.float32).tofile(str(tmp_path / ('%d.bin' % i)))
        paths.append(i)
    (tmp_path / 'image_list.txt').write_text(''.join('%s\n' % (tmp_path / ('%d.png' % i)) for i in paths))
    (tmp_path / 'label_list.txt').write_text(''.join('%s\n' % (tmp_path / ('%d.bin' % i)) for i in paths))
    a = argparse.Namespace(height=16, width=24, depth=False, synthetic=0, input_folder=str(tmp_path))
    src = open_source(a, False, needs_transform=False)
    assert src.count == 2 and src.transform is None
    frames, labels = src.batch([0, 1], False)
    assert frames.shape == (2, 16, 24, 3) and labels.shape == (2, 2, 3, 4)
    try:
        open_source(a, False)
    except OSError as e:
        assert 'transform.txt' in str(e)
    else:
        raise AssertionError('stage 1 still needs transform.txt')
