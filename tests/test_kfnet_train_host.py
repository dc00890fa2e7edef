"""Host side of fine-tuning SCoordNet through the Kalman filter (kfnet_amd/train_kfnet.py, kfnet_amd/KFNet/train.py; DESIGN.md
6e): the group list and its step-addressed stream, the schedule, the refusals of the command line, the new exports, and the
reference of the GPU tests (tests/kf_train_ref.py) against the oracle's sampler, process model and Kalman update."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kf_train_ref as KR
from kfnet_amd import _lib
from kfnet_amd.train_kfnet import GROUP, group_indices, group_list, sequence_length, start_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kfn_measurement_map', 'kfn_filter_loss_grad', 'kfn_filter_backward_scratch_bytes', 'kfn_filter_backward')


# -- groups ------------------------------------------------------------------------------------------------------------------
def test_group_list_follows_get_indexes_on_and_off_a_sequence_boundary():
    assert GROUP == 4 and sequence_length('stairs') == 500 and sequence_length('fire') == 1000
    g = group_list(6, 1000)
    assert g == [[0, 1, 2, 3], [3, 2, 1, 0], [1, 2, 3, 4], [4, 3, 2, 1], [2, 3, 4, 5], [5, 4, 3, 2]]
    # two full ranges of 5: no group straddles frame 4 | 5
    g = group_list(10, 5)
    assert g == [[0, 1, 2, 3], [3, 2, 1, 0], [1, 2, 3, 4], [4, 3, 2, 1], [5, 6, 7, 8], [8, 7, 6, 5], [6, 7, 8, 9], [9, 8, 7, 6]]
    assert all(max(x) // 5 == min(x) // 5 for x in g)
    # a tail range of 3 frames yields nothing, one of 4 yields one group and its reverse
    assert group_list(8, 5) == group_list(5, 5)
    assert group_list(9, 5)[-2:] == [[5, 6, 7, 8], [8, 7, 6, 5]]
    assert group_list(3, 1000) == []
    # the reference's counts: 2 (L - 3) per full range
    assert len(group_list(2000, 1000)) == 2 * 2 * 997 and len(group_list(2000, 500)) == 4 * 2 * 497
    for fwd, rev in zip(g[0::2], g[1::2]):
        assert rev == fwd[::-1]


def test_the_stream_of_groups_wraps_and_shuffle_is_reproducible_and_step_addressed():
    g = group_list(7, 1000)                    # 8 groups
    assert len(g) == 8
    assert group_indices(0, 1, g) == g[0] and group_indices(1, 1, g) == g[1] and group_indices(8, 1, g) == g[0]
    assert group_indices(3, 2, g) == g[6] + g[7] and group_indices(4, 2, g) == g[0] + g[1]
    assert group_indices(1, 3, g) == g[3] + g[4] + g[5] and group_indices(2, 3, g) == g[6] + g[7] + g[0]
    a = [group_indices(s, 2, g, True, 5) for s in range(12)]
    b = [group_indices(s, 2, g, True, 5) for s in reversed(range(12))][::-1]       # any order of asking: a function of the step
    assert a == b
    assert a != [group_indices(s, 2, g, True, 6) for s in range(12)]
    for e in range(3):                                                         # every epoch is a permutation of the groups
        epoch = [tuple(x[i:i + 4]) for x in a[4 * e:4 * e + 4] for i in (0, 4)]
        assert sorted(epoch) == sorted(tuple(x) for x in g)
    assert a[0:4] != a[4:8]


def test_schedule_and_the_reset_step_rule():
    from kfnet_amd.KFNet.train import build_parser, format_line
    from kfnet_amd.SCoordNet.train import schedule
    assert schedule('fire') == (30000, 150000) and schedule('fire', max_steps=7) == (30000, 7)
    assert start_step(1234, 30000, -1, '', '') == 1234
    assert start_step(1234, 30000, 50, '', '') == 50
    assert start_step(1234, 30000, -1, 'a', '') == 1234 and start_step(1234, 30000, -1, '', 'b') == 1234
    assert start_step(1234, 30000, -1, 'a', 'b') == 120000 and start_step(0, 100000, 7, 'a', 'b') == 400000
    a = build_parser().parse_args(['--fix_flownet'])
    assert a.fix_flownet and a.groups == 1 and a.scoordnet == '' and a.oflownet == '' and a.loss_clip is None
    line = format_line('now', 2, 30, 100, [4, 5, 6, 7], dict(loss=1.5, l_measure=1.25, l_temp=2.0, l_KF=0.5, a_measure=0.5,
                                                             a_temp=0.25, a_KF=0.75, pixels=95.0, lr=1e-4), 0.25)
    assert line == ('[now] epoch 2, step 30/100,     4~    5~    6~    7, loss=1.500, l_measure=1.250, l_temp=2.000, l_KF= 0.500, '
                    'a_measure=0.500, a_temp=0.250,a_KF=0.750, #pixels=95, lr = 0.000100 (0.250 sec/step)')


def _cli(*args):
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    # a refusal must come before any device is touched: hide them all, so that touching one would be a traceback instead
    env['HIP_VISIBLE_DEVICES'] = env['CUDA_VISIBLE_DEVICES'] = ''
    return subprocess.run([sys.executable, '-m', 'kfnet_amd.KFNet.train'] + list(args), cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def test_command_line_refusals_exit_with_status_1_before_any_device(tmp_path):
    r = _cli('--help')
    assert r.returncode == 0
    for flag in ('--scoordnet', '--oflownet', '--fix_flownet', '--groups', '--sequence_length', '--model_folder', '--reset_step',
                 '--shuffle', '--loss_clip', '--depth', '--synthetic'):
        assert flag in r.stdout, flag
    base = ['--scene', 'fire', '--model_folder', str(tmp_path), '--synthetic', '8', '--height', '64', '--width', '96']
    r = _cli(*base)
    assert r.returncode == 1 and 'training OFlowNet is not built' in r.stderr and 'Traceback' not in r.stderr
    assert len(r.stderr.strip().splitlines()) == 1
    r = _cli(*(base + ['--fix_flownet', '--augment']))
    assert r.returncode == 1 and '--augment' in r.stderr and 'Traceback' not in r.stderr
    r = _cli(*(base[:-1] + ['100', '--fix_flownet']))
    assert r.returncode == 1 and 'multiples of 8' in r.stderr and 'Traceback' not in r.stderr
    r = _cli('--scene', 'fire', '--model_folder', str(tmp_path), '--synthetic', '3', '--height', '64', '--width', '96', '--fix_flownet')
    assert r.returncode == 1 and 'no group' in r.stderr and 'Traceback' not in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_trainer_refuses_bad_sizes_without_a_device():
    from kfnet_amd.train_kfnet import KFNetTrainer
    with pytest.raises(ValueError):
        KFNetTrainer({}, image_size=(60, 96))
    with pytest.raises(ValueError):
        KFNetTrainer({}, image_size=(64, 96), groups=0)


# -- exports -----------------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_bound_and_check_their_arguments_without_a_device():
    header = open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()
    lib = _lib.load()
    assert lib.kfn_abi_version() == 13 and '#define KFN_ABI_VERSION 13' in header
    for name in NEW:
        assert re.search(r'\bint %s\(' % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    for struct, cls in (('kfn_filter_loss_desc', _lib.FilterLossDesc), ('kfn_filter_backward_desc', _lib.FilterBackwardDesc)):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct), header, re.S).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        fields = [f.strip().split('[')[0] for decl in re.findall(r'(?:int32_t|float|double)\s+([^;]+);', body) for f in decl.split(',')]
        assert fields == [f[0] for f in cls._fields_], struct
    ARG = -1
    buf = np.zeros(64, np.float32).ctypes.data
    assert lib.kfn_measurement_map(buf, 3, buf, 4, None) == ARG and lib.kfn_measurement_map(None, 4, buf, 4, None) == ARG
    ld = _lib.FilterLossDesc(B=1, h=2, w=2, ld_pred=4, ld_dpred=4, label_stride=1, img_stride=8, smooth_weight=50.0,
                             weight_measure=0.2, weight_temporal=0.2, weight_kf=0.6, dist_threshold=0.05, min_uncertainty=1e-5)
    assert lib.kfn_filter_loss_grad(C.byref(ld), buf, buf, buf, buf, None, buf, buf, buf, buf, None) == ARG
    assert b'frames' in lib.kfn_last_error()
    ld.smooth_weight, ld.struct_size = 0.0, 8
    assert lib.kfn_filter_loss_grad(C.byref(ld), buf, buf, buf, buf, None, buf, buf, buf, buf, None) == ARG
    bd = _lib.FilterBackwardDesc(S=1, T=4, H=5, W=7, ld_dpred=16, radius=4, min_uncertainty=1e-5)
    nb = C.c_size_t()
    assert lib.kfn_filter_backward_scratch_bytes(C.byref(bd), C.byref(nb)) == 0 and nb.value == 2 * 35 * 16
    bd.radius = 3
    assert lib.kfn_filter_backward(C.byref(bd), buf, buf, buf, buf, buf, buf, buf, buf, buf, None) == ARG
    assert b'radius' in lib.kfn_last_error()
    bd.radius = 4
    assert lib.kfn_filter_backward(C.byref(bd), buf, buf, buf, buf, buf, buf, buf, buf, None, None) == ARG


# -- the reference -------------------------------------------------------------------------------------------------------------
def test_reference_sampler_equals_the_oracle_on_random_and_out_of_range_coordinates():
    import torch
    from oracle.kfnet_oracle_torch import bilinear_sampler
    rng = np.random.default_rng(0)
    for (h, w) in ((5, 7), (9, 13)):
        img = rng.normal(size=(1, h, w, 4)).astype(np.float32)
        for spread in (1.0, 6.0, 40.0):            # the last puts most coordinates outside the image
            coords = np.stack([rng.uniform(-spread, w - 1 + spread, size=(1, h, w)),
                               rng.uniform(-spread, h - 1 + spread, size=(1, h, w))], -1).astype(np.float32)
            coords[0, 0, 0] = (-0.0, h - 1.0)          # exactly on corners and edges
            coords[0, 0, 1] = (w - 1.0, 0.0)
            want = bilinear_sampler(img, coords)
            got = KR.sampler(torch.from_numpy(img), torch.from_numpy(coords)).numpy()
            assert np.array_equal(got, want), (h, w, spread)
    # batches address their own image
    img = rng.normal(size=(3, 5, 7, 2)).astype(np.float32)
    coords = np.stack([rng.uniform(-2, 8, size=(3, 5, 7)), rng.uniform(-2, 6, size=(3, 5, 7))], -1).astype(np.float32)
    got = KR.sampler(torch.from_numpy(img), torch.from_numpy(coords)).numpy()
    for b in range(3):
        assert np.array_equal(got[b:b + 1], bilinear_sampler(img[b:b + 1], coords[b:b + 1]))


def test_reference_filter_equals_process_model_and_build_kf_coord():
    import torch
    from oracle.kfnet_oracle_torch import build_kf_coord, process_model
    rng = np.random.default_rng(1)
    h, w, T = 5, 7, 4
    offsets = np.array([(j - 4, i - 4) for i in range(8) for j in range(8)], dtype=np.float32)
    logits = 3.0 * rng.normal(size=(T, h * w, 64))
    prob = (np.exp(logits) / np.exp(logits).sum(-1, keepdims=True)).astype(np.float32)
    st = (10.0 ** rng.uniform(-7, -1, size=(T, h, w))).astype(np.float32)          # below and above the variance floor
    meas = rng.normal(size=(1, T, h, w, 4)).astype(np.float32)
    meas[..., 3] = 10.0 ** rng.uniform(-7, -1, size=(1, T, h, w))
    flow = np.zeros((1, T, h, w, 2), np.float32)
    sx, ss = meas[:, 0, ..., 0:3], meas[:, 0, ..., 3:4]
    want_t, want_k = [meas[:, 0]], [meas[:, 0]]
    for t in range(1, T):
        tx, ts, fl = process_model(prob[t], st[t], offsets, sx, ss)
        flow[:, t] = fl
        sx, ss = build_kf_coord(tx, ts, meas[:, t, ..., 0:3], meas[:, t, ..., 3:4])
        want_t.append(np.concatenate([tx, ts], -1))
        want_k.append(np.concatenate([sx, ss], -1))
    temp, kf = KR.filter_forward(torch.from_numpy(meas), flow, st[None])
    np.testing.assert_allclose(temp.numpy(), np.stack(want_t, 1), rtol=2e-6, atol=1e-9)
    np.testing.assert_allclose(kf.numpy(), np.stack(want_k, 1), rtol=2e-6, atol=1e-9)
    assert np.array_equal(temp.numpy()[:, 0], meas[:, 0]) and np.array_equal(kf.numpy()[:, 0], meas[:, 0])
    assert np.abs(flow[:, 1:]).max() <= 4.0


def test_reference_step_loss_gradient_matches_finite_differences():
    import torch
    rng = np.random.default_rng(2)
    S, T, h, w = 1, 3, 4, 5
    pred = rng.normal(size=(S * T, h, w, 4))
    pred[..., 3] = rng.uniform(-2.0, 0.0, size=(S * T, h, w))
    flow = rng.uniform(-2.0, 2.0, size=(S, T, h, w, 2))
    st = 10.0 ** rng.uniform(-2, -1, size=(S, T, h, w))
    labels = rng.normal(size=(S * T, h, w, 4))
    labels[..., 3] = rng.uniform(size=(S * T, h, w)) < 0.8
    img = rng.integers(0, 256, size=(S * T, h, w, 3)).astype(np.float64)
    img[:, :, 2:] = img[:, :, 2:3]
    p = torch.from_numpy(pred).requires_grad_(True)
    L = KR.step_loss(p, S, T, flow, st, labels, img)[0]
    g, = torch.autograd.grad(L, [p])
    eps = 1e-6
    for idx in [(0, 1, 2, 0), (0, 0, 0, 3), (1, 3, 4, 1), (2, 2, 2, 3), (1, 0, 4, 2), (0, 3, 0, 3)]:
        hi, lo = pred.copy(), pred.copy()
        hi[idx] += eps
        lo[idx] -= eps
        fd = (KR.step_loss(torch.from_numpy(hi), S, T, flow, st, labels, img)[0].item() -
              KR.step_loss(torch.from_numpy(lo), S, T, flow, st, labels, img)[0].item()) / (2 * eps)
        assert abs(fd - g[idx].item()) <= 1e-6 * max(1.0, abs(fd)), (idx, fd, g[idx].item())
    # frame 0 feels the later frames: its gradient differs from the measurement term's alone
    Lm = KR.filter_loss(p, p.detach(), p.detach(), labels, img, weights=(0.2, 0.0, 0.0))[0]
    gm, = torch.autograd.grad(Lm, [p])
    assert (g[0] - gm[0]).abs().max() > 1e-3
