"""Joint stage 3 on the device: kfn_filter_backward_joint against fp64 autograd of tests/joint_train_ref.py and,
on the arguments they share, against kfn_filter_backward bit for bit; OFlowNetTrainer on shared frames against its default
layout; the whole joint step of kfnet_amd.train_kfnet.KFNetTrainer (gradients of both scopes, Adam, reproducibility, the fixed
path beside it, learning) and the command line.

The tolerance of every gradient comparison is the project's rule: e = max|g - g64| / max|g64| per output, for the
device and for torch-CPU fp32 autograd of the same reference on the same inputs; the device passes at e <= max(8 e_fp32, 1e-6)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import flow_train_ref as FR
import joint_train_ref as JR
import kf_train_ref as KR
import test_gpu_kfnet_train as K3
import train_ref as R
from gpu_util import dev, stream, sync
from kfnet_amd import _lib

pytestmark = pytest.mark.gpu

EPS = K3.EPS
GUARD = 64
T = 4


def passes(what, got, g64, g32):
    e, e32 = FR.rel_err(got, g64), FR.rel_err(g32, g64)
    print('%-50s e device %.3e   e torch-fp32 %.3e   bound %.3e' % (what, e, e32, K3.bound(e32)))
    assert e <= K3.bound(e32), (what, e, e32)


# -- 1. kfn_filter_backward_joint ------------------------------------------------------------------------------------------------
# (S, T, h, w, radius, reach): K3.backward_inputs with seed 0 -- flows uniform in [-reach, reach], so border samples leave the
# grid and several targets share a source -- and every flow's fraction then held inside [0.01, 0.99].  Seed 0 leaves every case
# clear of the gates (assert_clear below, checked on the CPU when the seed was chosen).
KERNEL_SEED = 0
KERNEL_CASES = [(2, 4, 5, 7, 4, 4.0), (2, 4, 9, 13, 4, 4.0), (2, 2, 9, 13, 4, 4.0), (2, 4, 9, 13, 7, 7.0), (1, 4, 60, 80, 4, 4.0)]


def kernel_inputs(S, T_, h, w, reach, seed=KERNEL_SEED):
    pred, flow, st, d_temp, d_kf = K3.backward_inputs(S, T_, h, w, reach, seed)
    whole = np.floor(flow)
    flow = (whole + np.clip(flow - whole, 0.01, 0.99)).astype(np.float32)
    return pred, flow, st, d_temp, d_kf


def assert_clear(pred, flow, st, reach):
    """Every warped position at least 0.01 (less fp32 rounding) from an integer, no flow beyond the reach, sigma_trans^2, s_l^2
    and 1 - K clear of their thresholds: no floor and no gate decides a cell."""
    frac = flow.astype(np.float64) - np.floor(flow)
    assert frac.min() >= 0.01 - 1e-6 and frac.max() <= 0.99 + 1e-6 and np.abs(flow).max() <= reach
    assert not np.any(np.abs(st.astype(np.float64) / EPS - 1.0) < K3.GATE_MARGIN)
    K3.assert_clear_of_the_gates(pred, flow, st)


def run_joint(pred, flow, st, d_temp, d_kf, radius=4, ld_dpred=16):
    """The measurement map, the scan and kfn_filter_backward_joint from a zeroed dpred, every output buffer with a guard behind
    it and -4 in the two new ones.  Returns (dpred, total d_kf, count, d_flow [S,T,h,w,2], d_sigma_trans [S,T,h,w])."""
    lib = _lib.load()
    S, T_, h, w, _ = pred.shape
    P = S * T_ * h * w
    pd = dev(pred.astype(np.float32))
    meas = torch.zeros((P, 4), device='cuda')
    _lib.check(lib.kfn_measurement_map(pd.data_ptr(), 4, meas.data_ptr(), P, stream()), 'kfn_measurement_map')
    sync()
    temp, kf = K3.run_scan(flow, st, meas.cpu().numpy().reshape(pred.shape))
    bd = _lib.FilterBackwardDesc(S=S, T=T_, H=h, W=w, ld_dpred=ld_dpred, radius=radius, min_uncertainty=EPS)
    nb = C.c_size_t()
    _lib.check(lib.kfn_filter_backward_scratch_bytes(C.byref(bd), C.byref(nb)), 'scratch bytes')
    scratch = torch.full((nb.value // 4 + GUARD,), -9.0, device='cuda')
    dp = torch.zeros((P + GUARD, ld_dpred), device='cuda')
    dp[:, 4:] = -5.0
    dp[P:] = -5.0
    dk = torch.full((P + GUARD, 4), -3.0, device='cuda')
    dk[:P] = dev(d_kf.astype(np.float32).reshape(P, 4))
    df = torch.full((P + GUARD, 2), -4.0, device='cuda')
    ds = torch.full((P + GUARD,), -4.0, device='cuda')
    stats = torch.full((16,), -1.0, device='cuda')
    fd, sd, td, kd, dtd = dev(flow.astype(np.float32)), dev(st.astype(np.float32)), dev(temp), dev(kf), dev(d_temp.astype(np.float32))
    _lib.check(lib.kfn_filter_backward_joint(C.byref(bd), fd.data_ptr(), sd.data_ptr(), meas.data_ptr(), td.data_ptr(), kd.data_ptr(),
                                             dtd.data_ptr(), dk.data_ptr(), dp.data_ptr(), df.data_ptr(), ds.data_ptr(),
                                             stats.data_ptr(), scratch.data_ptr(), stream()), 'kfn_filter_backward_joint')
    sync()
    dph, dkh, dfh, dsh, sh = dp.cpu().numpy(), dk.cpu().numpy(), df.cpu().numpy(), ds.cpu().numpy(), stats.cpu().numpy()
    assert np.all(dph[:, 4:] == -5.0) and np.all(dph[P:] == -5.0), 'wrote outside the four gradient channels'
    assert np.all(dkh[P:] == -3.0) and np.all(scratch.cpu().numpy()[-GUARD:] == -9.0), 'wrote past d_kf or the scratch buffer'
    assert np.all(dfh[P:] == -4.0) and np.all(dsh[P:] == -4.0), 'wrote past d_flow or d_sigma_trans'
    assert np.all(np.delete(sh, 11) == -1.0), 'the reverse scan owns word 11 of stats alone'
    return (dph[:P, :4].reshape(pred.shape), dkh[:P].reshape(pred.shape), int(sh.view(np.uint32)[11]),
            dfh[:P].reshape(S, T_, h, w, 2), dsh[:P].reshape(S, T_, h, w))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('case', KERNEL_CASES, ids=['S%d-T%d-%dx%d-r%d' % c[:5] for c in KERNEL_CASES])
def test_filter_backward_joint_against_fp64_autograd_and_the_fixed_entry_point(case):
    S, T_, h, w, radius, reach = case
    pred, flow, st, d_temp, d_kf = kernel_inputs(S, T_, h, w, reach)
    assert_clear(pred, flow, st, reach)
    if (h, w) == (5, 7):
        xs = np.arange(w)[None, None, None, :] + flow[..., 0]
        assert (xs[:, 1:] < 0).any() and (xs[:, 1:] > w - 1).any()            # border samples leave the grid
    g, dk, count, df, ds = run_joint(pred, flow, st, d_temp, d_kf, radius)
    assert count == 0
    # the arguments the two entry points share: the same bits
    g0, dk0, count0, _, _ = K3.run_backward(pred, flow, st, d_temp, d_kf, radius)
    assert count0 == count and np.array_equal(bits(g), bits(g0)) and np.array_equal(bits(dk), bits(dk0))
    # the two new outputs, every cell of every frame
    p64, f64, s64 = JR.backward_grads(pred, flow, st, d_temp, d_kf, torch.float64)
    p32, f32, s32 = JR.backward_grads(pred, flow, st, d_temp, d_kf, torch.float32)
    passes('joint %s d_flow' % (case,), df, f64, f32)
    passes('joint %s d_sigma_trans' % (case,), ds, s64, s32)
    assert not df[:, 0].any() and not ds[:, 0].any() and not f64[:, 0].any() and not s64[:, 0].any()
    assert np.all(ds[:, 1:] != 0.0) and df[:, 1:].any()
    # bit-identical from launch to launch
    again = run_joint(pred, flow, st, d_temp, d_kf, radius)
    for a, b in zip((g, dk, df, ds), (again[0], again[1], again[3], again[4])):
        assert np.array_equal(bits(a), bits(b))


def test_filter_backward_joint_hand_cases():
    S, T_, h, w = 2, 4, 9, 13
    pred, flow, st, d_temp, d_kf = kernel_inputs(S, T_, h, w, 4.0, seed=3)
    flow[:, 1:, :, 0, 0] = -1.5            # column 0 sampled to the left of the grid: both x corners clamp to column 0
    flow[:, 1:, h - 1, :, 1] = 2.25        # the last row sampled below it
    st[1, 2, 3:5] = 3e-6                   # sigma_trans^2 <= eps^2
    st[1, 3, 0, 0] = np.float32(EPS)       # the gate is strict
    # sequence 0, frame 0: sigma_z = 1e-7 everywhere, so every s_l of frame 1 lies below the variance floor
    pred[0, 0, ..., 3] = np.log(1e-7)
    g, dk, count, df, ds = run_joint(pred, flow, st, d_temp, d_kf)
    assert count == 0 and np.isfinite(df).all() and np.isfinite(ds).all()
    xs = np.arange(w, dtype=np.float32)[None, None, None, :] + flow[..., 0]
    ys = np.arange(h, dtype=np.float32)[None, None, :, None] + flow[..., 1]
    one_x = np.clip(np.floor(xs), 0, w - 1) == np.clip(np.floor(xs) + 1, 0, w - 1)
    one_y = np.clip(np.floor(ys), 0, h - 1) == np.clip(np.floor(ys) + 1, 0, h - 1)
    outside = (one_x | one_y)[:, 1:]
    assert outside[..., 0].all() and outside[:, :, h - 1].all() and not outside.all()
    # both corners clamped to one cell: exact zeros (a sample outside along the other axis has weights w_0 = -w_1 there)
    assert np.all(df[:, 1:][outside] == 0.0) and np.all(df[:, 1:][~outside] != 0.0)
    assert np.all(ds[1, 2, 3:5] == 0.0) and ds[1, 3, 0, 0] == 0.0 and np.all(ds[1, 2, :3] != 0.0)
    assert not df[:, 0].any() and not ds[:, 0].any()                              # frame 0: zeros over the -4 fill
    # s_l^2 <= eps^2: whatever sigma KF_0 holds below the floor, its channel adds nothing to frame 1's d_flow
    other = pred.copy()
    other[0, 0, ..., 3] = np.log(np.random.default_rng(6).uniform(1e-8, 5e-6, size=(h, w)))
    _, dk2, _, df2, ds2 = run_joint(other, flow, st, d_temp, d_kf)
    assert np.array_equal(df[0, 1], df2[0, 1]) and df[0, 1].any()
    assert np.array_equal(dk[0, 0, ..., 3], d_kf[0, 0, ..., 3]) and np.array_equal(dk2[0, 0, ..., 3], d_kf[0, 0, ..., 3])
    assert np.any(dk[1, 0, ..., 3] != d_kf[1, 0, ..., 3])                         # the other sequence's sigma is sampled
    # and fp64 autograd says the same of all of it
    _, f64, s64 = JR.backward_grads(pred, flow, st, d_temp, d_kf)
    _, f32, s32 = JR.backward_grads(pred, flow, st, d_temp, d_kf, torch.float32)
    passes('hand cases d_flow', df, f64, f32)
    passes('hand cases d_sigma_trans', ds, s64, s32)


# -- 2. OFlowNetTrainer on shared frames -----------------------------------------------------------------------------------------
def test_pair_index_on_four_shared_frames_equals_the_default_layout_on_duplicated_frames():
    from kfnet_amd.synth import synthetic_sequence
    from kfnet_amd.train import synthetic_labels
    from kfnet_amd.train_flow import OFlowNetTrainer
    from kfnet_amd.train_kfnet import pair_table
    from kfnet_amd.weights import synthetic_weights
    size, seed = (64, 96), 39                                  # DESIGN.md 6f's inputs for this size
    frames = synthetic_sequence(T, size[0], size[1], seed=seed)
    labels = synthetic_labels(T, (size[0] // 8, size[1] // 8))
    W = {k: v for k, v in synthetic_weights(seed=100 + seed).items() if k.startswith('Temporal/')}
    a, b = pair_table(1, T)
    dup = np.stack([a, b], 1).reshape(-1)                      # 0 1 1 2 2 3
    plain = OFlowNetTrainer(W, image_size=size, pairs=T - 1)
    plain.stage(frames[dup], labels[dup])
    plain.forward()
    plain.loss()
    plain.backward()
    shared = OFlowNetTrainer(W, image_size=size, pairs=T - 1, frames=T, pair_index=(a, b))
    assert shared.frames.shape[0] == T and shared.feat.shape[0] == T * 8 * 12 and shared.tower[0].y.n == T
    assert shared.stage(frames) is None
    shared.forward()
    with pytest.raises(ValueError):
        shared.loss()
    shared.backward(plain.d_flow, plain.d_sigma)
    sync()
    # the gathers pick the frames the default layout holds twice (another frame would move the flow by whole cells)
    assert np.abs(shared.flow.cpu().numpy() - plain.flow.cpu().numpy()).max() <= 1e-4
    np.testing.assert_allclose(shared.sigma.cpu().numpy(), plain.sigma.cpu().numpy(), rtol=1e-4)
    gp, gs = plain.gradients(), shared.gradients()
    _, g64 = FR.step_loss_and_grads(frames[dup], labels[dup], W)
    _, g32 = FR.step_loss_and_grads(frames[dup], labels[dup], W, dtype=torch.float32)
    for name in sorted(g64):
        if name == 'Temporal/prediction/bias':                 # zero by the softmax's symmetry
            assert np.abs(gs[name]).max() <= 1e-6 * np.abs(g64['Temporal/prediction/kernel']).max()
            continue
        passes('shared frames %s' % name, gs[name], g64[name], g32[name])
        passes('default layout %s' % name, gp[name], g64[name], g32[name])
    # a device batch is read where it lies; twice the same bits
    again = OFlowNetTrainer(W, image_size=size, pairs=T - 1, frames=T, pair_index=(a, b))
    on_device = dev(frames)
    again.stage(on_device)
    assert again.frames.data_ptr() == on_device.data_ptr()
    again.forward()
    again.backward(plain.d_flow, plain.d_sigma)
    sync()
    ga = again.gradients()
    assert all(np.array_equal(bits(ga[n]), bits(gs[n])) for n in gs)


# -- 3. the whole joint step -----------------------------------------------------------------------------------------------------
# synthetic_sequence(seed) with initial_weights(seed) for both scopes: an untrained graph, whose flows sit near -0.5 cells (the
# mean of the offsets -4 .. 3).  Of seeds 1..40 these have the largest smallest fp64 |pre-activation| over every ReLU unit of
# both networks (JR.smallest_preactivation, found on the CPU): 4.5e-9 at 64x96 with one group, 1.2e-9 at 72x104 with two.
STEP_CASES = {(64, 96): (1, 33), (72, 104): (2, 19)}
ZERO_BY_SYMMETRY = 'Temporal/prediction/bias'


def _step_inputs(size):
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    from kfnet_amd.train import synthetic_labels
    from kfnet_amd.weights import initial_weights
    S, seed = STEP_CASES[size]
    frames = synthetic_sequence(S * T, size[0], size[1], seed=seed)
    labels = synthetic_labels(S * T, (size[0] // 8, size[1] // 8))
    return S, frames, labels, synthetic_transform().astype(np.float32), initial_weights(seed, scopes=('ScoreNet', 'Temporal'))


@functools.lru_cache(maxsize=None)
def _reference(size):
    """The fp64 and the torch-fp32 gradients of one joint step: computed once, shared, never written to."""
    S, frames, labels, M, W = _step_inputs(size)
    return JR.loss_and_grads(frames, labels, W, S, T, M), JR.loss_and_grads(frames, labels, W, S, T, M, dtype=torch.float32)


def _trainer(size, W, S, M, **kw):
    from kfnet_amd.train_kfnet import KFNetTrainer
    return KFNetTrainer(W, image_size=size, groups=S, transform=M, base_lr=1e-4, weight_decay=1e-4, **kw)


@pytest.mark.parametrize('size', sorted(STEP_CASES), ids=['64x96-S1', '72x104-S2'])
def test_one_joint_step_gradients_and_update_of_both_scopes_against_fp64(size):
    S, frames, labels, M, W = _step_inputs(size)
    (s64, g64, flow64), (s32, g32, _) = _reference(size)
    tr = _trainer(size, W, S, M, train_flownet=True)
    stats = dict(tr.step(frames, labels))
    g = tr.gradients()
    h, w = size[0] // 8, size[1] // 8
    flow = tr.c_flow.cpu().numpy().reshape(S, T, h, w, 2)
    # untrained flows: near -0.5 cells, so no warped position is within 0.05 of a step of the sampler's floor
    for f in (flow[:, 1:], flow64[:, 1:]):
        assert f.min() >= -0.95 and f.max() <= -0.05, (f.min(), f.max())
    assert np.abs(flow[:, 1:] - flow64[:, 1:]).max() <= 1e-4 and not flow[:, 0].any()
    for k in ('loss', 'l_measure', 'l_temp', 'l_KF', 'a_measure', 'a_temp', 'a_KF', 'pixels'):
        print('%-10s device %.7g torch-fp32 %.7g fp64 %.7g' % (k, stats[k], s32[k], s64[k]))
    assert abs(stats['loss'] - s64['loss']) <= 1e-4 * abs(s64['loss'])
    assert stats['pixels'] == float((labels[..., 3] == 1.0).sum()) and stats['lr'] == 1e-4
    assert sorted(g) == sorted(g64) == sorted(W)
    for scope in ('ScoreNet', 'Temporal'):
        e_dev, e_32 = {}, {}
        for name in sorted(n for n in g64 if n.startswith(scope + '/')):
            if name == ZERO_BY_SYMMETRY:
                scale = np.abs(g64['Temporal/prediction/kernel']).max()
                assert np.abs(g[name]).max() <= 1e-6 * scale and np.abs(g64[name]).max() <= 1e-12 * scale
                continue
            e_dev[name], e_32[name] = FR.rel_err(g[name], g64[name]), FR.rel_err(g32[name], g64[name])
            print('%-32s e device %.3e  e torch-fp32 %.3e' % (name, e_dev[name], e_32[name]))
        worst_dev, worst_32 = max(e_dev.values()), max(e_32.values())
        print('%s worst e: device %.3e, torch-CPU fp32 %.3e, bound %.3e' % (scope, worst_dev, worst_32, K3.bound(worst_32)))
        assert worst_dev <= K3.bound(worst_32), scope
    # the filter's loss reaches OFlowNet: its gradients are not zero
    assert np.abs(g64['Temporal/feat1/kernel']).max() > 0 and np.abs(g64['Temporal/uncertainty/kernel']).max() > 0
    # the update: numpy Adam on the device's own gradients, bit for bit, both scopes with one step count
    after, st_ = tr.weights(), tr.state()
    assert int(st_['global_step']) == 1 and int(st_['adam_t']) == 1 and tr.ft.global_step == 1 and tr.ft.adam_t == 1
    assert sorted(after) == sorted(W) and sorted(k[7:] for k in st_ if k.startswith('adam_m/')) == sorted(W)
    for name in sorted(g):
        z = np.zeros_like(W[name])
        w1, m1, v1 = R.adam_step(W[name], z, z, g[name], 1e-4, 1, 1e-4)
        for what, got, want in (('w', after[name], w1), ('m', st_['adam_m/' + name], m1), ('v', st_['adam_v/' + name], v1)):
            assert np.array_equal(bits(got), bits(want)), (name, what)
    assert all(not np.array_equal(after[k], W[k]) for k in W if k.startswith('Temporal/') and k.endswith('kernel'))


def test_two_joint_trainers_give_the_same_bits_and_the_fixed_path_leaves_temporal_alone():
    size = (64, 96)
    S, frames, labels, M, W = _step_inputs(size)
    runs = []
    for overlap in (True, True, False):                        # the third on one stream: the same launches in another order
        tr = _trainer(size, W, S, M, train_flownet=True, overlap=overlap)
        first = dict(tr.step(frames, labels))
        tr.step(frames, labels)
        sync()
        runs.append((first['loss'], tr.gradients(), tr.weights()))
    for other in runs[1:]:
        assert other[0] == runs[0][0]
        assert all(np.array_equal(bits(other[1][k]), bits(runs[0][1][k])) for k in W)
        assert all(np.array_equal(bits(other[2][k]), bits(runs[0][2][k])) for k in W)
    fixed = _trainer(size, W, S, M)
    assert fixed.train_flownet is False and fixed.engine is not None
    loss = fixed.step(frames, labels)['loss']
    fixed.step(frames, labels)
    sync()
    out = fixed.weights()
    assert sorted(fixed.gradients()) == sorted(k for k in W if k.startswith('ScoreNet/'))
    for k in W:
        if k.startswith('Temporal/'):
            assert np.array_equal(bits(out[k]), bits(W[k])), k
            assert k.endswith('bias') or not np.array_equal(runs[0][2][k], W[k]), k
    # the frozen engine and the trainer see the same pairs (t - 1, t): one loss, up to their kernels' rounding
    print('loss of the first step: fixed %.7g, joint %.7g' % (loss, runs[0][0]))
    assert abs(loss - runs[0][0]) <= 1e-4 * abs(loss)


def test_ten_joint_steps_on_one_group_follow_the_fp64_run():
    """Both networks trained for ten updates on one group at 64x96 (seed 33).  Measured on an MI355X: L 2011.912 -> 1905.214 on
    the device, 2011.912 -> 1905.166 in the fp64 run (2.5e-5 relative; the bound is the 5 % of the other ten-step tests)."""
    from kfnet_amd.train import learning_rate
    size = (64, 96)
    S, frames, labels, M, W = _step_inputs(size)
    tr = _trainer(size, W, S, M, train_flownet=True)
    dev_losses = [tr.step(frames, labels)['loss'] for _ in range(11)]          # entry i = the loss after i updates
    ref = {k: v.copy() for k, v in W.items()}
    m = {k: np.zeros_like(v) for k, v in ref.items()}
    v_ = {k: np.zeros_like(v) for k, v in ref.items()}
    ref_losses = []
    for t in range(1, 12):
        s, g, _ = JR.loss_and_grads(frames, labels, ref, S, T, M)
        ref_losses.append(s['loss'])
        lr = learning_rate(1e-4, 0.5, 80000, t - 1)
        for k in ref:
            ref[k], m[k], v_[k] = R.adam_step(ref[k], m[k], v_[k], g[k].astype(np.float32), lr, t, 1e-4)
    for i in (0, 1, 5, 10):
        print('after %2d updates: device L %.6f, fp64 run %.6f' % (i, dev_losses[i], ref_losses[i]))
    assert ref_losses[10] < ref_losses[0] and dev_losses[10] < dev_losses[0]
    assert abs(dev_losses[0] - ref_losses[0]) <= 1e-4 * abs(ref_losses[0])
    assert abs(dev_losses[10] - ref_losses[10]) <= 0.05 * abs(ref_losses[10])


# -- 4. the command line ---------------------------------------------------------------------------------------------------------
def test_joint_command_line_snapshots_both_scopes_eval_reads_them_and_a_run_resumes(tmp_path):
    from kfnet_amd.weights import initial_weights, load_npz
    whole, parts, out = tmp_path / 'whole', tmp_path / 'parts', tmp_path / 'o'
    out.mkdir()
    small = ['--height', '64', '--width', '96', '--scene', 'fire', '--synthetic', '8', '--joint', '--display', '3']
    log = K3._cli('kfnet_amd.KFNet.train', ['--model_folder', str(whole), '--max_steps', '6', '--snapshot', '3'] + small)
    assert sorted(os.listdir(str(whole))) == ['kfnet_train_state-3.npz', 'kfnet_train_state-6.npz', 'kfnet_weights-3.npz',
                                              'kfnet_weights-6.npz']
    assert 'step 6/6' in log and 'l_temp=' in log and 'current step:  0' in log
    assert 'nothing restores ScoreNet' in log and 'nothing restores Temporal' in log
    saved = load_npz(str(whole / 'kfnet_weights-6.npz'))
    start = initial_weights(0, scopes=('ScoreNet', 'Temporal'))
    assert sorted(saved) == sorted(start)
    assert all(not np.array_equal(saved[k], start[k]) for k in start if k.endswith('kernel'))
    with np.load(str(whole / 'kfnet_train_state-6.npz')) as z:
        state = {k: z[k] for k in z.files}
    assert sorted(k[7:] for k in state if k.startswith('adam_m/')) == sorted(start) and int(state['global_step']) == 6
    K3._cli('kfnet_amd.KFNet.eval', ['--model_folder', str(whole), '--synthetic', '4', '--output_folder', str(out), '--height', '64',
                                     '--width', '96', '--scene', 'fire'])
    recs = [np.load(str(out / ('coord_%d.npy' % i))) for i in range(4)]
    assert all(r.shape == (8, 12, 4) and np.isfinite(r).all() for r in recs)
    # interrupted at step 3, then resumed: the arrays of the uninterrupted run
    K3._cli('kfnet_amd.KFNet.train', ['--model_folder', str(parts), '--max_steps', '3', '--snapshot', '3'] + small)
    log = K3._cli('kfnet_amd.KFNet.train', ['--model_folder', str(parts), '--max_steps', '6', '--snapshot', '3'] + small)
    assert 'current step:  3' in log and 'Adam slots restored' in log and 'start at zero' not in log
    resumed = load_npz(str(parts / 'kfnet_weights-6.npz'))
    assert all(np.array_equal(bits(resumed[k]), bits(saved[k])) for k in saved)
    with np.load(str(parts / 'kfnet_train_state-6.npz')) as z:
        assert sorted(z.files) == sorted(state) and all(np.array_equal(z[k], state[k]) for k in state)
