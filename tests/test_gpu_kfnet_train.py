"""Fine-tuning SCoordNet through the Kalman filter on the device: the forward identity with the eval scan, the
reverse scan and the three-term loss against fp64 autograd of tests/kf_train_ref.py, a whole step's gradients and update,
reproducibility, resuming, the command line, and learning on one group.

The tolerance of every gradient comparison: e = max|g - g64| / max|g64| per output, for the device and for torch-CPU fp32
autograd of the same reference on the same inputs; the device passes when its e is at most 8 times the fp32 figure, with a
floor of 1e-6 (an output whose fp32 figure happens to be tiny)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import kf_train_ref as KR
import test_gpu_train as G1
import train_ref as R
from gpu_util import dev, stream, sync
from kfnet_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (64, 96)
EPS = 1e-5                        # min_uncertainty
GATE_MARGIN = 1e-3                # no input within this, relative, of a gate


def bound(e32):
    return max(8.0 * e32, 1e-6)


def rel_err(g, g64):
    return float(np.abs(np.asarray(g, np.float64) - g64).max() / np.abs(g64).max())


# -- device calls ---------------------------------------------------------------------------------------------------------------
def run_scan(flow, st, meas):
    """kfn_kalman_scan_ex as the trainer calls it: (temp, kf) [S,T,h,w,4]."""
    import torch
    lib = _lib.load()
    S, T, h, w, _ = meas.shape
    d = _lib.KalmanDesc(S=S, T=T, H=h, W=w, t0=0, reset_period=T, min_uncertainty=EPS, nis_gate=0.0, has_transform=0)
    need = C.c_size_t(0)
    _lib.check(lib.kfn_kalman_scan_scratch_bytes(C.byref(d), C.byref(need)), 'scratch bytes')
    scratch = torch.zeros(need.value // 4 + 4, device='cuda') if need.value else None
    fd, sd, md = dev(flow.astype(np.float32)), dev(st.astype(np.float32)), dev(meas.astype(np.float32))
    state = torch.zeros(S * h * w * 4, device='cuda')
    rec, temp, kf = (torch.zeros(S * T * h * w * 4, device='cuda') for _ in range(3))
    _lib.check(lib.kfn_kalman_scan_ex(C.byref(d), fd.data_ptr(), sd.data_ptr(), md.data_ptr(), state.data_ptr(), rec.data_ptr(),
                                      temp.data_ptr(), None, kf.data_ptr(), 0, scratch.data_ptr() if scratch is not None else None,
                                      stream()), 'kfn_kalman_scan_ex')
    sync()
    return temp.cpu().numpy().reshape(meas.shape), kf.cpu().numpy().reshape(meas.shape)


def run_backward(pred, flow, st, d_temp, d_kf, radius=4, ld_dpred=16):
    """pred [S,T,h,w,4] raw.  The measurement map, the scan and kfn_filter_backward from a zeroed dpred.  Returns (dpred
    [S,T,h,w,4], total d_kf, count, temp, kf)."""
    import torch
    lib = _lib.load()
    S, T, h, w, _ = pred.shape
    P = S * T * h * w
    G = 64
    pd = dev(pred.astype(np.float32))
    meas = torch.full((P + G, 4), -7.0, device='cuda')
    _lib.check(lib.kfn_measurement_map(pd.data_ptr(), 4, meas.data_ptr(), P, stream()), 'kfn_measurement_map')
    sync()
    mh = meas.cpu().numpy()
    assert np.all(mh[P:] == -7.0), 'the measurement map wrote past its pixels'
    mh = mh[:P].reshape(pred.shape)
    assert np.array_equal(mh[..., :3], pred[..., :3].astype(np.float32))
    temp, kf = run_scan(flow, st, mh)
    bd = _lib.FilterBackwardDesc(S=S, T=T, H=h, W=w, ld_dpred=ld_dpred, radius=radius, min_uncertainty=EPS)
    nb = C.c_size_t()
    _lib.check(lib.kfn_filter_backward_scratch_bytes(C.byref(bd), C.byref(nb)), 'scratch bytes')
    scratch = torch.full((nb.value // 4 + G,), -9.0, device='cuda')
    dp = torch.zeros((P + G, ld_dpred), device='cuda')
    dp[:, 4:] = -5.0
    dp[P:] = -5.0
    dk = torch.full((P + G, 4), -3.0, device='cuda')
    dk[:P] = dev(d_kf.astype(np.float32).reshape(P, 4))
    stats = torch.full((16,), -1.0, device='cuda')
    fd, td, kd, dtd = dev(flow.astype(np.float32)), dev(temp), dev(kf), dev(d_temp.astype(np.float32))
    _lib.check(lib.kfn_filter_backward(C.byref(bd), fd.data_ptr(), meas.data_ptr(), td.data_ptr(), kd.data_ptr(), dtd.data_ptr(),
                                       dk.data_ptr(), dp.data_ptr(), stats.data_ptr(), scratch.data_ptr(), stream()),
               'kfn_filter_backward')
    sync()
    dph, dkh, sh = dp.cpu().numpy(), dk.cpu().numpy(), stats.cpu().numpy()
    assert np.all(dph[:, 4:] == -5.0) and np.all(dph[P:] == -5.0), 'wrote outside the four gradient channels'
    assert np.all(dkh[P:] == -3.0) and np.all(scratch.cpu().numpy()[-G:] == -9.0), 'wrote past d_kf or the scratch buffer'
    assert np.all(np.delete(sh, 11) == -1.0), 'the reverse scan owns word 11 of stats alone'
    return dph[:P, :4].reshape(pred.shape), dkh[:P].reshape(pred.shape), int(sh.view(np.uint32)[11]), temp, kf


def ref_backward(pred, flow, st, d_temp, d_kf, dtype):
    """d/dpred of sum(d_temp temp + d_kf kf) through KR.filter_forward, and the forward maps, in `dtype`."""
    import torch
    p = torch.from_numpy(pred.astype(np.float64)).to(dtype).requires_grad_(True)
    temp, kf = KR.filter_forward(KR.measurement(p), flow, st)
    obj = (temp * torch.from_numpy(d_temp.astype(np.float64)).to(dtype)).sum() + \
          (kf * torch.from_numpy(d_kf.astype(np.float64)).to(dtype)).sum()
    g, = torch.autograd.grad(obj, [p])
    return g.to(torch.float64).numpy(), temp.detach().to(torch.float64).numpy(), kf.detach().to(torch.float64).numpy()


def backward_inputs(S, T, h, w, reach=4.0, seed=0):
    """Measurements and sigmas over two decades, flows uniform in [-reach, reach]: border cells sample outside the image
    and several targets share a source."""
    rng = np.random.default_rng([seed, S, T, h, w])
    pred = rng.normal(size=(S, T, h, w, 4)).astype(np.float32)
    pred[..., 3] = np.log(10.0 ** rng.uniform(-2, 0, size=(S, T, h, w)))
    flow = rng.uniform(-reach, reach, size=(S, T, h, w, 2)).astype(np.float32)
    st = (10.0 ** rng.uniform(-3, -1, size=(S, T, h, w))).astype(np.float32)
    d_temp = (rng.normal(size=(S, T, h, w, 4)) * 10.0 ** rng.uniform(-2, 0, size=(S, T, h, w, 1))).astype(np.float32)
    d_kf = (rng.normal(size=(S, T, h, w, 4)) * 10.0 ** rng.uniform(-2, 0, size=(S, T, h, w, 1))).astype(np.float32)
    return pred, flow, st, d_temp, d_kf


def assert_clear_of_the_gates(pred, flow, st):
    """No pixel within 1e-3 relative of a gate of the filter: s_l^2 = eps^2 (s_l recovered from the fp64 forward) and 1 - K = 0."""
    import torch
    p = torch.from_numpy(pred.astype(np.float64))
    meas = KR.measurement(p)
    temp, kf = KR.filter_forward(meas, flow, st)
    S, T = pred.shape[:2]
    pm = KR.pixel_map(pred.shape[2], pred.shape[3], torch.float64)
    fl = torch.from_numpy(flow.astype(np.float64))
    for t in range(1, T):
        s_l = KR.sampler(kf[:, t - 1], pm + fl[:, t])[..., 3].numpy()
        assert not np.any(np.abs(s_l / EPS - 1.0) < GATE_MARGIN)
        lv, mv = temp[:, t, ..., 3].numpy() ** 2, meas[:, t, ..., 3].numpy() ** 2
        assert np.all(mv / (lv + mv) > GATE_MARGIN * 1e-3)           # 1 - K: far from 0 on fp32's scale


# -- 1. the forward identity ------------------------------------------------------------------------------------------------------
def _flow_weights(seed=1234):
    from kfnet_amd.weights import synthetic_weights
    return {k: v for k, v in synthetic_weights(seed, init='he').items() if k.startswith('Temporal/')}


def _weights(seed=2):
    from kfnet_amd.weights import initial_weights
    W = initial_weights(seed)
    W.update(_flow_weights())
    return W


def _data(size, count, seed=1):
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    from kfnet_amd.train import synthetic_labels
    return (synthetic_sequence(count, size[0], size[1], seed=seed), synthetic_labels(count, (size[0] // 8, size[1] // 8)),
            synthetic_transform().astype(np.float32))


@pytest.mark.parametrize('size', [(40, 56), (72, 104)], ids=['5x7', '9x13'])
def test_trainer_forward_is_the_eval_scan_bit_for_bit(size):
    from kfnet_amd.train_kfnet import KFNetTrainer
    frames, labels, M = _data(size, 8)
    tr = KFNetTrainer(_weights(), image_size=size, groups=2, transform=M)
    import torch
    main = torch.cuda.current_stream()
    tr.sc.stage(frames, labels, None, main.cuda_stream)
    tr.flow(main)
    tr.forward()
    sync()
    h, w = size[0] // 8, size[1] // 8
    meas = tr.meas.cpu().numpy().reshape(2, 4, h, w, 4)
    pred = tr.sc.act[-1].cpu().numpy().reshape(2, 4, h, w, 4)
    assert np.array_equal(meas[..., :3], pred[..., :3]) and np.all(meas[..., 3] > 0)
    np.testing.assert_allclose(meas[..., 3], np.exp(pred[..., 3].astype(np.float64)), rtol=1e-6)
    dbg = tr.engine.debug(8)
    flow, st = dbg['flow'].reshape(2, 4, h, w, 2), dbg['sigma_trans'].reshape(2, 4, h, w)
    assert np.abs(flow[:, 1:]).max() > 0.05, 'the seeded OFlowNet must move something'
    temp, kf = run_scan(flow, st, meas)
    got_t, got_k = tr.temp.cpu().numpy().reshape(meas.shape), tr.kf.cpu().numpy().reshape(meas.shape)
    assert np.array_equal(got_t.view(np.uint32), temp.view(np.uint32)) and np.array_equal(got_k.view(np.uint32), kf.view(np.uint32))
    assert np.array_equal(got_t[:, 0], meas[:, 0]) and np.array_equal(got_k[:, 0], meas[:, 0])
    assert not np.array_equal(got_k[:, 1], meas[:, 1])
    # and the reference's filter says the same
    import torch
    rt, rk = KR.filter_forward(torch.from_numpy(meas.astype(np.float64)), flow, st)
    np.testing.assert_allclose(got_t, rt.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(got_k, rk.numpy(), rtol=1e-4, atol=1e-4)


# -- 2. the reverse scan ----------------------------------------------------------------------------------------------------------
BACKWARD_CASES = [(2, 4, 5, 7, 4, 4.0), (2, 4, 9, 13, 4, 4.0), (2, 2, 9, 13, 4, 4.0), (2, 4, 9, 13, 7, 7.0),
                  (1, 4, 60, 80, 4, 4.0), (1, 3, 90, 120, 4, 4.0)]        # the last: above 10 240 cells, the scan's per-frame path


@pytest.mark.parametrize('case', BACKWARD_CASES, ids=['S%d-T%d-%dx%d-r%d' % c[:5] for c in BACKWARD_CASES])
def test_filter_backward_against_fp64_autograd(case):
    import torch
    S, T, h, w, radius, reach = case
    pred, flow, st, d_temp, d_kf = backward_inputs(S, T, h, w, reach)
    assert_clear_of_the_gates(pred, flow, st)
    g, dk, count, temp, kf = run_backward(pred, flow, st, d_temp, d_kf, radius)
    assert count == 0
    g64, t64, k64 = ref_backward(pred, flow, st, d_temp, d_kf, torch.float64)
    g32, _, _ = ref_backward(pred, flow, st, d_temp, d_kf, torch.float32)
    # (the forward is the eval scan's: a sanity check only.  A sample outside the image has weights up to (radius + 1)^2 on
    #  coordinates of a few units, so its fp32 sum carries an absolute error of some 1e-5)
    np.testing.assert_allclose(temp, t64, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(kf, k64, rtol=1e-4, atol=1e-4)
    for name, sl in (('coordinates', slice(0, 3)), ('log sigma', slice(3, 4))):
        e, e32 = rel_err(g[..., sl], g64[..., sl]), rel_err(g32[..., sl], g64[..., sl])
        print('backward %s %s: e device %.3e, e torch-fp32 %.3e, bound %.3e' % (case, name, e, e32, bound(e32)))
        assert e <= bound(e32), (name, e, e32)
    # every frame but the last receives gradient through the sampler
    assert np.abs(dk[:, :-1] - d_kf[:, :-1]).max() > 0 and np.array_equal(dk[:, -1], d_kf[:, -1])
    # bit-identical from launch to launch
    g2, dk2, _, _, _ = run_backward(pred, flow, st, d_temp, d_kf, radius)
    assert np.array_equal(g.view(np.uint32), g2.view(np.uint32)) and np.array_equal(dk.view(np.uint32), dk2.view(np.uint32))


def test_filter_backward_gives_exact_zeros_below_the_floors():
    S, T, h, w = 2, 4, 9, 13
    pred, flow, st, d_temp, d_kf = backward_inputs(S, T, h, w, seed=3)
    # sequence 0, frame 0: sigma_z = 1e-7 everywhere, so every s_l of frame 1 lies below the variance floor: no gradient reaches
    # KF_0's sigma through the sampler.  Sequence 0, frame 2: sigma_z = 1e-9, so K rounds to 1 and max(1 - K, 0) is closed: with
    # d_temp = 0 there nothing reaches KF_1's coordinates, and the measurement takes d_kf as it is.
    pred[0, 0, ..., 3] = np.log(1e-7)
    pred[0, 2, ..., 3] = np.log(1e-9)
    d_temp[0, 2] = 0.0
    g, dk, count, temp, kf = run_backward(pred, flow, st, d_temp, d_kf)
    assert count == 0
    assert np.all(kf[0, 0, ..., 3] < 2e-7) and np.all(kf[0, 2, ..., 3] == 0.0)
    assert np.array_equal(dk[0, 0, ..., 3], d_kf[0, 0, ..., 3])
    assert not np.array_equal(dk[0, 0, ..., :3], d_kf[0, 0, ..., :3])
    assert np.array_equal(dk[0, 1, ..., :3], d_kf[0, 1, ..., :3])
    assert np.array_equal(g[0, 2, ..., :3], dk[0, 2, ..., :3])
    # the other sequence has neither region
    assert np.any(dk[1, 0, ..., 3] != d_kf[1, 0, ..., 3])
    assert np.any(dk[1, 1, ..., :3] != d_kf[1, 1, ..., :3])
    assert np.isfinite(g).all() and np.isfinite(dk).all()


def test_a_flow_beyond_the_radius_sets_the_counter_and_the_trainer_raises():
    pred, flow, st, d_temp, d_kf = backward_inputs(2, 4, 5, 7, seed=4)
    flow[1, 2, 3, 4, 0] = 4.5
    flow[0, 3, 0, 0, 1] = -4.5
    flow[0, 0, 1, 1, 0] = 9.0                       # frame 0 has no predecessor: not read
    assert run_backward(pred, flow, st, d_temp, d_kf)[2] == 2
    assert run_backward(pred, flow, st, d_temp, d_kf, radius=5)[2] == 0
    from kfnet_amd.train_kfnet import KFNetTrainer
    frames, labels, M = _data(SIZE, 4)
    tr = KFNetTrainer(_weights(), image_size=SIZE, transform=M)
    before = tr.weights()
    launch = tr.flow

    def flow_with_an_outlier(main):
        launch(main)
        main.wait_event(tr.ev_flow)
        tr.engine._view(tr.engine.c_flow, 4)[2, 3, 4, 0] = 4.5
        tr.ev_flow.record(main)
    tr.flow = flow_with_an_outlier
    with pytest.raises(_lib.KfnError, match='beyond the radius'):
        tr.step(frames, labels)
    sync()
    after = tr.weights()
    assert tr.global_step == 0 and all(np.array_equal(before[k], after[k]) for k in before)
    tr.flow = launch
    assert np.isfinite(tr.step(frames, labels)['loss']) and tr.global_step == 1


# -- 3. the loss ------------------------------------------------------------------------------------------------------------------
def run_filter_loss(pred, temp, kf, labels, frames, M, clip, sw, weights=KR.LOSS_WEIGHTS, ld_pred=4, ld_dpred=16):
    import torch
    lib = _lib.load()
    B, h, w, _ = pred.shape
    P = B * h * w
    G = 64
    pb = np.full((P, ld_pred), 3.0, np.float32)
    pb[:, :4] = pred.reshape(-1, 4)
    d = _lib.FilterLossDesc(B=B, h=h, w=w, ld_pred=ld_pred, ld_dpred=ld_dpred, label_stride=labels.shape[1] // h,
                            img_stride=frames.shape[1] // h, has_transform=int(M is not None), has_loss_clip=int(clip is not None),
                            loss_clip=clip or 0.0, smooth_weight=sw, weight_measure=weights[0], weight_temporal=weights[1],
                            weight_kf=weights[2], dist_threshold=0.05, min_uncertainty=EPS)
    if M is not None:
        d.transform = (C.c_float * 12)(*[float(v) for v in np.asarray(M, np.float32)[:3].reshape(-1)])
    g = torch.full((P, ld_dpred), -5.0, device='cuda')
    gt, gk = torch.full((P + G, 4), -5.0, device='cuda'), torch.full((P + G, 4), -5.0, device='cuda')
    st = torch.full((16,), -1.0, device='cuda')
    pd, td, kd = dev(pb), dev(temp.astype(np.float32)), dev(kf.astype(np.float32))
    ld, fd = dev(labels.astype(np.float32)), dev(frames)
    _lib.check(lib.kfn_filter_loss_grad(C.byref(d), pd.data_ptr(), td.data_ptr(), kd.data_ptr(), ld.data_ptr(), fd.data_ptr(),
                                        g.data_ptr(), gt.data_ptr(), gk.data_ptr(), st.data_ptr(), stream()), 'kfn_filter_loss_grad')
    sync()
    gh, gth, gkh, sh = g.cpu().numpy(), gt.cpu().numpy(), gk.cpu().numpy(), st.cpu().numpy()
    assert np.all(gh[:, 4:] == -5.0), 'the loss wrote outside its four gradient channels'
    assert np.all(gth[P:] == -5.0) and np.all(gkh[P:] == -5.0), 'the loss wrote past d_temp or d_kf'
    assert sh[11] == -1.0 and sh[15] == 0.0
    return sh, gh[:, :4].reshape(pred.shape), gth[:P].reshape(pred.shape), gkh[:P].reshape(pred.shape)


def filter_maps(pred, seed, shift=0.05):
    """Temporal and KF maps beside a raw prediction: its coordinates moved by a few centimetres, sigmas over two decades."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        m = pred.copy()
        m[..., :3] += (shift * rng.normal(size=pred.shape[:3] + (3,))).astype(np.float32)
        m[..., 3] = 10.0 ** rng.uniform(-2, 0, size=pred.shape[:3])
        out.append(m)
    return out


def ref_filter_loss(pred, temp, kf, labels, frames, M, clip, sw, weights, dtype):
    import torch
    B, h, w, _ = pred.shape
    leaves = [torch.from_numpy(a.astype(np.float64)).to(dtype).requires_grad_(True) for a in (pred, temp, kf)]
    L, stats, _ = KR.filter_loss(leaves[0], leaves[1], leaves[2], R.grid_labels(labels, (h, w)),
                                 frames[:, ::8, ::8].astype(np.float64), M, clip, sw, weights)
    grads = torch.autograd.grad(L, leaves, allow_unused=True)
    grads = [np.zeros(pred.shape) if g is None else g.to(torch.float64).numpy() for g in grads]
    return [float(s.detach()) for s in stats], grads


def check_filter_loss(pred, temp, kf, labels, frames, M, clip, sw, what, weights=KR.LOSS_WEIGHTS):
    import torch
    for m in (pred, temp, kf):              # the fp64 reference alone decides the three accuracy counts
        G1._assert_clear_of_the_threshold(m, labels, M)
    for m in (temp, kf):
        assert not np.any(np.abs(m[..., 3] / EPS - 1.0) < GATE_MARGIN)
    sh, g, gt, gk = run_filter_loss(pred, temp, kf, labels, frames, M, clip, sw, weights)
    s64, g64 = ref_filter_loss(pred, temp, kf, labels, frames, M, clip, sw, weights, torch.float64)
    s32, g32 = ref_filter_loss(pred, temp, kf, labels, frames, M, clip, sw, weights, torch.float32)
    names = ('L', 'NLL m', 'NLL t', 'NLL KF', 'smooth m', 'smooth t', 'smooth KF', 'acc m', 'acc t', 'acc KF', 'valid')
    for i, name in enumerate(names):
        e32 = abs(s32[i] - s64[i])
        print('%s %s: device %.9g fp64 %.9g torch-fp32 %.9g' % (what, name, sh[i], s64[i], s32[i]))
        if name.startswith('acc') or name == 'valid':
            assert sh[i] == np.float32(s64[i]), (what, name)
        else:
            assert abs(sh[i] - s64[i]) <= max(8.0 * e32, 1e-6 * abs(s64[i])) + 1e-12, (what, name)
    for name, got, want, w32 in zip(('dpred', 'd_temp', 'd_kf'), (g, gt, gk), g64, g32):
        if not np.any(want):
            assert not np.any(got), (what, name)
            continue
        e, e32 = rel_err(got, want), rel_err(w32, want)
        print('%s %s: e device %.3e, e torch-fp32 %.3e, bound %.3e' % (what, name, e, e32, bound(e32)))
        assert e <= bound(e32), (what, name, e, e32)
    return sh, (g, gt, gk), g64


LOSS_GRIDS = [(8, 8, 12), (8, 17, 23)]            # B = 2 x 4 frames: one pass of the 1024-thread loop, and 3128 pixels in four


@pytest.mark.parametrize('grid', LOSS_GRIDS, ids=['%dx%dx%d' % g for g in LOSS_GRIDS])
def test_filter_loss_and_gradients_against_fp64_autograd(grid):
    B, h, w = grid
    for full_res, with_M, sw in ((False, True, 50.0), (True, True, 50.0), (False, False, 50.0), (True, False, 0.0)):
        pred, labels, frames, M = G1._loss_inputs(300 + h + int(full_res), B=B, h=h, w=w, full_res=full_res)
        G1._flatten_upper_half(frames)
        temp, kf = filter_maps(pred, 7 + h)
        check_filter_loss(pred, temp, kf, labels, frames, M if with_M else None, None, sw,
                          '%dx%dx%d labels %s%s smooth %g' % (B, h, w, 'full' if full_res else 'grid', ' M' if with_M else '', sw))


def test_filter_loss_with_weights_1_0_0_is_the_stage_1_loss_bit_for_bit():
    for grid in LOSS_GRIDS:
        B, h, w = grid
        pred, labels, frames, M = G1._loss_inputs(310 + h, B=B, h=h, w=w)
        G1._flatten_upper_half(frames)
        temp, kf = filter_maps(pred, 8)
        for clip in (None, -2.0):
            want_s, want_g = G1.run_loss(pred, labels, frames, M, clip, 50.0)
            sh, g, gt, gk = run_filter_loss(pred, temp, kf, labels, frames, M, clip, 50.0, weights=(1.0, 0.0, 0.0))
            assert np.array_equal(g.view(np.uint32), want_g.view(np.uint32))
            got = np.array([sh[1], sh[4], sh[7], sh[10], sh[0]], np.float32)
            assert np.array_equal(got.view(np.uint32), want_s[:5].view(np.uint32)), (got, want_s)
            assert sh[12] == sh[0] and not gt.any() and not gk.any()


def test_filter_loss_clip_with_both_branches_an_empty_mask_and_the_sigma_floor():
    pred, labels, frames, M, l, m = G1._clip_inputs(3)
    # the filter's maps carry the prediction's own coordinates and sigma: the same loss map on both sides of the clip
    maps = pred.copy()
    maps[..., 3] = np.exp(pred[..., 3].astype(np.float64))
    _, (g, gt, gk), g64 = check_filter_loss(pred, maps, maps.copy(), labels, frames, M, -2.0, 50.0, 'loss_clip -2 with smoothness')
    _, (g, gt, gk), g64 = check_filter_loss(pred, maps, maps.copy(), labels, frames, M, -2.0, 0.0, 'loss_clip -2')
    for got, want in zip((g, gt, gk), g64):
        assert np.all(want[(l > -2.0)] == 0.0) and np.any(want[(l < -2.0) & m] != 0.0)
        assert np.all(got[(l > -2.0)] == 0.0) and np.any(got[(l < -2.0) & m] != 0.0)
    # sigma below 1e-5 in a region of each filter map: u is the floor, exact zeros for sigma there
    pred, labels, frames, M = G1._loss_inputs(5)
    temp, kf = filter_maps(pred, 9)
    temp[0, 2:4, :, 3] = 2e-6
    kf[1, 5:7, :, 3] = 0.0
    _, (g, gt, gk), g64 = check_filter_loss(pred, temp, kf, labels, frames, M, None, 50.0, 'sigma below 1e-5')
    assert np.all(gt[0, 2:4, :, 3] == 0.0) and np.all(gk[1, 5:7, :, 3] == 0.0)
    assert np.all(g64[1][0, 2:4, :, 3] == 0.0) and np.any(gt[0, 2:4, :, :3] != 0.0)
    empty = labels.copy()
    empty[..., 3] = 0.0
    sh, (g, gt, gk), _ = check_filter_loss(pred, temp, kf, empty, frames, M, None, 50.0, 'all-zero mask')
    assert sh[10] == 1.0 and sh[0] == 0.0 and not g.any() and not gt.any() and not gk.any()
    assert np.all(sh[1:7] == 0.0) and np.all(sh[7:10] == 1.0)


def test_filter_loss_smoothness_does_not_reach_across_a_frame_seam():
    """G1._seam_inputs: rows 100 apart on both sides of every frame seam, edge weights of 1 there.  The filter maps carry the
    same coordinates, so a neighbour from across a seam would move each of the three gradients by more than 100 times
    1e-5 max|g64| (asserted on the host there); the comparison allows at most max(8 e32, 1e-6) max|g64|."""
    pred, labels, frames, M, tol = G1._seam_inputs()
    temp, kf = filter_maps(pred, 10, shift=0.0)
    _, (g, gt, gk), g64 = check_filter_loss(pred, temp, kf, labels, frames, M, None, 50.0, 'frame seam', weights=(1.0, 1.0, 1.0))
    assert 1e-5 * float(np.abs(g64[0]).max()) == pytest.approx(tol, rel=1e-9)
    for got, want in zip((g, gt, gk), g64):
        assert np.abs(got[..., :3] - want[..., :3]).max() <= 1e-5 * np.abs(want).max()


# -- 4. a whole step ----------------------------------------------------------------------------------------------------------------
def _engine_params(tr):
    return {k: p.storage.clone() for k, p in tr.engine.graph.params.items()}


@pytest.mark.parametrize('size', [(64, 96), (72, 104)], ids=['64x96', '72x104'])
def test_one_step_gradients_and_update_against_fp64(size):
    import torch
    from kfnet_amd.train_kfnet import KFNetTrainer
    frames, labels, M = _data(size, 4)
    W = _weights()
    tr = KFNetTrainer(W, image_size=size, transform=M, base_lr=1e-4, weight_decay=1e-4)
    flow_before = _engine_params(tr)
    stats = dict(tr.step(frames, labels))
    g = tr.gradients()
    dbg = tr.engine.debug(4)
    flow, st = dbg['flow'], dbg['sigma_trans']
    assert np.abs(flow[1:]).max() > 0.05 and np.abs(flow[1:]).max() <= 4.0
    s64, g64 = KR.loss_and_grads(frames, labels, W, 1, 4, flow, st, M)
    s32, g32 = KR.loss_and_grads(frames, labels, W, 1, 4, flow, st, M, dtype=torch.float32)
    for k in ('loss', 'l_measure', 'l_temp', 'l_KF', 'a_measure', 'a_temp', 'a_KF', 'pixels'):
        print('%-10s device %.7g torch-fp32 %.7g fp64 %.7g' % (k, stats[k], s32[k], s64[k]))
    assert abs(stats['loss'] - s64['loss']) <= 1e-4 * abs(s64['loss'])
    assert stats['pixels'] == float((labels[..., 3] == 1.0).sum()) and stats['lr'] == 1e-4
    e_dev, e_32 = {}, {}
    for name in sorted(g64):
        scale = np.abs(g64[name]).max()
        e_dev[name] = float(np.abs(g[name] - g64[name]).max() / scale)
        e_32[name] = float(np.abs(g32[name] - g64[name]).max() / scale)
        print('%-28s e device %.3e  e torch-fp32 %.3e' % (name, e_dev[name], e_32[name]))
    worst_dev, worst_32 = max(e_dev.values()), max(e_32.values())
    print('worst e: device %.3e, torch-CPU fp32 %.3e, bound %.3e' % (worst_dev, worst_32, bound(worst_32)))
    assert worst_dev <= bound(worst_32)
    # the filter matters: the gradients differ from the measurement term's alone
    _, gm = R.loss_and_grads(frames, labels, W, M)
    assert np.abs(g64['ScoreNet/prediction/kernel'] - 0.2 * gm['ScoreNet/prediction/kernel']).max() > \
        1e-3 * np.abs(g64['ScoreNet/prediction/kernel']).max()
    # the update: numpy Adam on the device's own gradients, bit for bit
    after, st_ = tr.weights(), tr.state()
    assert int(st_['global_step']) == 1 and int(st_['adam_t']) == 1
    for name in sorted(g):
        z = np.zeros_like(W[name])
        w1, m1, v1 = R.adam_step(W[name], z, z, g[name], 1e-4, 1, 1e-4)
        for what, got, want in (('w', after[name], w1), ('m', st_['adam_m/' + name], m1), ('v', st_['adam_v/' + name], v1)):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, what, float(R.ulp_distance(got, want).max()))
    # Temporal/* after three steps: handed through, and untouched on the device
    tr.step(frames, labels)
    tr.step(frames, labels)
    sync()
    out = tr.weights()
    assert sorted(out) == sorted(W)
    for k in W:
        if k.startswith('Temporal/'):
            assert np.array_equal(out[k].view(np.uint32), W[k].view(np.uint32)), k
    for k, p in tr.engine.graph.params.items():
        assert torch.equal(p.storage, flow_before[k]), k


# -- 5. run-level properties ----------------------------------------------------------------------------------------------------------
def _run_steps(tr, frames, labels, groups, first, count):
    from kfnet_amd.train_kfnet import group_indices
    for s in range(first, first + count):
        idx = group_indices(s, 1, groups)
        tr.step(frames[idx], labels[idx])


def test_runs_are_bit_identical_and_resume_from_snapshot_files(tmp_path):
    from kfnet_amd.train_kfnet import KFNetTrainer, group_list, restore
    frames, labels, M = _data(SIZE, 6)
    groups = group_list(6, 1000)
    W = _weights()
    kw = dict(image_size=SIZE, transform=M, base_lr=1e-3, stepvalue=3)
    runs = []
    for _ in range(2):
        tr = KFNetTrainer(W, **kw)
        _run_steps(tr, frames, labels, groups, 0, 5)
        runs.append(tr.weights())
    for k in W:
        assert np.array_equal(runs[0][k].view(np.uint32), runs[1][k].view(np.uint32)), k
        assert k.startswith('Temporal/') or not np.array_equal(runs[0][k], W[k]), k
    tr = KFNetTrainer(W, **kw)
    _run_steps(tr, frames, labels, groups, 0, 2)
    wp, sp = tr.save(str(tmp_path))
    assert os.path.basename(wp) == 'kfnet_weights-2.npz' and os.path.basename(sp) == 'kfnet_train_state-2.npz'
    del tr
    W2, state, step = restore(str(tmp_path), verbose=False)
    assert step == 2 and state is not None and sorted(W2) == sorted(W)
    tr = KFNetTrainer(W2, **kw)
    tr.load_state(state)
    tr.global_step = step
    assert tr.global_step == 2 and tr.adam_t == 2
    _run_steps(tr, frames, labels, groups, 2, 3)
    resumed = tr.weights()
    for k in W:
        assert np.array_equal(resumed[k].view(np.uint32), runs[0][k].view(np.uint32)), k


def test_a_reversed_group_gives_the_loss_of_the_reference_on_the_reversed_frames():
    from kfnet_amd.train_kfnet import KFNetTrainer
    frames, labels, M = _data(SIZE, 4)
    W = _weights()
    tr = KFNetTrainer(W, image_size=SIZE, transform=M)
    losses = {}
    for name, idx in (('forward', [0, 1, 2, 3]), ('reversed', [3, 2, 1, 0])):
        tr.sc.set_weights(W)
        s = dict(tr.step(frames[idx], labels[idx]))
        dbg = tr.engine.debug(4)
        ref, _ = KR.loss_and_grads(frames[idx], labels[idx], W, 1, 4, dbg['flow'], dbg['sigma_trans'], M)
        for k in ('loss', 'l_measure', 'l_temp', 'l_KF'):
            print('%s %-10s device %.7g fp64 %.7g' % (name, k, s[k], ref[k]))
            assert abs(s[k] - ref[k]) <= 1e-4 * abs(ref[k]), (name, k)
        losses[name] = s
    assert losses['forward']['l_measure'] == pytest.approx(losses['reversed']['l_measure'], rel=1e-5)
    assert losses['forward']['l_temp'] != losses['reversed']['l_temp']


# -- 6. the command line ----------------------------------------------------------------------------------------------------------
def _cli(module, args, timeout=900):
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT'):
        env.pop(k, None)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    r = subprocess.run([sys.executable, '-m', module] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_train_command_line_then_eval_reads_its_snapshot(tmp_path):
    from kfnet_amd.weights import initial_weights, load_npz, save_npz
    model, flownet, out = tmp_path / 'm', tmp_path / 'f', tmp_path / 'o'
    out.mkdir()
    flownet.mkdir()
    save_npz(str(flownet / 'kfnet_weights-7.npz'), _flow_weights())
    small = ['--height', '64', '--width', '96', '--scene', 'fire']
    log = _cli('kfnet_amd.KFNet.train', ['--model_folder', str(model), '--synthetic', '8', '--fix_flownet', '--oflownet', str(flownet),
                                         '--max_steps', '6', '--snapshot', '6', '--display', '2'] + small)
    assert sorted(os.listdir(str(model))) == ['kfnet_train_state-6.npz', 'kfnet_weights-6.npz']
    assert 'step 6/6' in log and 'l_temp=' in log and 'l_KF=' in log and 'Restore from scope Temporal' in log
    assert 'nothing restores ScoreNet' in log and 'current step:  0' in log
    saved = load_npz(str(model / 'kfnet_weights-6.npz'))
    flow_w, start = _flow_weights(), initial_weights(0)
    for k, v in flow_w.items():
        assert np.array_equal(saved[k].view(np.uint32), v.view(np.uint32)), k
    assert all(not np.array_equal(saved[k], start[k]) for k in start)
    _cli('kfnet_amd.KFNet.eval', ['--model_folder', str(model), '--synthetic', '4', '--output_folder', str(out)] + small)
    recs = [np.load(str(out / ('coord_%d.npy' % i))) for i in range(4)]
    assert all(r.shape == (8, 12, 4) and np.isfinite(r).all() for r in recs)
    # a second run resumes at step 6 and has nothing left to do
    log = _cli('kfnet_amd.KFNet.train', ['--model_folder', str(model), '--synthetic', '8', '--fix_flownet', '--max_steps', '6'] + small)
    assert 'current step:  6' in log and 'Adam slots restored' in log


# -- 7. learning --------------------------------------------------------------------------------------------------------------------
def test_ten_steps_on_one_group_lower_the_loss_like_the_fp64_run():
    from kfnet_amd.train import learning_rate
    from kfnet_amd.train_kfnet import KFNetTrainer
    frames, labels, M = _data(SIZE, 4)
    W = _weights()
    tr = KFNetTrainer(W, image_size=SIZE, transform=M, base_lr=1e-4, weight_decay=1e-4)
    dev_losses = [tr.step(frames, labels) for _ in range(11)]          # entry i = the loss after i updates
    dev_losses = [s['loss'] for s in dev_losses]
    dbg = tr.engine.debug(4)                                           # the same frames and a frozen OFlowNet: constants of the run
    flow, st = dbg['flow'], dbg['sigma_trans']
    ref = {k: v.copy() for k, v in W.items() if k.startswith('ScoreNet/')}
    m = {k: np.zeros_like(v) for k, v in ref.items()}
    v_ = {k: np.zeros_like(v) for k, v in ref.items()}
    ref_losses = []
    for t in range(1, 12):
        s, g = KR.loss_and_grads(frames, labels, ref, 1, 4, flow, st, M)
        ref_losses.append(s['loss'])
        lr = learning_rate(1e-4, 0.5, 80000, t - 1)
        for k in ref:
            ref[k], m[k], v_[k] = R.adam_step(ref[k], m[k], v_[k], g[k].astype(np.float32), lr, t, 1e-4)
    for i in (0, 1, 5, 10):
        print('after %2d updates: device L %.6f, fp64 run %.6f' % (i, dev_losses[i], ref_losses[i]))
    assert ref_losses[10] < ref_losses[0] and dev_losses[10] < dev_losses[0]
    assert abs(dev_losses[0] - ref_losses[0]) <= 1e-4 * abs(ref_losses[0])
    assert abs(dev_losses[10] - ref_losses[10]) <= 0.05 * abs(ref_losses[10])
