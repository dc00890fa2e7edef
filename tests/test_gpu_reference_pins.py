"""The HIP path against the reference's OWN model code: tests/golden/ref_kfnet_small.npz and ref_train_small.npz, written by
oracle/run_reference.py from the reference's modules over the stand-in of oracle/tf_standin (tests/test_reference_pins.py holds
the restatements to the same files).  Only fixtures are read here.

The engine is held to the bounds tests/test_golden.py uses against kfnet_small.npz.  Losses, backward kernels and whole steps
are held to the project's rule: e = max|g - g64| / max|g64| <= max(8 e_fp32, 1e-6), where e_fp32 is the error of
the REFERENCE's float32 run against its fp64 run, both stored in the fixture."""
import hashlib
import os

import numpy as np
import pytest

import test_gpu_joint_train as J3
import test_gpu_kfnet_train as K3
import test_gpu_reproj as P9
import test_gpu_train as G1
from oracle import run_reference as RECIPE

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CLIP, SMOOTH = -2.0, 50.0


def bound(e32):
    return max(8.0 * e32, 1e-6)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    s = np.abs(b).max()
    return float(np.abs(a - b).max() / s) if s > 0 else float(np.abs(a).max())


def passes(what, got, want64, e32):
    e = rel(got, want64)
    print('%-44s e device %.3e   e reference-fp32 %.3e   bound %.3e' % (what, e, e32, bound(e32)))
    assert e <= bound(e32), (what, e, e32)


# ---- the engine ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ev():
    from kfnet_amd.weights import synthetic_weights
    z = np.load(os.path.join(GOLD, 'ref_kfnet_small.npz'))
    W = synthetic_weights(int(z['seed_w']))
    assert RECIPE.weights_digest(W) == str(z['weights_sha256']), 'synthetic weight generator drifted'
    return z, W


def _close(rec, ref, tol=1e-4):
    assert np.abs(rec[..., :3] - ref[..., :3]).max() <= tol
    assert (np.abs(rec[..., 3] - ref[..., 3]) / np.abs(ref[..., 3])).max() <= tol


@pytest.mark.parametrize('nis', [False, True])
def test_hip_engine_reproduces_the_reference_run(ev, nis):
    from kfnet_amd.engine import KFNetEngine
    z, W = ev
    eng = KFNetEngine(W, image_size=(64, 96), batch=2, transform=z['transform'], reset_period=int(z['reset_period']),
                      nis_gate=7.815 if nis else 0.0, max_chunk=8, emit_debug=True)
    rec = eng.process(eng.upload_frames(z['images'])).cpu().numpy()
    _close(rec, z['records_nis'] if nis else z['records'])
    d = eng.debug(5)
    assert np.abs(d['meas'][1][..., :3] - z['z1'][0]).max() < 5e-5
    assert np.abs(d['flow'][1] - z['flow1'][0]).max() < 5e-5
    assert np.abs(d['temp'][1][..., :3] - z['temp_x1'][0]).max() < 5e-5
    assert np.allclose(d['temp'][1][..., 3:4], z['temp_s1'][0], rtol=1e-4)


def test_hip_feature_tower_reproduces_the_reference_run(ev):
    from kfnet_amd.engine import KFNetEngine
    z, W = ev
    eng = KFNetEngine(W, image_size=(64, 96), batch=2, reset_period=500, max_chunk=4)
    eng.process(eng.upload_frames(z['images'][:2]))      # one full batch: frames 0, 1 -> ring slots 1, 2
    ring = eng.net.temp_feat_maps.numpy()
    assert np.abs(ring[1] - z['feat1'][0]).max() < 2e-5 and np.abs(ring[2] - z['feat1'][1]).max() < 2e-5


# ---- losses and backward kernels on the stored leaves ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tr():
    from kfnet_amd.synth import synthetic_sequence
    z = np.load(os.path.join(GOLD, 'ref_train_small.npz'))
    frames = synthetic_sequence(4, 64, 96, seed=int(z['train_seed']))
    assert hashlib.sha256(frames.tobytes()).hexdigest() == str(z['frames_sha256']), 'synthetic frame generator drifted'
    assert float(z['e_fp32_worst']) <= 1e-3
    return z, frames, z['matrix'].astype(np.float32)


def scalar_passes(what, got, z, key):
    want, w32 = float(z['one64:' + key]), float(z['one32:' + key])
    e, e32 = abs(got - want) / abs(want), abs(np.float32(w32) - want) / abs(want)
    print('%-44s device %.9g reference %.9g   e %.3e   e reference-fp32 %.3e' % (what, got, want, e, e32))
    assert e <= bound(e32), (what, e, e32)


def test_coord_loss_grad_against_measure_coord_loss(tr):
    z, frames, M = tr
    st, g = G1.run_loss(z['pred'], z['labels1'], frames, M, CLIP, SMOOTH)
    scalar_passes('kfn_coord_loss_grad L', float(st[4]), z, 'l_measure')
    assert st[2] == np.float32(z['one64:a_measure']) and st[3] == float(z['one64:valid']) + 1.0
    passes('kfn_coord_loss_grad dpred', g, z['one64:d_pred_measure'], rel(z['one32:d_pred_measure'], z['one64:d_pred_measure']))
    # the grid-sized frames (img_stride 1) are the same pixels
    st1, g1 = G1.run_loss(z['pred'], z['labels1'], z['frames_grid'], M, CLIP, SMOOTH)
    assert np.array_equal(g1, g) and np.array_equal(st1, st)


def test_scan_filter_loss_and_joint_backward_against_the_reference(tr):
    """kfn_measurement_map + kfn_kalman_scan_ex, kfn_filter_loss_grad on the device's own maps, kfn_filter_backward_joint on
    the device's own d_temp and d_kf: the chain the joint trainer runs, from the leaves to d_pred, d_flow and d_sigma_trans."""
    z, frames, M = tr
    B, h, w, _ = z['pred'].shape
    pred = z['pred'][None]                                                                       # one group of four
    flow = np.concatenate([np.zeros((1, h, w, 2)), z['one64:flow']])[None].astype(np.float32)
    st = np.concatenate([np.zeros((1, h, w)), z['sigma_trans'].astype(np.float64).reshape(B - 1, h, w)])[None].astype(np.float32)
    meas = np.concatenate([pred[..., :3], np.exp(pred[..., 3:4].astype(np.float64))], -1).astype(np.float32)
    temp, kf = K3.run_scan(flow, st, meas)
    passes('scan temp', temp[0], z['one64:temp'], float(z['one_e:temp']))
    passes('scan kf', kf[0], z['one64:kf'], float(z['one_e:kf']))
    sh, g, gt, gk = K3.run_filter_loss(pred[0], temp[0], kf[0], z['labels1'], frames, M, CLIP, SMOOTH)
    scalar_passes('kfn_filter_loss_grad L', float(sh[0]), z, 'loss')
    for i, key in enumerate(('l_measure', 'l_temp', 'l_KF')):
        scalar_passes('kfn_filter_loss_grad ' + key, float(sh[1 + i]) + SMOOTH * float(sh[4 + i]), z, key)
        assert sh[7 + i] == np.float32(z['one64:a_' + key[2:]]), key
    assert sh[10] == float(z['one64:valid']) + 1.0
    dp, dk, count, df, ds = J3.run_joint(pred, flow, st, gt[None], gk[None])
    assert count == 0
    e32 = {k: rel(z['one32:' + k], z['one64:' + k]) for k in ('d_pred', 'd_flow', 'd_sigma_trans')}
    passes('chain d_pred', g + dp[0], z['one64:d_pred'], e32['d_pred'])
    passes('chain d_flow', df[0, 1:], z['one64:d_flow'], e32['d_flow'])
    passes('chain d_sigma_trans', ds[0, 1:], z['one64:d_sigma_trans'], e32['d_sigma_trans'])
    assert not df[0, 0].any() and not ds[0, 0].any()


def test_reproj_loss_grad_against_reprojection_loss(tr):
    from kfnet_amd.labels import DepthCamera
    z, frames, M = tr
    B, h, w, _ = z['pred'].shape
    fx, fy, u, v = (float(c) for c in z['camera'])
    x = np.ascontiguousarray(z['pred'][..., :3])
    poses = z['poses'][:, :3].reshape(B, 12).astype(np.float32)
    stats, dxs = P9.run_reproj([x], poses, z['labels1'], None, float(z['one64:valid']) + 1.0, [1.0], 4, 4, 1,
                               camera=DepthCamera(fx=fx, fy=fy, u=u, v=v))
    scalar_passes('kfn_reproj_loss_grad R', float(stats[0]), z, 'reproj')
    assert stats[4] == float(z['one64:valid']) + 2.0                       # valid_pixel + 1, taken twice
    passes('kfn_reproj_loss_grad dx', dxs[0][..., :3], z['one64:d_reproj'], rel(z['one32:d_reproj'], z['one64:d_reproj']))
    assert not dxs[0][z['labels1'][..., 3] != 1.0].any()


# ---- whole steps ------------------------------------------------------------------------------------------------------------------------
def check_step(z, stage, stats, g, scopes=('ScoreNet',)):
    pre = 's%d:' % stage
    ends = np.cumsum(z[pre + 'bias_sizes'])
    want = dict(zip((str(s) for s in z[pre + 'stats']), z[pre + 'stat_values']))
    e_stat = dict(zip((str(s) for s in z[pre + 'stats']), z[pre + 'e_stat']))
    e = abs(stats['loss'] - want['loss']) / abs(want['loss'])
    print('stage %d loss: device %.9g reference %.9g   e %.3e   bound %.3e' % (stage, stats['loss'], want['loss'], e,
                                                                             bound(e_stat['loss'])))
    assert e <= bound(e_stat['loss'])
    assert sorted(g) == sorted([str(n) for n in z[pre + 'biases']] + [str(n) for n in z[pre + 'kernels']])
    for scope in scopes:
        e_dev, e_32 = {}, {}
        for n, k, end, e32 in zip(z[pre + 'biases'], z[pre + 'bias_sizes'], ends, z[pre + 'e_bias']):
            n = str(n)
            if not n.startswith(scope + '/'):
                continue
            if n == RECIPE.ZERO_BY_SYMMETRY:
                assert np.abs(g[n]).max() <= 1e-6 * np.abs(g['Temporal/prediction/kernel']).max()
                continue
            e_dev[n], e_32[n] = rel(g[n], z[pre + 'bias_grads'][end - k:end]), float(e32)
        for n, norm, proj, en, ep in zip(z[pre + 'kernels'], z[pre + 'norms'], z[pre + 'projections'], z[pre + 'e_norm'],
                                         z[pre + 'e_projection']):
            n = str(n)
            if not n.startswith(scope + '/'):
                continue
            g64 = g[n].astype(np.float64)
            e_dev[n + ' norm'], e_32[n + ' norm'] = abs(np.sqrt((g64 * g64).sum()) / norm - 1.0), float(en)
            e_dev[n + ' projection'] = abs((g64 * RECIPE.projection_vector(n, g64.shape)).sum() - proj) / norm
            e_32[n + ' projection'] = float(ep)
        for n in sorted(e_dev):
            print('%-44s e device %.3e   e reference-fp32 %.3e' % (n, e_dev[n], e_32[n]))
        worst_dev, worst_32 = max(e_dev.values()), max(e_32.values())
        print('stage %d %s worst e: device %.3e, reference fp32 %.3e, bound %.3e' % (stage, scope, worst_dev, worst_32,
                                                                                    bound(worst_32)))
        assert worst_dev <= bound(worst_32), (stage, scope, worst_dev, worst_32)


def train_weights(z):
    W = RECIPE.train_weights()
    assert RECIPE.weights_digest(W) == str(z['weights_sha256']), 'initial weight generator drifted'
    return W


def test_one_stage_1_step_against_the_reference(tr):
    from kfnet_amd.train import SCoordNetTrainer
    z, frames, M = tr
    W = {k: v for k, v in train_weights(z).items() if k.startswith('ScoreNet/')}
    t = SCoordNetTrainer(W, image_size=(64, 96), batch=4, transform=M, base_lr=1e-4, weight_decay=1e-4, loss_clip=CLIP)
    stats = dict(t.step(frames, z['labels2']))
    assert stats['pixels'] == float((z['labels2'][..., 3] == 1.0).sum())
    check_step(z, 1, stats, t.gradients())


@pytest.fixture(scope='module')
def joint_step(tr):
    """One step of the joint trainer, shared by the two tests below and left unchanged."""
    from kfnet_amd.train_kfnet import KFNetTrainer
    z, frames, M = tr
    t = KFNetTrainer(train_weights(z), image_size=(64, 96), groups=1, transform=M, base_lr=1e-4, weight_decay=1e-4,
                     loss_clip=CLIP, train_flownet=True)
    stats = dict(t.step(frames, z['labels2']))
    return stats, t.gradients(), t.c_flow.cpu().numpy().reshape(1, 4, 8, 12, 2)


def test_one_joint_step_against_the_reference(tr, joint_step):
    """The flow, the loss, the three accuracy counts and every SCoordNet gradient of a joint step."""
    z, frames, M = tr
    stats, g, flow = joint_step
    passes('joint step flow', flow[0, 1:], z['s3:flow'], float(z['s3:e_flow']))
    assert not flow[0, 0].any()
    want = dict(zip((str(s) for s in z['s3:stats']), z['s3:stat_values']))
    for k in ('a_measure', 'a_temp', 'a_KF'):
        assert np.float32(stats[k]) == np.float32(want[k]), k
    check_step(z, 3, stats, g, ('ScoreNet',))


def test_one_joint_step_temporal_scope_against_the_reference(tr, joint_step):
    """OFlowNet's gradients of the same step, under the same rule.  Before the fixture's weights were moved clear of the ReLU
    kinks (oracle/run_reference.py find_nudges) this missed by three decades, worst e 1.3e-2 against a bound of 1.6e-5: ONE unit
    of conv6, 3.4e-8 from zero in fp64, was gated the other way by the device, and under the device's own gates every gradient
    agreed with fp64 autograd to 2.1e-6.  With the cleared weights: worst e 2.5e-6, bound 1.9e-5."""
    z, frames, M = tr
    stats, g, flow = joint_step
    check_step(z, 3, stats, g, ('Temporal',))
