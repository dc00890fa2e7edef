"""The restatements every other test leans on -- oracle/kfnet_oracle*.py, oracle/kfnet_metrics_oracle.py and tests/*_ref.py --
against the reference's OWN model code: tests/golden/ref_kfnet_small.npz and ref_train_small.npz, which oracle/run_reference.py
writes by importing the reference's modules over the eager stand-in of oracle/tf_standin.  Both sides run in fp64, so what may
differ is rounding, and each bound below is 100 times the deviation measured when the fixtures were made (floor 1e-13: another
BLAS may order its sums differently), never above 1e-8: above that the two would MEAN something different.

What stays unpinned: TensorFlow's own op semantics as the stand-in reads them (tests/test_tf_standin.py).

Where a reference checkout is present (KFN_REFERENCE, default /root/reference) the recipe runs again and must reproduce the
committed fixtures to 1e-12."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import flow_train_ref as FR
import joint_train_ref as JR
import kf_train_ref as KR
import reproj_ref as RR
import train_ref as R
from oracle import kfnet_metrics_oracle as MO
from oracle import kfnet_oracle as O
from oracle import kfnet_oracle_torch as OT
from oracle import run_reference as RECIPE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, 'golden')
CLIP, SMOOTH = -2.0, 50.0                 # KFNet/KFNet.py:217, KFNet/KFNet.py:252

# measured relative deviation (max |a - b| / max |b|) of each restatement from the fixture, fp64 against fp64; see CHANGELOG
MEASURED = {
    'eval z': 2.4e-15, 'eval sigma_z': 5.3e-16, 'eval feat': 1.6e-15, 'eval flow': 2.9e-15, 'eval prob': 3.6e-15,
    'eval temp_x': 2.5e-15, 'eval temp_s': 3.6e-16, 'eval kf_x': 1.8e-15, 'eval kf_s': 5.2e-16, 'eval nis': 3.0e-15,
    'eval records': 5.5e-16, 'eval records_nis': 0.0, 'eval kf2_x': 1.8e-15, 'eval kf2_s': 3.9e-16,
}


def bound(name):
    return min(max(100.0 * MEASURED[name], 1e-13), 1e-8)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    s = np.abs(b).max()
    return float(np.abs(a - b).max() / s) if s > 0 else float(np.abs(a).max())


SEEN = {}


def pin(name, got, want):
    e = rel(got, want)
    SEEN[name] = e
    print('%-28s deviation %.3e  bound %.1e' % (name, e, bound(name)))
    assert e <= bound(name), (name, e, bound(name))


# ---- the forward pass ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ev():
    from kfnet_amd.weights import synthetic_weights
    z = np.load(os.path.join(GOLD, 'ref_kfnet_small.npz'))
    W = synthetic_weights(int(z['seed_w']))
    assert RECIPE.weights_digest(W) == str(z['weights_sha256']), 'synthetic weight generator drifted'
    rec, dbg = O.eval_sequence(z['images'], W, z['transform'], reset_period=int(z['reset_period']), dtype=np.float64,
                               return_debug=True)
    return z, W, rec, dbg


def test_forward_fixture_has_the_inputs_of_kfnet_small():
    z, g = np.load(os.path.join(GOLD, 'ref_kfnet_small.npz')), np.load(os.path.join(GOLD, 'kfnet_small.npz'))
    assert np.array_equal(z['images'], g['images']) and np.array_equal(z['transform'], g['transform'])
    assert int(z['reset_period']) == int(g['reset_period']) == 4 and int(z['seed_w']) == int(g['seed_w']) == 1234
    assert z['records'].shape == (5, 8, 12, 4) and z['records'].dtype == np.float64
    assert any('eval.py:94-104' in r for r in z['restated']) and 'tf_standin' in str(z['source'])
    for name in ('ref_kfnet_small.npz', 'ref_train_small.npz'):
        assert os.path.getsize(os.path.join(GOLD, name)) <= os.path.getsize(os.path.join(GOLD, 'kfnet_full.npz'))


def test_oracle_stage_outputs_match_the_reference(ev):
    z, W, rec, dbg = ev
    d = dbg[1]
    for key, fix in (('z', 'z1'), ('feat', 'feat1'), ('flow', 'flow1'), ('prob', 'prob1'), ('temp_x', 'temp_x1'),
                     ('temp_s', 'temp_s1'), ('kf_x', 'kf_x1'), ('kf_s', 'kf_s1'), ('nis', 'nis1')):
        want = z[fix][-1:] if z[fix].shape[0] == 2 and fix != 'prob1' else z[fix]       # feat1 holds the pair: frame 1 is last
        pin('eval ' + key, d[key], want)
    pin('eval sigma_z', d['sz'], z['sz1'])
    assert np.abs(np.linalg.norm(z['feat1'], axis=-1) - 1.0).max() < 1e-12
    assert np.abs(z['prob1'].sum(-1) - 1.0).max() < 1e-12 and z['prob1'].shape == (96, 64)
    # the translate direction of the cost volume: the flow of the reference and of the oracle agree in SIGN cell by cell
    assert np.abs(z['flow1']).max() > 0.05 and np.array_equal(np.sign(d['flow']), np.sign(z['flow1']))


def test_oracle_records_match_the_reference(ev):
    z, W, rec, dbg = ev
    T = z['transform']
    # the oracle's records are rounded to float32; rebuild them in fp64 from its stage outputs for the tight comparison
    rec64 = []
    for i, d in enumerate(dbg):
        x, s = (d['z'], d['sz']) if i % int(z['reset_period']) == 0 else (d['kf_x'], d['kf_s'])
        rec64.append(np.concatenate([O.apply_transform(x, T)[0], 1.0 / s[0]], -1))
    pin('eval records', np.stack(rec64), z['records'])
    assert np.array_equal(rec, np.stack(rec64).astype(np.float32))
    assert np.array_equal(z['records'][0, ..., :3], O.apply_transform(dbg[0]['z'], T)[0]) or rel(
        z['records'][0, ..., :3], O.apply_transform(dbg[0]['z'], T)[0]) < 1e-13              # step 0 = pair (1, 0): frame 0
    rec_nis = O.eval_sequence(z['images'], W, T, reset_period=int(z['reset_period']), nis_gate=True, dtype=np.float64)
    pin('eval records_nis', rec_nis.astype(np.float64), z['records_nis'].astype(np.float32).astype(np.float64))
    gated = sum(int((d['nis'].sum(-1) > 7.815).sum()) for d in dbg if 'nis' in d)
    assert gated == int(z['gated_cells'])
    # the fp32 restatements against the fp64 reference, under tests/test_golden.py's bound for them
    for r32 in (O.eval_sequence(z['images'], W, T, reset_period=int(z['reset_period']), dtype=np.float32),
                OT.eval_sequence(z['images'], W, T, reset_period=int(z['reset_period']))):
        assert np.abs(r32[..., :3] - z['records'][..., :3]).max() <= 2e-5
        assert (np.abs(r32[..., 3] - z['records'][..., 3]) / np.abs(z['records'][..., 3])).max() <= 2e-5


def test_oracle_symmetric_form_fusion_matches_get_kf_coord2(ev):
    z, W, rec, dbg = ev
    d = dbg[1]
    x, s = O.get_kf_coord2(d['temp_x'], d['temp_s'], d['z'], d['sz'])
    pin('eval kf2_x', x, z['kf2_x1'])
    pin('eval kf2_s', s, z['kf2_s1'])
    # the two forms of the posterior variance agree here (1 - K > 0), as algebra says they must
    assert rel(z['kf2_s1'], z['kf_s1']) < 1e-12


def test_oracle_samplers_keep_their_batch_1_contract():
    img, at = np.zeros((2, 4, 5, 3)), np.zeros((2, 4, 5, 2))
    with pytest.raises(ValueError, match='batch 1'):
        O.bilinear_sampler(img, at)
    with pytest.raises(ValueError, match='batch 1'):
        OT.bilinear_sampler(img, at)
    assert O.bilinear_sampler(img[:1], at[:1]).shape == (1, 4, 5, 3)


# ---- the losses and the filter from leaves -------------------------------------------------------------------------------------------
MEASURED.update({
    'one l_measure': 0.0, 'one l_temp': 0.0, 'one l_KF': 0.0, 'one loss': 0.0, 'one temp': 2.4e-16, 'one kf': 4.0e-16,
    'one flow': 0.0, 'one d_pred': 1.5e-15, 'one d_flow': 8.2e-16, 'one d_sigma_trans': 4.4e-16, 'one reproj': 0.0,
    'one d_reproj': 6.1e-17, 'one sampler': 0.0, 'one sampler O': 0.0,
})


@pytest.fixture(scope='module')
def tr():
    from kfnet_amd.synth import synthetic_sequence
    z = np.load(os.path.join(GOLD, 'ref_train_small.npz'))
    frames = synthetic_sequence(4, 64, 96, seed=int(z['train_seed']))
    assert hashlib.sha256(frames.tobytes()).hexdigest() == str(z['frames_sha256']), 'synthetic frame generator drifted'
    assert np.array_equal(frames[:, ::8, ::8], z['frames_grid'])
    # KFNet/train.py:49-58 and :280: the graph gets inv(float32 matrix) and inverts it again; the restatements take the matrix
    M = np.linalg.inv(np.linalg.inv(z['matrix'].astype(np.float32)).astype(np.float64))
    assert np.abs(M - z['matrix']).max() < 1e-6
    return z, frames, M


def part_one_inputs(z):
    B, h, w, _ = z['pred'].shape
    flow = np.concatenate([np.zeros((1, h, w, 2)), z['one64:flow']])[None]                       # [1,4,h,w,2], slot 0 unused
    st = np.concatenate([np.zeros((1, h, w)), z['sigma_trans'].astype(np.float64).reshape(B - 1, h, w)])[None]
    return B, h, w, flow, st


def test_fixture_inputs_sit_clear_of_every_kink(tr):
    z, frames, M = tr
    assert float(z['e_fp32_worst']) <= 1e-3                      # no ReLU, floor or clip decides a case
    assert np.isfinite(z['one64:d_pred']).all() and np.abs(z['one64:d_flow']).max() > 0 and np.abs(z['one64:d_sigma_trans']).max() > 0
    m = z['labels1'][..., 3]
    assert (m == 0.5).sum() == 1 and 0.5 < (m == 1.0).mean() < 0.95          # a mask with holes, one value that is not 1
    at = KR.pixel_map(8, 12, torch.float64).numpy() + z['one64:flow']
    assert np.abs(at - np.round(at)).min() > 1e-3
    assert (at.min() < 0) and (at[..., 0].max() > 11)             # the clamped-weight branch of the sampler is live


def test_stage_1_loss_restatement_matches_measure_coord_loss(tr):
    z, frames, M = tr
    pred = torch.from_numpy(z['pred'].astype(np.float64))
    L, nll, smooth, acc, valid = R.coord_loss(pred, z['labels1'], z['frames_grid'].astype(np.float64), M, CLIP, SMOOTH)
    pin('one l_measure', L.item(), z['one64:l_measure'])
    assert acc.item() == float(z['one64:a_measure']) and valid.item() == float(z['one64:valid']) + 1.0
    # without the reference's clip the number is another one: the cap from above is live in this fixture
    assert abs(R.coord_loss(pred, z['labels1'], z['frames_grid'].astype(np.float64), M, None, SMOOTH)[0].item() - L.item()) > 1.0


def test_filter_restatement_matches_get_kf_coord_batch(tr):
    z, frames, M = tr
    B, h, w, flow, st = part_one_inputs(z)
    pred = torch.from_numpy(z['pred'].astype(np.float64))
    # the soft-argmax: cell k = 8 i + j of the window stands for the offset (j - 4, i - 4) = (x, y)
    pin('one flow', (z['prob'].astype(np.float64) @ FR.OFFSETS).reshape(3, h, w, 2), z['one64:flow'])
    assert np.array_equal(FR.flow_head(torch.zeros(1, 64), torch.zeros(1))[1].numpy(), FR.OFFSETS.mean(0, keepdims=True))
    temp, kf = KR.filter_forward(KR.measurement(pred)[None], flow, st)
    pin('one temp', temp[0].numpy(), z['one64:temp'])
    pin('one kf', kf[0].numpy(), z['one64:kf'])
    L, stats, terms = KR.filter_loss(pred, temp[0], kf[0], z['labels1'], z['frames_grid'].astype(np.float64), M, CLIP, SMOOTH)
    pin('one loss', L.item(), z['one64:loss'])
    pin('one l_temp', terms[1].item(), z['one64:l_temp'])
    pin('one l_KF', terms[2].item(), z['one64:l_KF'])
    assert [s.item() for s in stats[7:10]] == [float(z['one64:a_measure']), float(z['one64:a_temp']), float(z['one64:a_KF'])]
    L2, _, _ = KR.step_loss(pred, 1, B, flow[0], st[0], z['labels1'], z['frames_grid'].astype(np.float64), M, CLIP, SMOOTH)
    assert L2.item() == L.item()


def test_joint_restatement_gradients_match_the_reference(tr):
    z, frames, M = tr
    B, h, w, flow, st = part_one_inputs(z)
    p, fl, s = JR.tensor(z['pred'], torch.float64, True), JR.tensor(flow, torch.float64, True), JR.tensor(st, torch.float64, True)
    temp, kf = JR.filter_forward(KR.measurement(p)[None], fl, s)
    L, _, _ = KR.filter_loss(p, temp[0], kf[0], z['labels1'], z['frames_grid'].astype(np.float64), M, CLIP, SMOOTH)
    gp, gf, gs = torch.autograd.grad(L, [p, fl, s])
    pin('one d_pred', gp.numpy(), z['one64:d_pred'])
    pin('one d_flow', gf.numpy()[0, 1:], z['one64:d_flow'])
    pin('one d_sigma_trans', gs.numpy()[0, 1:], z['one64:d_sigma_trans'])
    assert not gf.numpy()[0, 0].any() and not gs.numpy()[0, 0].any()


def test_reprojection_restatement_matches_the_reference(tr):
    z, frames, M = tr
    x = torch.from_numpy(z['pred'][..., :3].astype(np.float64)).requires_grad_(True)
    Rv, rho = RR.reproj_loss(x, z['poses'][:, :3], z['rays'], (z['labels1'][..., 3] == 1.0).astype(np.float64))
    g, = torch.autograd.grad(Rv, [x])
    pin('one reproj', Rv.item(), z['one64:reproj'])
    pin('one d_reproj', g.numpy(), z['one64:d_reproj'])
    # valid_pixel + 1 taken twice: with a single + 1 the value differs in the fourth digit at this mask
    once = (torch.from_numpy((z['labels1'][..., 3] == 1.0).astype(np.float64)) * rho).sum() / (float(z['one64:valid']) + 1.0)
    assert abs(once.item() / float(z['one64:reproj']) - 1.0) > 1e-4


def test_batched_sampler_restatement_matches_the_reference_at_batch_3(tr):
    z, frames, M = tr
    B, h, w, flow, st = part_one_inputs(z)
    at = KR.pixel_map(h, w, torch.float64) + torch.from_numpy(z['one64:flow'])
    got = KR.sampler(torch.from_numpy(z['one64:kf'][:3]), at)
    pin('one sampler', got.numpy(), z['one64:sampler_batched'])
    one = np.concatenate([O.bilinear_sampler(z['one64:kf'][b:b + 1], at.numpy()[b:b + 1]) for b in range(3)])
    pin('one sampler O', one, z['one64:sampler_batched'])
    # element 1 of the batch reads frame 1: sampling everything from frame 0 is a different map
    assert rel(KR.sampler(torch.from_numpy(z['one64:kf'][:1]).expand(3, -1, -1, -1), at).numpy(), z['one64:sampler_batched']) > 1e-2


def test_metrics_oracle_matches_the_loss_as_the_eval_graph_calls_it(tr):
    """oracle/kfnet_metrics_oracle.py works in float32: its bound is float32's, 1e-5 of a sum of some 170 terms of size <= 8."""
    z, frames, M = tr
    T = np.linalg.inv(z['matrix'].astype(np.float32))
    pred = z['pred'][1:2]
    loss, acc = MO.coord_loss_with_uncertainty(MO.apply_transform(pred[..., :3], T), np.exp(pred[..., 3:4].astype(np.float64)),
                                               z['labels1'][0:2, ..., :3], z['labels1'][0:2, ..., 3:4])
    print('metrics oracle loss %.9g reference %.9g, accuracy %.9g reference %.9g' % (loss, z['one64:eval_loss'], acc,
                                                                                    z['one64:eval_accuracy']))
    assert abs(loss - float(z['one64:eval_loss'])) <= 1e-5 * abs(float(z['one64:eval_loss']))
    assert abs(acc - float(z['one64:eval_accuracy'])) <= 1e-6


# ---- whole steps -----------------------------------------------------------------------------------------------------------------------
MEASURED.update({'s1 stats': 1.6e-16, 's1 bias': 8.6e-16, 's1 norm': 3.3e-16, 's1 projection': 1.3e-15,
                 's3 stats': 1.5e-16, 's3 bias': 4.8e-14, 's3 norm': 4.1e-14, 's3 projection': 6.9e-14, 's3 flow': 1.1e-15})


def unpack(z, stage):
    pre = 's%d:' % stage
    sizes = z[pre + 'bias_sizes']
    ends = np.cumsum(sizes)
    biases = {str(n): z[pre + 'bias_grads'][e - k:e] for n, k, e in zip(z[pre + 'biases'], sizes, ends)}
    kernels = [str(n) for n in z[pre + 'kernels']]
    stats = dict(zip((str(s) for s in z[pre + 'stats']), z[pre + 'stat_values']))
    return biases, kernels, z[pre + 'norms'], z[pre + 'projections'], stats


def check_step(z, stage, stats, grads):
    biases, kernels, norms, projs, want = unpack(z, stage)
    tag = 's%d ' % stage
    assert sorted(grads) == sorted(list(biases) + kernels)
    keys = [k for k in want if not k.startswith('a_')]
    pin(tag + 'stats', [stats[k] for k in keys], [want[k] for k in keys])
    for k in want:
        if k.startswith('a_'):
            assert stats[k] == want[k], k
    worst = {'bias': 0.0, 'norm': 0.0, 'projection': 0.0}
    for n, g in biases.items():
        if n == RECIPE.ZERO_BY_SYMMETRY:
            scale = np.abs(grads['Temporal/prediction/kernel']).max()
            assert np.abs(g).max() <= 1e-12 * scale and np.abs(grads[n]).max() <= 1e-12 * scale
            continue
        worst['bias'] = max(worst['bias'], rel(grads[n], g))
    for i, n in enumerate(kernels):
        g = grads[n]
        worst['norm'] = max(worst['norm'], abs(np.sqrt((g * g).sum()) / norms[i] - 1.0))
        worst['projection'] = max(worst['projection'], abs((g * RECIPE.projection_vector(n, g.shape)).sum() - projs[i]) / norms[i])
    for k, e in worst.items():
        SEEN[tag + k] = e
        print('%-28s deviation %.3e  bound %.1e' % (tag + k, e, bound(tag + k)))
        assert e <= bound(tag + k), (tag + k, e)


def train_weights(z):
    W = RECIPE.train_weights()
    assert RECIPE.weights_digest(W) == str(z['weights_sha256']), 'initial weight generator drifted'
    return W


def test_stage_1_step_restatement_matches_the_reference(tr):
    z, frames, M = tr
    stats, grads = R.loss_and_grads(frames, z['labels2'], train_weights(z), M, CLIP, SMOOTH)
    # tests/train_ref.py calls the NLL alone l_measure; MeasureCoordLoss returns it with 50 x SmoothLoss added
    stats = dict(stats, l_measure=stats['l_measure'] + SMOOTH * stats['l_smooth'])
    check_step(z, 1, stats, grads)


def test_joint_step_restatement_matches_the_reference(tr):
    z, frames, M = tr
    stats, grads, flow = JR.loss_and_grads(frames, z['labels2'], train_weights(z), 1, 4, M, CLIP, SMOOTH)
    check_step(z, 3, stats, grads)
    pin('s3 flow', flow[0, 1:], z['s3:flow'])
    assert np.abs(grads['Temporal/feat1/kernel']).max() > 0 and np.abs(grads['Temporal/uncertainty/kernel']).max() > 0


# ---- the recipe again -------------------------------------------------------------------------------------------------------------------
REFERENCE = os.environ.get('KFN_REFERENCE', '/root/reference')


@pytest.mark.skipif(not os.path.isfile(os.path.join(REFERENCE, 'KFNet', 'KFNet.py')),
                    reason='no reference checkout at KFN_REFERENCE=%s: the committed fixtures are used as they are' % REFERENCE)
def test_recipe_reproduces_the_committed_fixtures(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'oracle', 'run_reference.py'), '--reference', REFERENCE,
                          '--out', str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout.decode()[-3000:]
    for name in ('ref_kfnet_small.npz', 'ref_train_small.npz'):
        new, old = np.load(str(tmp_path / name)), np.load(os.path.join(GOLD, name))
        assert sorted(new.files) == sorted(old.files), name
        for k in old.files:
            if old[k].dtype.kind in 'US':
                assert k == 'source' or np.array_equal(new[k], old[k]), (name, k)
            elif old[k].dtype.kind in 'iub':
                assert np.array_equal(new[k], old[k]), (name, k)
            elif k.startswith('one32:'):
                # the values of a float32 run: to float32's precision (another CPU may round another way)
                assert rel(new[k], old[k]) <= 1e-5, (name, k, rel(new[k], old[k]))
            elif ':e_' in k or k.startswith('one_e:') or k == 'e_fp32_worst':
                # the measured errors of a float32 run are rounding noise themselves: held to the fixture's own requirement
                # (the bias that is zero by symmetry has no scale: its entry is a ratio to nothing, and is left out)
                assert np.all(new[k][np.asarray(new[k]) < 1e3] <= 1e-3), (name, k)
            else:
                assert rel(new[k], old[k]) <= 1e-12, (name, k, rel(new[k], old[k]))
    # the reference checkout was only read
    assert b'Traceback' not in out.stdout
