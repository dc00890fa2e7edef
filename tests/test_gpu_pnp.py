"""kfn_pnp_ransac / kfn_pnp_hypotheses on the device (ABI 11) against ground truth and against the numpy restatement
tests/pnp_ref.py.  Synthetic records: random poses, depths 0.5..5 m, scene coordinates back-projected from pixel (8c, 8r)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pnp_ref as P
from kfnet_amd import _lib
from kfnet_amd.KFNet import pnp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frames(seed, B, h=60, w=80, outliers=0.0, noise=0.0, fx=525., fy=525., u=320., v=240.):
    rng = np.random.default_rng(seed)
    recs, gts, masks = [], [], []
    for _ in range(B):
        R, t = P.random_pose(rng)
        rec = P.synthetic_records(rng, h, w, R, t, fx, fy, u, v)
        if noise:
            rec[..., :3] += rng.normal(scale=noise, size=rec[..., :3].shape).astype(np.float32)
        out = rng.random((h, w)) < outliers
        rec[..., :3][out] = rng.uniform(-5, 5, size=(int(out.sum()), 3)).astype(np.float32)
        recs.append(rec)
        gts.append(P.cam_to_world(R, t))
        masks.append(~out)
    return np.stack(recs), np.stack(gts), np.stack(masks)


def test_noise_free_all_inliers():
    recs, gts, _ = _frames(1, 8)
    poses, info = pnp.PnPSolver(60, 80).solve(recs)
    rot, trans = pnp.pose_errors(poses, gts)
    assert (info[:, 0] == _lib.PNP_OK).all() and (info[:, 1] == 4800).all()
    assert (info[:, 2] >= 4790).all(), info
    assert rot.max() < 1e-2 and trans.max() < 1e-3, (rot, trans)


def test_half_outliers_and_1cm_noise():
    recs, gts, masks = _frames(2, 8, outliers=0.5, noise=0.01)
    poses, info = pnp.PnPSolver(60, 80).solve(recs)
    rot, trans = pnp.pose_errors(poses, gts)
    assert (info[:, 0] == _lib.PNP_OK).all()
    assert rot.max() < 0.5 and trans.max() < 0.02, (rot, trans)
    true_inliers = masks.reshape(8, -1).sum(1)
    # a noisy near point can leave the 10 px gate, a few outliers fall into it by chance
    assert (np.abs(info[:, 2] - true_inliers) <= 0.1 * true_inliers).all(), (info[:, 2], true_inliers)


def test_unconfident_and_nan_cells_are_excluded():
    recs, gts, _ = _frames(3, 4)
    rng = np.random.default_rng(30)
    low = rng.random(recs.shape[:3]) < 0.3
    recs[..., 3][low] = 20.0                                   # == threshold: excluded (strict >)
    recs[..., 0:3][low] = rng.uniform(-5, 5, size=(int(low.sum()), 3))   # and wrong
    nan = rng.random(recs.shape[:3]) < 0.1
    recs[..., 1][nan] = np.nan
    inf = rng.random(recs.shape[:3]) < 0.05
    recs[..., 2][inf] = np.inf
    expect = ((recs[..., 3] > 20.0) & np.isfinite(recs[..., :3]).all(-1)).reshape(4, -1).sum(1)
    poses, info = pnp.PnPSolver(60, 80).solve(recs)
    assert (info[:, 1] == expect).all(), (info[:, 1], expect)
    assert (info[:, 2] <= expect).all() and (info[:, 2] >= expect - 10).all()
    rot, trans = pnp.pose_errors(poses, gts)
    assert rot.max() < 1e-2 and trans.max() < 1e-3


def test_too_few_candidates_gives_status_and_nan_without_touching_neighbours():
    recs, gts, _ = _frames(4, 3)
    bad = recs.copy()
    bad[1, ..., 3] = 1.0
    bad[1, 0, :10, 3] = 100.0                                  # 10 candidates < min_points 16
    solver = pnp.PnPSolver(60, 80)
    poses, info = solver.solve(bad)
    assert tuple(info[1]) == (_lib.PNP_TOO_FEW_POINTS, 10, 0, -1)
    assert np.isnan(poses[1]).all()
    ref_poses, ref_info = solver.solve(recs)
    for b in (0, 2):
        assert np.array_equal(poses[b], ref_poses[b]) and np.array_equal(info[b], ref_info[b])


def test_frame_alone_equals_frame_in_batch_and_launches_repeat():
    recs, _, _ = _frames(5, 20, outliers=0.4, noise=0.01)
    solver = pnp.PnPSolver(60, 80)
    p1, i1 = solver.solve(recs)
    p2, i2 = solver.solve(recs)
    assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32)) and np.array_equal(i1, i2)
    for k in (0, 7, 19):
        pk, ik = solver.solve(recs[k:k + 1], t0=k)
        assert np.array_equal(pk[0].view(np.uint32), p1[k].view(np.uint32)) and np.array_equal(ik[0], i1[k])


def test_hypotheses_match_the_numpy_reference():
    recs, _, _ = _frames(6, 3, outliers=0.5, noise=0.01)
    H, t0, seed = 256, 40, 99
    solver = pnp.PnPSolver(60, 80, hypotheses=H, seed=seed)
    samples, hp, counts = solver.hypotheses_probe(recs, t0=t0)
    valid = agree = 0
    for b in range(3):
        rs, rp, rc, X, _ = P.hypotheses(recs[b], t0 + b, H, seed=seed)
        n = X.shape[0]
        assert np.array_equal(samples[b], rs)                          # the same draws, bit for bit
        both = (counts[b] >= 0) & (rc >= 0)
        assert ((counts[b] >= 0) == (rc >= 0)).mean() >= 0.99
        assert np.abs(hp[b][both] - rp[both]).max() < 1e-4
        assert np.abs(counts[b][both] - rc[both]).max() <= 0.005 * n   # fp32 vs fp64 at the 10 px threshold
        valid += both.sum()
        agree += (counts[b][both] == rc[both]).sum()
    assert valid > 0.5 * 3 * H and agree > 0.5 * valid      # (a sample with an outlier often has no P3P solution)


def test_config5_grid_and_intrinsics():
    fx = fy = 1050.0 * 540 / 1080
    u, v = 480.0, 270.0
    recs, gts, _ = _frames(7, 4, h=68, w=120, outliers=0.3, noise=0.005, fx=fx, fy=fy, u=u, v=v)
    poses, info = pnp.PnPSolver(68, 120, fx, fy, u, v).solve(recs)
    rot, trans = pnp.pose_errors(poses, gts)
    assert (info[:, 0] == _lib.PNP_OK).all() and (info[:, 1] == 8160).all()
    assert rot.max() < 0.5 and trans.max() < 0.02, (rot, trans)


def test_torch_input_stays_on_the_device():
    import torch
    recs, gts, _ = _frames(8, 2)
    t = torch.from_numpy(recs).cuda()
    poses, info = pnp.PnPSolver(60, 80).solve(t)
    assert poses.is_cuda and poses.shape == (2, 4, 4) and info.dtype == torch.int32
    rot, trans = pnp.pose_errors(poses.cpu().numpy(), gts)
    assert rot.max() < 1e-2 and trans.max() < 1e-3


def _run(args):
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, timeout=600)


def test_cli_end_to_end(tmp_path):
    recs, gts, _ = _frames(9, 5, outliers=0.5, noise=0.01)
    coord_list, gt_list = [], []
    for i in range(5):
        c = str(tmp_path / ('coord_%d.npy' % i))
        np.save(c, recs[i])
        g = str(tmp_path / ('frame-%06d.pose.txt' % i))
        pnp.write_pose(g, gts[i])
        coord_list.append(c)
        gt_list.append(g)
    (tmp_path / 'coords.txt').write_text('\n'.join(coord_list) + '\n')
    (tmp_path / 'gt.txt').write_text('\n'.join(gt_list) + '\n')
    out = tmp_path / 'out'
    r = _run(['-m', 'kfnet_amd.KFNet.pnp', str(tmp_path / 'coords.txt'), str(out), '--gt', str(tmp_path / 'gt.txt'),
              '--thread_num', '4', '--batch', '2'])
    assert r.returncode == 0, r.stdout
    assert 'median rotation error' in r.stdout and 'within 5cm/5deg: 100.0 %' in r.stdout, r.stdout
    for i in range(5):
        rot, trans = pnp.pose_errors(pnp.read_pose(str(out / ('pose_%d.txt' % i))), gts[i])
        assert rot < 0.5 and trans < 0.02


def test_eval_pose_writes_pose_files(tmp_path):
    r = _run(['-m', 'kfnet_amd.KFNet.eval', '--scene', 'chess', '--synthetic', '8', '--random_weights', '--pose',
              '--output_folder', str(tmp_path)])
    assert r.returncode == 0, r.stdout
    assert 'poses:' in r.stdout
    for i in range(8):
        rec = np.load(str(tmp_path / ('coord_%d.npy' % i)))
        T = pnp.read_pose(str(tmp_path / ('pose_%d.txt' % i)))
        _, info = pnp.PnPSolver(rec.shape[0], rec.shape[1]).solve(rec[None], t0=i)
        assert np.isfinite(T).all() == (info[0, 0] == _lib.PNP_OK)
        assert np.isnan(T).all() == (info[0, 0] != _lib.PNP_OK)
