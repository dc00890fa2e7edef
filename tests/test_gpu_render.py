"""kfn_render on the device against the numpy float32 restatement of tests/render_ref.py, bit for bit at every
sample; the atomic z-buffer under contention; the existing depth path; the round trip through the pose stage; the program
`python -m kfnet_amd.render make` and training from what it writes; hipGraph capture."""
import os

import numpy as np
import pytest

import render_ref as R
from kfnet_amd import _lib, synth
from kfnet_amd import render as M
from kfnet_amd.labels import DepthCamera, DepthLabeler, decorrelating_transform, add_frames, load_depth

pytestmark = pytest.mark.gpu


def _camera(cam):
    return DepthCamera(cam.fx, cam.fy, cam.u, cam.v, scale=cam.scale, raw_min=cam.raw_min, raw_max=cam.raw_max)


def _host(r, out, n):
    import torch
    labels, depth, frames, stats = out
    torch.cuda.synchronize()
    keys = r.zbuf[:n].cpu().numpy()
    z = np.where(keys == -1, 0, (keys >> 32) & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
    return dict(labels=labels.cpu().numpy().copy(), depth=depth.cpu().numpy().copy(), frames=frames.cpu().numpy().copy(),
                stats=stats.cpu().numpy().copy(), winner=r.winners(n), z=z)


def _device(v, c, t, poses, H, W, stride, cam, batch=None):
    n = len(poses)
    r = M.Renderer(v, t, c, (H, W), batch or n, stride, _camera(cam), cam.near)
    return _host(r, r.render(poses), n), r


def _same_bits(dev, ref, what):
    assert np.array_equal(dev['stats'], ref['stats']), (what, dev['stats'], ref['stats'])
    assert np.array_equal(dev['winner'], ref['winner']), (what, int((dev['winner'] != ref['winner']).sum()))
    assert np.array_equal(dev['z'].view(np.uint32), ref['z'].astype(np.float32).view(np.uint32)), what
    assert np.array_equal(dev['labels'].view(np.uint32), ref['labels'].view(np.uint32)), what
    assert np.array_equal(dev['depth'], ref['depth']), what
    assert np.array_equal(dev['frames'], ref['frames']), (what, int((dev['frames'] != ref['frames']).sum()))


# -- bit identity with the float32 restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(R.hand_cases()))
def test_hand_cases_bit_for_bit(name):
    v, t, cam = R.hand_cases()[name]
    dev, _ = _device(v, None, t, R.IDENTITY, 16, 24, 1, cam)
    _same_bits(dev, R.render(v, None, t, R.IDENTITY, 16, 24, 1, cam), name)


@pytest.mark.parametrize('args', [a for a, _ in R.RANDOM_CASES], ids=lambda a: '%dx%d_s%d_cells%d_B%d' % a[:5])
def test_synthetic_scenes_bit_for_bit(args):
    v, c, t, poses, cam = R.scene_case(*args)
    H, W, s = args[:3]
    dev, _ = _device(v, c, t, poses, H, W, s, cam)
    ref = R.render(v, c, t, poses, H, W, s, cam)
    assert (ref['winner'] >= 0).all()                                        # a closed room: no sample sees nothing
    _same_bits(dev, ref, args)


def test_a_non_finite_pose_gives_zeros_and_its_flag():
    v, c, t, poses, cam = R.scene_case(64, 96, 8, 4, 3, 2)
    poses = poses.copy()
    poses[1, 0, 3] = np.nan
    dev, _ = _device(v, c, t, poses, 64, 96, 8, cam)
    _same_bits(dev, R.render(v, c, t, poses, 64, 96, 8, cam), 'nan pose')
    assert dev['stats'][:, 3].tolist() == [0, 1, 0] and not dev['labels'][1].any() and not dev['depth'][1].any()
    assert (dev['winner'][1] == -1).all() and dev['labels'][0][..., 3].all()


# -- the z-buffer under contention -------------------------------------------------------------------------------------------------
def test_256_layers_over_one_image_the_nearest_last():
    import torch
    layers = 256
    tris = [((-1000, -1000, 1), (3000, -1000, 1), (-1000, 3000, 1))]
    v = np.concatenate([np.asarray(tris[0], dtype=np.float32) * np.float32(1.0 + (layers - 1 - k) / 64.0) for k in range(layers)])
    t = np.arange(3 * layers, dtype=np.int32).reshape(-1, 3)
    cam = R.hand_camera()
    dev, r = _device(v, None, t, R.IDENTITY, 16, 24, 1, cam)
    assert (dev['winner'] == layers - 1).all() and (dev['z'] == 1.0).all()
    _same_bits(dev, R.render(v, None, t, R.IDENTITY, 16, 24, 1, cam), 'layers')
    again = _host(r, r.render(R.IDENTITY), 1)
    r.zbuf.copy_(torch.randint(-2 ** 62, 2 ** 62, tuple(r.zbuf.shape), dtype=torch.int64, device=r.zbuf.device))   # garbage
    r.stats.fill_(77)
    dirty = _host(r, r.render(R.IDENTITY), 1)
    for other in (again, dirty):
        _same_bits(other, dev, 'relaunch')


# -- one production-size frame -------------------------------------------------------------------------------------------------------
def test_production_size_at_both_strides():
    v, c, t, poses, cam = R.scene_case(480, 640, 8, 32, 2, 4)
    grid, _ = _device(v, c, t, poses, 480, 640, 8, cam)
    _same_bits(grid, R.render(v, c, t, poses, 480, 640, 8, cam), 'stride 8')
    full, _ = _device(v, c, t, poses, 480, 640, 1, cam)
    assert full['stats'][:, 0].tolist() == [480 * 640] * 2 and np.array_equal(full['stats'][:, 1:], grid['stats'][:, 1:])
    for k in ('labels', 'depth', 'frames', 'winner', 'z'):
        assert np.array_equal(full[k][:, ::8, ::8], grid[k]), k


# -- vertex indices are checked ------------------------------------------------------------------------------------------------------
def test_out_of_range_triangles_are_counted_and_change_nothing():
    v, c, t, poses, cam = R.scene_case(64, 96, 1, 4, 2, 7)
    bad = np.asarray([(0, 1, len(v)), (-1, 2, 3), (4, 2 ** 31 - 1, 5)], dtype=np.int32)
    clean, _ = _device(v, c, t, poses, 64, 96, 1, cam)
    dirty, _ = _device(v, c, np.concatenate([bad, t]), poses, 64, 96, 1, cam)
    assert dirty['stats'][:, 4].tolist() == [3, 3] and clean['stats'][:, 4].tolist() == [0, 0]
    assert np.array_equal(dirty['stats'][:, :4], clean['stats'][:, :4])
    assert np.array_equal(dirty['winner'], clean['winner'] + 3)
    for k in ('labels', 'depth', 'frames', 'z'):
        assert np.array_equal(dirty[k], clean[k]), k


# -- against the depth path that training already consumes -------------------------------------------------------------------------
def test_rendered_depth_through_the_depth_labeler_gives_the_rendered_labels():
    import torch
    H, W = 64, 96
    v, c, t, poses, cam = R.scene_case(H, W, 1, 4, 3, 6)
    dev, r = _device(v, c, t, poses, H, W, 1, cam)
    lab = DepthLabeler(3, H, W, 1, _camera(cam)).labels(dev['depth'], poses)
    torch.cuda.synchronize()
    lab = lab.cpu().numpy()
    assert np.array_equal(lab[..., 3], dev['labels'][..., 3]) and lab[..., 3].all()
    rx = (np.arange(W)[None, :] - cam.u) * cam.inv_fx
    ry = (np.arange(H)[:, None] - cam.v) * cam.inv_fy
    ray = np.sqrt(rx * rx + ry * ry + 1.0)
    diff = np.abs(lab[..., :3].astype(np.float64) - dev['labels'][..., :3]).max(axis=-1)
    # The depth map holds z rounded to the nearest raw unit: |dz| <= scale / 2, and the point moves along its ray by |dz| |ray|
    # (R is orthonormal).  The fp32 term: each route evaluates raw * scale or 1 / w, two ray products and three sums of four
    # terms below 8 m in magnitude, each rounding at most half an ulp of 8 m = 2^-22 m; six roundings a route, two routes:
    # 12 * 2^-22 m = 2.9e-6 m.  Measured on the MI355X: the largest |dxyz| - scale / 2 |ray| was -8.9e-7 m: never above the first term.
    fp32_term = 12.0 * 2.0 ** -22
    print('largest |dxyz| %.3g m; largest excess over scale/2 |ray| %.3g m' % (diff.max(), (diff - 0.5 * cam.scale * ray).max()))
    assert (diff <= 0.5 * cam.scale * ray[None] + fp32_term).all()


# -- round trip through the pose stage -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,cells', ((64, 96, 4), (480, 640, 8)))
def test_poses_come_back_from_the_rendered_labels(H, W, cells):
    from kfnet_amd.KFNet import pnp
    v, c, t, poses, cam = R.scene_case(H, W, 8, cells, 8, 12)
    dev, _ = _device(v, c, t, poses, H, W, 8, cam)
    solver = pnp.PnPSolver(H // 8, W // 8, cam.fx, cam.fy, cam.u, cam.v, min_confidence=0.5)      # the mask is the confidence: 1
    for name, records in (('device fp32', dev['labels']),
                          ('fp64 restatement', R.render(v, c, t, poses, H, W, 8, cam, dtype=np.float64)['labels'].astype(np.float32))):
        est, info = solver.solve(records)
        rot, trans = pnp.pose_errors(est, poses)
        print('%s labels: rotation error %.3g deg, centre error %.3g m, inliers %s' % (name, rot.max(), trans.max(), info[:, 2].tolist()))
        if name == 'device fp32':
            assert (info[:, 0] == _lib.PNP_OK).all() and (info[:, 1] == (H // 8) * (W // 8)).all()
            # the tolerance of outlier-free synthetic frames: tests/test_gpu_pnp.py:40 (test_noise_free_all_inliers)
            assert rot.max() < 1e-2 and trans.max() < 1e-3, (rot, trans)


# -- the program, and training from what it writes ---------------------------------------------------------------------------------
H, W = 64, 96


@pytest.fixture(scope='module')
def written(tmp_path_factory):
    root = tmp_path_factory.mktemp('render')
    v, c, t = synth.synthetic_scene(8, 4)
    model = str(root / 'scene.ply')
    M.write_ply(model, v, t, c)
    poses = synth.synthetic_trajectory(6, 8)
    poses[2, 1, 1] = np.inf
    from kfnet_amd.KFNet.pnp import write_pose
    paths = []
    for k in range(6):
        paths.append(str(root / ('frame-%06d.pose.txt' % k)))
        if np.isfinite(poses[k]).all():
            write_pose(paths[-1], poses[k])
        else:
            open(paths[-1], 'w').write('\n'.join('\t'.join('inf' if not np.isfinite(x) else '%.9e' % x for x in row) for row in poses[k]) + '\n')
    plist = str(root / 'poses.txt')
    open(plist, 'w').write(''.join(p + '\n' for p in paths))
    out = str(root / 'out')
    cam = R.scene_camera(H, W)
    flags = ['--focal_x', repr(cam.fx), '--focal_y', repr(cam.fy), '--u', repr(cam.u), '--v', repr(cam.v)]
    rc = M.main(['make', '--model', model, '--poses', plist, '--output_folder', out, '--depth_png', '--frames', '--height', str(H),
                 '--width', str(W), '--batch', '4'] + flags)
    return dict(rc=rc, out=out, mesh=(v, c, t), poses=poses, paths=paths, cam=cam, flags=flags)


def test_render_make_writes_what_the_renderer_gives(written):
    from kfnet_amd.tools.io import read_lines
    assert written['rc'] == 0
    out, cam = written['out'], written['cam']
    lists = dict((n, [x for x in read_lines(os.path.join(out, n)) if x])
                 for n in ('pose_list.txt', 'label_list.txt', 'depth_list.txt', 'image_list.txt'))
    assert all(len(col) == 5 for col in lists.values())
    keep = [0, 1, 3, 4, 5]
    assert lists['pose_list.txt'] == [written['paths'][k] for k in keep]
    v, c, t = written['mesh']
    poses = written['poses'][keep]
    full, _ = _device(v, c, t, poses, H, W, 1, cam)
    grid, r = _device(v, c, t, poses, H, W, 8, cam)
    for k in range(5):
        assert np.array_equal(np.fromfile(lists['label_list.txt'][k], dtype=np.float32).reshape(H, W, 4), full['labels'][k])
    assert np.array_equal(load_depth(lists['depth_list.txt'], (H, W)), full['depth'])
    from PIL import Image
    for k in range(5):
        assert np.array_equal(np.asarray(Image.open(lists['image_list.txt'][k])), full['frames'][k])
    import torch
    pivot = poses[0, :3, 3]
    total = add_frames(None, r.moments(torch.from_numpy(grid['labels']).cuda(), pivot).cpu().numpy())
    assert np.array_equal(np.loadtxt(os.path.join(out, 'transform.txt')),
                          np.array([[float('%.9e' % x) for x in row] for row in decorrelating_transform(total, pivot)]))


@pytest.mark.parametrize('depth', (False, True), ids=('label_files', 'depth'))
def test_training_takes_two_steps_on_the_written_folder(written, tmp_path, depth):
    from kfnet_amd.SCoordNet import train as T
    model = tmp_path / 'model'
    args = ['--scene', 'fire', '--input_folder', written['out'], '--height', str(H), '--width', str(W), '--batch', '2',
            '--max_steps', '2', '--snapshot', '2', '--display', '1', '--seed', '4', '--model_folder', str(model)]
    assert T.main(args + (['--depth'] + written['flags'] if depth else [])) == 0
    with np.load(str(model / 'kfnet_train_state-2.npz')) as st:
        assert int(st['global_step']) == 2
    with np.load(str(model / 'kfnet_weights-2.npz')) as w:
        assert len(w.files) >= 24 and all(np.isfinite(np.asarray(w[k])).all() for k in w.files)


# -- hipGraph capture ---------------------------------------------------------------------------------------------------------------
def test_render_is_captured_and_replayed_with_the_same_bits():
    import torch
    v, c, t, poses, cam = R.scene_case(64, 96, 8, 4, 2, 2)
    direct, r = _device(v, c, t, poses, 64, 96, 8, cam)
    cap = torch.cuda.Stream(device=r.device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cap):
        with torch.cuda.graph(g, stream=cap):
            out = r.launch(2)
    for _ in range(2):
        r.labels.zero_()
        r.zbuf.zero_()
        g.replay()
        _same_bits(_host(r, out, 2), direct, 'replay')
