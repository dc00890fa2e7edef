"""kfn_fuse_integrate, kfn_fuse_extract_count and kfn_fuse_extract on the device against the numpy float32
restatement of tests/fuse_ref.py, bit for bit at every voxel, vertex and triangle; carried state; the scan across its levels;
the topology of the device's own mesh; the round trip through the renderer; the program `python -m kfnet_amd.fuse make` and
what `render make` and training make of its file."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fuse_ref as F
from kfnet_amd import synth
from kfnet_amd import fuse as M
from kfnet_amd import render
from kfnet_amd.labels import DepthCamera, DepthLabeler

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _camera(S):
    depth = dict() if S.registered else dict(depth_fx=S.dfx, depth_fy=S.dfy, depth_u=S.du, depth_v=S.dv)
    return DepthCamera(S.fx, S.fy, S.u, S.v, scale=S.scale, raw_min=S.raw_min, raw_max=S.raw_max, **depth)


def _volume(S, batch, color=True):
    return M.Volume(S.dims, S.origin, S.voxel, S.trunc, _camera(S), S.image_size, batch, color, S.max_weight, S.near)


_rendered = dict()


def gpu_render(v, c, t, poses, H, W, cam):
    """(depth, frames) of the existing Renderer at stride 1, as host arrays."""
    import torch
    key = (len(t), poses.tobytes(), H, W, tuple(sorted(cam.items())))
    if key not in _rendered:
        r = render.Renderer(v, t, c, (H, W), len(poses), 1, DepthCamera(**cam))
        _, depth, frames, _ = r.render(poses)
        torch.cuda.synchronize()
        _rendered[key] = (depth.cpu().numpy().copy(), frames.cpu().numpy().copy())
    return _rendered[key]


def _same_volume(vol, tsdf, col, what):
    import torch
    torch.cuda.synchronize()
    dev = vol.tsdf()
    assert np.array_equal(dev.view(np.uint32), tsdf.view(np.uint32)), (what, int((dev.view(np.uint32) != tsdf.view(np.uint32)).sum()))
    if col is None:
        assert vol.colors() is None
    else:
        devc = vol.colors()
        assert np.array_equal(devc.view(np.uint32), col.view(np.uint32)), (what, int((devc.view(np.uint32) != col.view(np.uint32)).sum()))


def _same_mesh(dev, ref, what):
    for k, name in enumerate(('vertices', 'colors', 'triangles')):
        assert dev[k].shape == ref[k].shape and dev[k].dtype == ref[k].dtype, (what, name, dev[k].shape, ref[k].shape)
    assert np.array_equal(dev[0].view(np.uint32), ref[0].view(np.uint32)), (what, 'vertices')
    assert np.array_equal(dev[1], ref[1]), (what, 'colors')
    assert np.array_equal(dev[2], ref[2]), (what, 'triangles')


# -- integrate, bit for bit at every voxel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', F.INTEGRATE_CASES)
def test_integrate_bit_for_bit(name):
    S, depth, frames, poses = F.integrate_case(name, gpu_render)
    vol = _volume(S, 3, frames is not None)
    vol.integrate(depth, poses, frames)
    tsdf, col = F.integrate(*S.empty(frames is not None), depth, frames, poses, S)
    assert tsdf[..., 1].max() >= 2 and (tsdf[..., 0] < 0).any()
    _same_volume(vol, tsdf, col, name)


def test_hand_case():
    S, depth, frames, poses, where = F.hand_case()
    vol = _volume(S, 1)
    vol.integrate(depth, poses, frames)
    tsdf, col = F.integrate(*S.empty(), depth, frames, poses, S)
    _same_volume(vol, tsdf, col, 'hand')
    dev, devc = vol.tsdf(), vol.colors()
    at = lambda a, k: a[where[k][2], where[k][1], where[k][0]].tolist()
    assert at(dev, 'near') == [1.0, 1.0] and at(devc, 'near') == [0.0, 0.0, 0.0, 0.0]          # Z == near is taken; s = 2.5 > trunc
    assert at(dev, 'behind') == [1.0, 1.0] and at(devc, 'behind') == [0.0, 0.0, 0.0, 0.0]
    assert at(dev, 'minus_trunc') == [-1.0, 1.0] and at(devc, 'minus_trunc') == [200.0, 100.0, 50.0, 1.0]      # s == -trunc is taken
    assert at(dev, 'plus_trunc') == [1.0, 1.0] and at(devc, 'plus_trunc') == [200.0, 100.0, 50.0, 1.0]         # s == trunc: colour taken
    assert at(dev, 'tie_down') == [-1.0, 1.0] and at(devc, 'tie_down') == [200.0, 100.0, 50.0, 1.0]            # 8.5 -> 8
    assert at(dev, 'tie_up') == [-1.0, 1.0] and at(devc, 'tie_up') == [10.0, 20.0, 30.0, 1.0]                  # 9.5 -> 10
    assert at(dev, 'between') == [0.0, 0.0]                                                                    # 9: the invalid pixel


# -- carried state ---------------------------------------------------------------------------------------------------------------------
def test_state_is_carried_from_call_to_call():
    import torch
    S, depth, frames, poses = F.integrate_case('cap', gpu_render)
    whole = _volume(S, 3)
    whole.integrate(depth, poses, frames)
    torch.cuda.synchronize()
    want, wantc = whole.tsdf(), whole.colors()
    split = _volume(S, 4)
    split.integrate(depth[:2], poses[:2], frames[:2])
    split.integrate(depth[2:], poses[2:], frames[2:])
    _same_volume(split, want, wantc, 'frames 0-1, then 2')
    single = _volume(S, 1)
    for k in range(3):
        single.integrate(depth[k:k + 1], poses[k:k + 1], frames[k:k + 1])
    _same_volume(single, want, wantc, 'batch 1')
    dirty = _volume(S, 3)
    dirty.tsdf_volume.copy_(torch.randn(dirty.tsdf_volume.shape, device=dirty.device) * 1e6)
    dirty.color_volume.copy_(torch.randn(dirty.color_volume.shape, device=dirty.device) * 1e6)
    dirty.integrate(depth, poses, frames)
    torch.cuda.synchronize()
    assert not np.array_equal(dirty.tsdf(), want)
    dirty.tsdf_volume.zero_()
    dirty.color_volume.zero_()
    dirty.integrate(depth, poses, frames)
    _same_volume(dirty, want, wantc, 'garbage, then zeroed')


# -- workgroups that no frame touches -----------------------------------------------------------------------------------------------------
def test_workgroups_outside_every_frustum_change_nothing():
    H, W = F.FUSE_IMAGE
    cam = F.render_camera(H, W)
    v, c, t = synth.synthetic_scene(5, 4)
    poses = np.stack([np.eye(4)] * 2)
    for k, centre in enumerate(((1.0, 1.5, 1.2), (1.3, 1.4, 1.1))):
        poses[k, :3, 0], poses[k, :3, 1], poses[k, :3, 2], poses[k, :3, 3] = (0, -1, 0), (0, 0, -1), (1, 0, 0), centre    # looking along +x
    depth, frames = gpu_render(v, c, t, poses, H, W, cam)
    S = F.Setup(dims=(96, 40, 40), origin=(-0.3, 0.5, 0.3), voxel=0.05, image_size=(H, W), **cam)
    vol = _volume(S, 2)
    vol.integrate(depth, poses, frames)
    tsdf, col = F.integrate(*S.empty(), depth, frames, poses, S)
    W0 = tsdf[..., 1]
    assert (W0[:, :, :20] == 0).all() and (W0 == 2).any()                    # behind both cameras; and seen by both
    untouched = (W0.reshape(40, 10, 4, 96) == 0).all(axis=(2,))
    assert untouched[:, :, :64].all(axis=2).any()                             # whole 64 x 4 x 1 bricks see nothing
    _same_volume(vol, tsdf, col, 'bricks')


# -- extract, bit for bit and in order ------------------------------------------------------------------------------------------------------
def _device_mesh(S, tsdf, col, min_weight=1.0, vol=None):
    import torch
    vol = vol or _volume(S, 1, col is not None)
    vol.tsdf_volume.copy_(torch.from_numpy(np.ascontiguousarray(tsdf)))
    if col is not None:
        vol.color_volume.copy_(torch.from_numpy(np.ascontiguousarray(col)))
    return vol.mesh(min_weight), vol


@pytest.mark.parametrize('min_weight', (1.0, 2.0))
def test_extract_from_the_fused_volume_bit_for_bit(min_weight):
    S, depth, frames, poses = F.integrate_case('unregistered', gpu_render)
    vol = _volume(S, 3)
    vol.integrate(depth, poses, frames)
    dev = vol.mesh(min_weight)
    tsdf, col = F.integrate(*S.empty(), depth, frames, poses, S)
    ref = F.extract(tsdf, col, S, min_weight)
    assert len(ref[0]) > 50 and len(ref[2]) > 50 and len(np.unique(ref[1], axis=0)) > 10
    _same_mesh(dev, ref, min_weight)


@pytest.fixture(scope='module')
def field_meshes():
    out = dict()
    for name, (S, tsdf) in F.analytic_fields().items():
        (dev, _), ref = _device_mesh(S, tsdf, None), F.extract(tsdf, None, S)
        out[name] = (S, dev, ref)
    return out


@pytest.mark.parametrize('name', sorted(F.analytic_fields()))
def test_extract_from_analytic_fields_bit_for_bit(field_meshes, name):
    S, dev, ref = field_meshes[name]
    assert len(ref[2]) > 500
    _same_mesh(dev, ref, name)


def test_the_devices_own_sphere_is_closed_oriented_and_close(field_meshes):
    S, (v, c, t), _ = field_meshes['sphere']
    F.closed_surface_checks(v, t)
    dist = np.linalg.norm(v.astype(np.float64) - np.asarray(F.SPHERE_CENTRE), axis=1)
    assert np.abs(dist - F.SPHERE_RADIUS).max() <= 3.0 * S.voxel ** 2 / (8.0 * (F.SPHERE_RADIUS - np.sqrt(3.0) * S.voxel))
    S2, (v2, c2, t2), _ = field_meshes['two_spheres']
    F.closed_surface_checks(v2, t2, components=2)
    S3, (v3, c3, t3), _ = field_meshes['cut_sphere']
    uses = F.edge_uses(t3)
    assert set(uses.values()) == {1} and any((b, a) not in uses for a, b in uses)
    assert v3[np.unique(t3)][:, 0].max() <= np.floor(1.7 / S3.voxel - 1e-9) * S3.voxel


def test_a_shell_of_a_million_points_crosses_every_level_of_the_scan():
    import torch
    # 128 x 128 x 65 = 1 064 960 points: 1040 blocks of 1024 at the first level, 2 at the second, the totals above them
    S = F.Setup(dims=(128, 128, 65), origin=(0.0, 0.0, 0.0), voxel=1.0 / 32.0)
    centre, radius = (2.01, 1.97, 1.02), 0.93
    dist = F.sphere(centre, radius)
    tsdf = F.field_volume(S, dist, valid=lambda X, Y, Z: np.abs(dist(X, Y, Z)) < 3.0 * S.voxel)
    col = np.zeros(tsdf.shape[:3] + (4,), dtype=np.float32)
    rng = np.random.default_rng(4)
    col[..., :3] = rng.integers(0, 256, size=col.shape[:3] + (3,)).astype(np.float32)
    col[..., 3] = (rng.random(col.shape[:3]) < 0.97).astype(np.float32)
    ref = F.extract(tsdf, col, S)
    V, N = len(ref[0]), len(ref[2])
    assert V > 20000 and N > 40000
    dev, vol = _device_mesh(S, tsdf, col)
    _same_mesh(dev, ref, 'shell')
    F.closed_surface_checks(dev[0], dev[2])
    assert vol.totals.cpu().numpy().tolist() == [V, N]
    # a scratch full of garbage beforehand changes nothing; two runs give the same bits
    vol.scratch.copy_(torch.randint(-2 ** 62, 2 ** 62, tuple(vol.scratch.shape), dtype=torch.int64, device=vol.device))
    vol.totals.fill_(-7)
    _same_mesh(vol.mesh(1.0), dev, 'garbage in scratch')
    # capacities one short of the totals: nothing is written at or past them
    vol.count(1.0)
    vertices = torch.full((V, 3), -5.0, dtype=torch.float32, device=vol.device)
    colors = torch.full((V, 3), 7, dtype=torch.uint8, device=vol.device)
    triangles = torch.full((N, 3), -9, dtype=torch.int32, device=vol.device)
    vol.emit(vertices[:V - 1], colors[:V - 1], triangles[:N - 1])
    torch.cuda.synchronize()
    assert (vertices[V - 1] == -5.0).all() and (colors[V - 1] == 7).all() and (triangles[N - 1] == -9).all()
    _same_mesh((vertices[:V - 1].cpu().numpy(), colors[:V - 1].cpu().numpy(), triangles[:N - 1].cpu().numpy()),
               (ref[0][:V - 1], ref[1][:V - 1], ref[2][:N - 1]), 'one short')


def test_an_empty_volume_gives_an_empty_mesh():
    S = F.Setup(dims=(5, 4, 3), origin=(0, 0, 0), voxel=0.5)
    v, c, t = _volume(S, 1).mesh()
    assert v.shape == (0, 3) and c.shape == (0, 3) and t.shape == (0, 3)
    one = F.Setup(dims=(1, 1, 1), origin=(0, 0, 0), voxel=0.5)
    assert _volume(one, 1).mesh()[2].shape == (0, 3)


# -- round trip through the renderer ----------------------------------------------------------------------------------------------------------
RT_H, RT_W = 64, 96
RT_CAM = dict(fx=78.75, fy=78.75, u=48., v=32.)
RT_VOXEL = 0.04


def test_round_trip_through_the_renderer():
    """Render depth and colour from synthetic_scene(3, 8), fuse them, mesh, render the mesh from the same poses: over all
    samples of all frames the second depth map is the first to a fraction of a voxel.  The restatement (fuse_ref's mesh
    through render_ref, on the CPU) gave 0.68 % uncovered, a median of 0.025 voxel and a 90th percentile of 0.225 voxel (the 99th: 0.18 m, at the boxes' edges), so each
    limit stands a factor of 2.2 or more above it: DESIGN.md 6k."""
    import torch
    v, c, t = synth.synthetic_scene(3, 8)
    poses = synth.synthetic_trajectory(12, 3)
    depth1, frames1 = gpu_render(v, c, t, poses, RT_H, RT_W, RT_CAM)
    assert (depth1 > 0).all()
    S = F.Setup(dims=(106, 81, 69), origin=(-0.1, -0.1, -0.1), voxel=RT_VOXEL, image_size=(RT_H, RT_W), **RT_CAM)
    vol = _volume(S, 12)
    vol.integrate(depth1, poses, frames1)
    mv, mc, mt = vol.mesh(1.0)
    r = render.Renderer(mv, mt, mc, (RT_H, RT_W), 12, 1, DepthCamera(**RT_CAM))
    _, depth2, frames2, _ = r.render(poses)
    torch.cuda.synchronize()
    depth2, frames2 = depth2.cpu().numpy(), frames2.cpu().numpy()
    covered = depth2 > 0
    err = np.abs(depth2.astype(np.float64) - depth1.astype(np.float64))[covered] * S.scale
    uncovered = 1.0 - covered.mean()
    print('%d vertices, %d triangles; uncovered %.4f, median %.4f voxel, 90th percentile %.4f voxel, 99th %.4f m' %
          (len(mv), len(mt), uncovered, np.median(err) / RT_VOXEL, np.percentile(err, 90) / RT_VOXEL, np.percentile(err, 99)))
    assert uncovered <= 0.02
    assert np.median(err) <= RT_VOXEL / 4
    assert np.percentile(err, 90) <= RT_VOXEL / 2
    # the colours come back too: the median channel difference over the covered samples is small beside the texture's range
    diff = np.abs(frames2.astype(np.int32) - frames1.astype(np.int32))[covered]
    print('median colour difference %.1f of 255' % np.median(diff))


# -- the program, and what the renderer and training make of its file ---------------------------------------------------------------------------
def _child(args, limit):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    return subprocess.run([sys.executable, '-m'] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, timeout=limit)


def test_fuse_make_then_render_make_then_training(tmp_path):
    from kfnet_amd.KFNet.pnp import write_pose
    from kfnet_amd.tools.io import read_lines
    H, W, count, voxel = RT_H, RT_W, 6, 0.08
    v, c, t = synth.synthetic_scene(3, 8)
    poses = synth.synthetic_trajectory(count, 3)
    depth, frames = gpu_render(v, c, t, poses, H, W, RT_CAM)
    seq = tmp_path / 'seq-01'
    seq.mkdir()
    for k in range(count):
        render.write_png(str(seq / ('frame-%06d.color.png' % k)), frames[k])
        render.write_png(str(seq / ('frame-%06d.depth.png' % k)), depth[k])
        write_pose(str(seq / ('frame-%06d.pose.txt' % k)), poses[k])
    flags = ['--focal_x', repr(RT_CAM['fx']), '--focal_y', repr(RT_CAM['fy']), '--u', repr(RT_CAM['u']), '--v', repr(RT_CAM['v'])]
    size = ['--height', str(H), '--width', str(W)]
    ply = str(tmp_path / 'scene.ply')
    bounds = ['-0.1', '-0.1', '-0.1', '4.1', '3.1', '2.6']
    r = _child(['kfnet_amd.fuse', 'make', '--sequence', str(seq), '--output', ply, '--voxel', repr(voxel), '--bounds'] + bounds +
               ['--min_weight', '1', '--batch', '4'] + flags + size, 300)
    assert r.returncode == 0, r.stdout
    dims, origin = M.box_lattice([float(x) for x in bounds[:3]], [float(x) for x in bounds[3:]], voxel)
    vol = M.Volume(dims, origin, voxel, None, DepthCamera(**RT_CAM), (H, W), 4)
    for at in range(0, count, 4):
        vol.integrate(depth[at:at + 4], poses[at:at + 4], frames[at:at + 4])
    mv, mc, mt = vol.mesh(1.0)
    pv, pc, pt = render.read_ply(ply)
    assert np.array_equal(pv.view(np.uint32), mv.view(np.uint32)) and np.array_equal(pc, mc) and np.array_equal(pt, mt)
    last = r.stdout.strip().split('\n')[-1]
    assert '%d voxels, %d frames used, %d vertices, %d triangles' % (dims[0] * dims[1] * dims[2], count, len(mv), len(mt)) in last
    # the default box: the padded extent of the sequence's own stride-8 labels, in this process
    cam = DepthCamera(**RT_CAM)
    paths = [str(seq / ('frame-%06d.depth.png' % k)) for k in range(count)]
    lo, hi = M.bounds_from_sequence(paths, poses, cam, (H, W), 4 * voxel, batch=4)
    lab = DepthLabeler(count, H, W, 8, cam).labels(depth, poses).cpu().numpy()
    pts = lab[..., :3][lab[..., 3] > 0]
    assert np.array_equal(lo, pts.min(axis=0).astype(np.float64) - 4 * voxel) and np.array_equal(hi, pts.max(axis=0).astype(np.float64) + 4 * voxel)
    assert (lo > -0.4).all() and (hi < np.asarray(synth.ROOM) + 0.4).all() and (hi - lo > 1.5).all()
    boxed = str(tmp_path / 'boxed.ply')
    assert M.main(['make', '--sequence', str(seq), '--output', boxed, '--voxel', repr(voxel), '--every', '2', '--no_color'] + flags + size) == 0
    bv, bc, bt = render.read_ply(boxed)
    assert len(bt) > 1000 and (bc == 255).all() and (bv.min(axis=0) >= lo - 1e-6).all()
    out = str(tmp_path / 'rendered')
    r = _child(['kfnet_amd.render', 'make', '--model', ply, '--sequence', str(seq), '--output_folder', out, '--depth_png', '--frames',
                '--batch', '4'] + flags + size, 300)
    assert r.returncode == 0, r.stdout
    for name in ('pose_list.txt', 'label_list.txt', 'depth_list.txt', 'image_list.txt'):
        assert len([x for x in read_lines(os.path.join(out, name)) if x]) == count, name
    model = tmp_path / 'model'
    r = _child(['kfnet_amd.SCoordNet.train', '--scene', 'fire', '--input_folder', out, '--height', str(H), '--width', str(W),
                '--batch', '2', '--max_steps', '2', '--snapshot', '2', '--display', '1', '--seed', '4', '--model_folder', str(model),
                '--depth'] + flags, 600)
    assert r.returncode == 0, r.stdout
    with np.load(str(model / 'kfnet_train_state-2.npz')) as st:
        assert int(st['global_step']) == 2
