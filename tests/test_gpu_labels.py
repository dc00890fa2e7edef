"""Labels from depth maps on the device (kfn_depth_labels, kfn_label_moments) against the restatements of
tests/labels_ref.py: the label kernel bit for bit at every pixel, the moments within the summation bound, the closure with
the pose stage, `labels make` end to end, and training from its files against training with --depth."""
import ctypes as C
import os

import numpy as np
import pytest

import labels_ref as R
from kfnet_amd import _lib
from kfnet_amd import labels as L
from kfnet_amd.labels import DepthCamera, DepthLabeler, decorrelating_transform

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 8), (3, 24, 40), (2, 64, 96)]      # a single grid cell; partial waves, no power of two; several workgroups
SENTINEL = -12345.5
GUARD = 64                                          # pixels of guard rows behind the output tensor


def _camera(H, W, registered):
    """A short focal length so that the small test images see a wide field, and a depth camera whose columns leave the
    image on both sides.  ud = u + 1.5 puts colour column u exactly on a half (0 * kx + ud): the tie goes away from zero."""
    if not registered:
        return DepthCamera(40., 42., W / 2.0, H / 2.0)
    return DepthCamera(40., 42., W / 2.0, H / 2.0, depth_fx=47., depth_fy=45., depth_u=W / 2.0 + 1.5, depth_v=H / 2.0 - 0.5)


_inputs_cache = {}


def _inputs(shape):
    if shape not in _inputs_cache:
        rng = np.random.default_rng(sum(shape))
        depth = R.random_depth(rng, *shape)
        poses = np.stack([R.random_pose(rng) for _ in range(shape[0])])
        depth.setflags(write=False)
        poses.setflags(write=False)
        _inputs_cache[shape] = (depth, poses)
    return _inputs_cache[shape]


def _launch(depth, poses, cam, stride, ld=4):
    """kfn_depth_labels straight on the library: (labels [B,h,w,ld], guard [GUARD,ld]) with the sentinel wherever the kernel
    must not write."""
    import torch
    lib = _lib.load()
    B, H, W = depth.shape
    h, w = H // stride, W // stride
    dev_depth = torch.from_numpy(np.array(depth).view(np.int16)).cuda()
    dev_poses = torch.from_numpy(L.pose_rows(poses)).cuda()
    out = torch.full((B * h * w + GUARD, ld), SENTINEL, dtype=torch.float32, device='cuda')
    d = cam.descriptor(B, H, W, stride, ld_out=ld)
    _lib.check(lib.kfn_depth_labels(C.byref(d), dev_depth.data_ptr(), dev_poses.data_ptr(), out.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream), 'kfn_depth_labels')
    host = out.cpu().numpy()
    return host[:B * h * w].reshape(B, h, w, ld), host[B * h * w:]


@pytest.mark.parametrize('ld', [4, 6])
@pytest.mark.parametrize('registered', [False, True], ids=['plain', 'registered'])
@pytest.mark.parametrize('stride', [1, 8])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_depth_labels_equal_the_float32_restatement_bit_for_bit(shape, stride, registered, ld):
    depth, poses = _inputs(shape)
    cam = _camera(shape[1], shape[2], registered)
    want = R.labels32(depth, poses, cam, stride)
    got, guard = _launch(depth, poses, cam, stride, ld)
    assert np.array_equal(got[..., :4].view(np.uint32), want.view(np.uint32))
    assert np.all(got[..., 4:] == SENTINEL) and np.all(guard == SENTINEL)
    valid = want[..., 3].mean()
    if shape != SHAPES[0] or stride == 1:
        assert 0.2 < valid < 0.85, valid                      # both branches are taken
    if registered and stride == 1:
        # pixels that leave the depth image exist on this camera, and the tie column reads depth column u + 2
        x, y, xd, yd, ok_x, ok_y = R.depth_pixels(cam, shape[1], shape[2], 1, np.float32)
        assert not ok_x.all() and ok_x.any() and xd[shape[2] // 2] == shape[2] // 2 + 2


def test_a_frame_alone_equals_the_frame_in_a_batch_and_launches_repeat():
    depth, poses = _inputs(SHAPES[1])
    for registered in (False, True):
        cam = _camera(24, 40, registered)
        for stride in (1, 8):
            whole, _ = _launch(depth, poses, cam, stride)
            again, _ = _launch(depth, poses, cam, stride)
            assert np.array_equal(whole.view(np.uint32), again.view(np.uint32))
            for b in range(depth.shape[0]):
                alone, _ = _launch(depth[b:b + 1], poses[b:b + 1], cam, stride)
                assert np.array_equal(alone[0].view(np.uint32), whole[b].view(np.uint32))


def test_labeler_takes_arrays_and_tensors_and_short_batches():
    import torch
    depth, poses = (np.array(x) for x in _inputs(SHAPES[2]))
    cam = _camera(64, 96, False)
    lab = DepthLabeler(4, 64, 96, 8, cam)
    want = R.labels32(depth, poses, cam, 8)
    a = lab.labels(depth, poses).cpu().numpy()
    assert a.shape == (2, 8, 12, 4) and np.array_equal(a.view(np.uint32), want.view(np.uint32))
    dev = torch.from_numpy(np.array(depth).view(np.int16)).cuda()
    b = lab.labels(dev, torch.from_numpy(L.pose_rows(poses)).cuda()).cpu().numpy()
    c = lab.labels(dev.view(torch.uint16), torch.from_numpy(np.array(poses))).cpu().numpy()
    assert np.array_equal(a, b) and np.array_equal(a, c)
    for bad in (depth[:, :32], depth.astype(np.int32), np.concatenate([depth] * 3)):
        with pytest.raises(ValueError):
            lab.labels(bad, poses)
    with pytest.raises(ValueError):
        DepthLabeler(1, 60, 96)


# -- moments -------------------------------------------------------------------------------------------------------------------
def _moments(labels_host, pivot, ld):
    import torch
    B, h, w, _ = labels_host.shape
    padded = np.full((B, h, w, ld), SENTINEL, np.float32)
    padded[..., :4] = labels_host
    lab = DepthLabeler(B, 8, 8, 8)
    return lab.moments(torch.from_numpy(padded).cuda(), pivot).cpu().numpy()


@pytest.mark.parametrize('ld', [4, 6])
@pytest.mark.parametrize('shape,stride', [((3, 24, 40), 1), ((2, 64, 96), 1), ((2, 64, 96), 8)])
def test_label_moments_within_the_summation_bound_of_numpy_fp64(shape, stride, ld):
    """|sum - reference| <= 2 n 2^-53 sum |term|: the bound of a sum of n terms in any order, doubled for a fused product.  The
    middle frame of three has no valid pixel."""
    depth, poses = _inputs(shape)
    depth = depth.copy()
    if shape[0] == 3:
        depth[1] = 0
    labels = R.labels32(depth, poses, _camera(shape[1], shape[2], False), stride)
    pivot = np.asarray(poses[0][:3, 3])                      # the first frame's camera centre
    got = _moments(labels, pivot, ld)
    again = _moments(labels, pivot, ld)
    want, mags, counts = R.moments64(labels, pivot)
    assert got.shape == (shape[0], 10) and got.dtype == np.float64
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    assert np.array_equal(got[:, 0], counts) and counts.max() > 0
    lim = 2.0 * counts[:, None] * 2.0 ** -53 * mags
    print('largest error / bound: %.3f' % float((np.abs(got - want) / np.maximum(lim, 1e-300)).max()))
    assert np.all(np.abs(got - want) <= lim)
    if shape[0] == 3:
        assert counts[1] == 0 and np.all(got[1] == 0.0)


# -- closure with the pose stage ---------------------------------------------------------------------------------------------
def test_labels_at_stride_8_give_the_pose_back_through_pnp():
    """Labels of a few tilted planes under a random pose, handed to the RANSAC-PnP stage as confident records: it observes
    cell (r, c) at pixel (8c, 8r), so it returns the pose only if the labels belong to exactly those pixels.  Thresholds of
    test_gpu_pnp.py::test_noise_free_all_inliers."""
    import torch
    from kfnet_amd.KFNet import pnp
    cam = DepthCamera()
    rng = np.random.default_rng(11)
    pose = R.random_pose(rng)
    depth = R.plane_depth(480, 640, cam, [(2.0, 0.8, -0.5), (3.0, -1.0, 0.4), (1.5, 0.3, 0.9)])[None]
    lab = DepthLabeler(1, 480, 640, 8, cam).labels(depth, pose[None])
    assert tuple(lab.shape) == (1, 60, 80, 4) and bool((lab[..., 3] == 1).all())
    rec = lab.clone()
    rec[..., 3] = 1000.0
    poses, info = pnp.PnPSolver(60, 80).solve(rec)
    rot, trans = pnp.pose_errors(poses.cpu().numpy(), pose[None])
    info = info.cpu().numpy()
    print('rotation error %.3g deg, centre error %.3g m, inliers %d' % (rot.max(), trans.max(), info[0, 2]))
    assert (info[:, 0] == _lib.PNP_OK).all() and (info[:, 1] == 4800).all()
    assert rot.max() < 1e-2 and trans.max() < 1e-3, (rot, trans)


# -- labels make, and training from its files against training with --depth ----------------------------------------------------
H, W, FRAMES = 64, 96, 5


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    """A sequence folder of five 64x96 frames (synthetic images, plane depth maps with invalid pixels, random poses) and
    what `labels make` writes from it."""
    from kfnet_amd.synth import synthetic_sequence
    root = tmp_path_factory.mktemp('labels')
    seq, out = root / 'seq', root / 'in'
    seq.mkdir()
    cam = DepthCamera(80., 80., 48., 32.)
    rng = np.random.default_rng(21)
    depth = np.stack([R.plane_depth(H, W, cam, [(1.0 + 0.2 * i, 0.5, -0.3), (2.0, -0.6, 0.2 * i)]) for i in range(FRAMES)])
    depth[rng.random(depth.shape) < 0.1] = 0
    depth[:, 5, 7] = 65535
    base = R.random_pose(rng)
    poses = []
    for i in range(FRAMES):                                  # a camera that drifts: one scene seen from nearby places
        T = base.copy()
        T[:3, 3] += 0.05 * i * np.array([1.0, -0.5, 0.2])
        poses.append(T)
    R.write_sequence(str(seq), depth, np.stack(poses), synthetic_sequence(FRAMES, H, W))
    flags = ['--focal_x', '80', '--focal_y', '80', '--u', '48', '--v', '32', '--height', str(H), '--width', str(W)]
    assert L.main(['make', '--sequence', str(seq), '--output_folder', str(out), '--batch', '2'] + flags) == 0
    return dict(seq=seq, out=out, cam=cam, depth=depth, flags=flags)


def test_labels_make_end_to_end(dataset):
    out, cam = dataset['out'], dataset['cam']
    assert sorted(os.listdir(str(out))) == ['depth_list.txt', 'image_list.txt', 'label_list.txt', 'labels', 'pose_list.txt',
                                            'transform.txt']
    triples = L.read_sequence(str(out))
    assert triples == [tuple(os.path.abspath(p) for p in t) for t in L.read_sequence(str(dataset['seq']))]
    label_paths = [x for x in open(str(out / 'label_list.txt')).read().split('\n') if x]
    assert label_paths == [os.path.abspath(str(out / 'labels' / ('label_%d.bin' % i))) for i in range(FRAMES)]
    poses = L.read_poses([t[2] for t in triples])             # what the text files hold: %.9e of the fp64 poses
    assert np.array_equal(L.load_depth([t[1] for t in triples], (H, W)), dataset['depth'])
    want = R.labels32(dataset['depth'], poses, cam, 1)
    for i, p in enumerate(label_paths):
        got = np.fromfile(p, dtype=np.float32)
        assert got.size == H * W * 4 and np.array_equal(got.view(np.uint32), want[i].reshape(-1).view(np.uint32))
    pivot = poses[0, :3, 3]
    sums, _, counts = R.moments64(R.labels32(dataset['depth'], poses, cam, 8), pivot)
    M = decorrelating_transform(L.add_frames(None, sums), pivot)
    got = np.loadtxt(str(out / 'transform.txt'))
    assert counts.sum() > 300 and got.shape == (4, 4)
    assert np.abs(got - M).max() <= 1e-6 * np.abs(M).max()
    # --no_labels: the lists and the same transform, no label files
    bare = out.parent / 'bare'
    assert L.main(['make', '--sequence', str(dataset['seq']), '--output_folder', str(bare), '--no_labels'] + dataset['flags']) == 0
    assert sorted(os.listdir(str(bare))) == ['depth_list.txt', 'image_list.txt', 'pose_list.txt', 'transform.txt']
    assert open(str(bare / 'transform.txt')).read() == open(str(out / 'transform.txt')).read()


@pytest.mark.parametrize('augment', [False, True], ids=['plain', 'augment'])
def test_training_with_depth_equals_training_from_the_label_files(dataset, tmp_path, augment):
    import torch
    from kfnet_amd.SCoordNet import train as T
    common = ['--scene', 'fire', '--input_folder', str(dataset['out']), '--height', str(H), '--width', str(W), '--batch', '2',
              '--max_steps', '2', '--snapshot', '2', '--display', '1', '--seed', '4'] + (['--augment'] if augment else [])
    files, depth = tmp_path / 'files', tmp_path / 'depth'
    assert T.main(common + ['--model_folder', str(files)]) == 0
    assert T.main(common + ['--model_folder', str(depth), '--depth', '--focal_x', '80', '--focal_y', '80', '--u', '48',
                            '--v', '32']) == 0
    for name in ('kfnet_weights-2.npz', 'kfnet_train_state-2.npz'):
        with np.load(str(files / name)) as a, np.load(str(depth / name)) as b:
            assert sorted(a.files) == sorted(b.files) and len(a.files) >= 24
            for k in a.files:
                assert torch.equal(torch.from_numpy(np.asarray(a[k])), torch.from_numpy(np.asarray(b[k]))), (name, k)
    with np.load(str(files / 'kfnet_train_state-2.npz')) as st:
        assert int(st['global_step']) == 2
        assert any(np.abs(st[k]).max() > 0 for k in st.files if k.startswith('adam_m/'))       # the steps did learn
