"""The reprojection loss of DESIGN.md 6i without a device: the restatements of tests/reproj_ref.py against finite
differences, the closed form and hand cases; M_b; the pixel map and its augmentation; the exports' argument checks; the
command lines, the printed lines and the sources' poses."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import reproj_ref as R
from kfnet_amd import _lib, reproj
from kfnet_amd.augment import ENLARGE, SHRINK, TRANSLATE, AugmentParams, descriptor
from kfnet_amd.labels import DepthCamera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMERA = DepthCamera(fx=85.0, fy=80.0, u=47.5, v=31.0)          # a camera that fits the small test images


def _rigid(rng, t_scale=1.0):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = Q, t_scale * rng.normal(size=3)
    return P


def _inputs(seed, B=2, h=5, w=7):
    rng = np.random.default_rng(seed)
    poses = np.stack([_rigid(rng) for _ in range(B)])
    G = _rigid(rng, 0.3)
    M = R.pose_matrices64(poses, G)
    x = rng.normal(size=(B, h, w, 3)) * 2.0
    mask = (rng.uniform(size=(B, h, w)) < 0.7).astype(np.float64)
    return x, M, R.analytic_rays(h, w, CAMERA), mask, poses, G


# -- 1. the restatement ------------------------------------------------------------------------------------------------------
def test_restatement_gradient_against_finite_differences_and_the_closed_form():
    x, M, rays, mask, _, _ = _inputs(1)
    xt = torch.from_numpy(x).requires_grad_(True)
    Rv, rho = R.reproj_loss(xt, M, rays, mask)
    g, = torch.autograd.grad(Rv, xt)
    g = g.numpy()
    vp1 = mask.sum() + 2.0
    closed = R.closed_gradient(x, M, rays) * mask[..., None] / vp1
    assert np.abs(g - closed).max() <= 1e-12 * np.abs(closed).max()
    assert abs(Rv.item() - (mask * rho.detach().numpy()).sum() / vp1) <= 1e-15
    rng = np.random.default_rng(2)
    # central differences with h = 1e-6: the two values of R each carry a few ulp of R (sums of ~100 terms: take 8 ulp), so the
    # quotient is off by 8 * 2^-52 * R / h ~ 2e-9 R; the truncation h^2 |third derivative| / 6 ~ 1e-12 is far below
    tol = 8 * 2.0 ** -52 * max(Rv.item(), 1.0) / 1e-6
    for _ in range(12):
        i = tuple(rng.integers(0, n) for n in x.shape)
        d = np.zeros_like(x)
        d[i] = 1e-6
        fd = (R.reproj_loss(torch.from_numpy(x + d), M, rays, mask)[0].item() -
              R.reproj_loss(torch.from_numpy(x - d), M, rays, mask)[0].item()) / 2e-6
        assert abs(fd - g[i]) <= tol, (i, fd, g[i])


def test_hand_cases_on_the_ray_at_a_right_angle_and_at_the_camera_centre():
    M = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None]            # world = camera
    rays = np.array([[[0.25, -0.5]]])
    one = np.ones((1, 1, 1))
    q = np.array([0.25, -0.5, 1.0])
    # a point on its own ray, at any depth
    for depth in (0.3, 1.0, 17.0):
        Rv, rho = R.reproj_loss(torch.tensor((depth * q).reshape(1, 1, 1, 3)), M, rays, one)
        assert rho.item() <= 1e-30 and Rv.item() <= 1e-30
    # a point at 90 degrees to the ray: |n1 - n2|^2 = 2
    perp = np.cross(q, [0.0, 0.0, 1.0])
    _, rho = R.reproj_loss(torch.tensor((3.0 * perp).reshape(1, 1, 1, 3)), M, rays, one)
    assert abs(rho.item() - 2.0) <= 1e-14
    # R divides by valid + 1 = sum(mask) + 2 (KFNet/KFNet.py:422, :427)
    Rv, _ = R.reproj_loss(torch.tensor((3.0 * perp).reshape(1, 1, 1, 3)), M, rays, one)
    assert abs(Rv.item() - 2.0 / 3.0) <= 1e-14
    # the camera centre: sum cam^2 = 0 <= 1e-12, n(cam) = 1e6 cam = 0, rho = |n(q)|^2 = 1; the floor's gradient 2e6 e
    x0 = torch.zeros((1, 1, 1, 3), dtype=torch.float64, requires_grad=True)
    Rv, rho = R.reproj_loss(x0, M, rays, one)
    assert abs(rho.item() - 1.0) <= 1e-15
    g, = torch.autograd.grad(Rv, x0)
    nq = q / np.linalg.norm(q)
    want = 2.0e6 * (0.0 - nq) / 3.0
    assert np.abs(g.numpy().reshape(3) - want).max() <= 1e-9 * np.abs(want).max()
    assert np.abs(R.closed_gradient(np.zeros((1, 1, 1, 3)), M, rays).reshape(3) / 3.0 - want).max() <= 1e-9 * np.abs(want).max()
    # just inside the floor the same branch: |cam|^2 = 0.81e-12
    tiny = np.array([9e-7, 0.0, 0.0]).reshape(1, 1, 1, 3)
    g = R.closed_gradient(tiny, M, rays).reshape(3)
    assert np.abs(g - 2.0e6 * (1e6 * tiny.reshape(3) - nq)).max() <= 1e-6


def test_pose_matrices_for_a_known_pose_and_transform():
    # the camera sits at (1, 2, 3) looking down world -y: camera x = world x, camera y = world z, camera z = world -y
    pose = np.array([[1.0, 0, 0, 1], [0, 0, -1, 2], [0, 1, 0, 3], [0, 0, 0, 1]])
    G = np.array([[0.0, -1, 0, 0.5], [1, 0, 0, -0.25], [0, 0, 1, 2], [0, 0, 0, 1]])
    M = reproj.pose_matrices(pose[None], G)
    assert M.dtype == np.float32 and M.shape == (1, 12)
    Xw = np.array([1.5, -2.0, 3.25, 1.0])                  # a world point in front of the camera
    cam = np.array([0.5, 0.25, 4.0])                       # by hand: R^T (X - t)
    x = G @ Xw                                             # what the training loss asks the network to predict
    assert np.abs(M.reshape(3, 4).astype(np.float64) @ x - cam).max() <= 1e-6
    assert np.array_equal(M, R.pose_matrices64(pose[None], G).reshape(1, 12).astype(np.float32))
    assert np.array_equal(reproj.pose_matrices(pose[None]), np.linalg.inv(pose)[:3].reshape(1, 12).astype(np.float32))
    with pytest.raises(ValueError):
        reproj.pose_matrices(np.zeros((2, 3, 4)))
    d = reproj.descriptor(CAMERA, 2, 5, 7, 8, [(16, 4, 32, 16, 0.5)])
    assert d.struct_size == C.sizeof(_lib.ReprojDesc) == 40 + 3 * 32 and (d.B, d.h, d.w, d.label_stride, d.outputs) == (2, 5, 7, 8, 1)
    assert (np.float32(d.u), np.float32(d.v)) == (np.float32(47.5), np.float32(31.0))
    assert (np.float32(d.inv_fx), np.float32(d.inv_fy)) == (np.float32(1 / 85.0), np.float32(1 / 80.0))
    assert (d.out[0].x, d.out[0].ld_x, d.out[0].dx, d.out[0].ld_dx, d.out[0].weight) == (16, 4, 32, 16, 0.5) and d.out[1].x is None


# -- 2. the pixel map ----------------------------------------------------------------------------------------------------------
def get_pixel_map(height, width, cam):
    """KFNet/train.py:150-166 in fp64."""
    y, x = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing='ij')
    return np.stack([(x - cam.u) / cam.fx, (y - cam.v) / cam.fy], -1)


def test_plain_pixel_map_is_the_reference_map_at_the_cells_pixels():
    H, W = 64, 96
    want = get_pixel_map(H, W, CAMERA)[::8, ::8]
    for p in (AugmentParams(TRANSLATE), AugmentParams(TRANSLATE, 25.0, 0.1, 0.1, 0.85, delta=3.0)):     # mode 0 ignores the rest
        got = R.pixel_map32(p, H, W, CAMERA)
        assert got.shape == (8, 12, 2) and got.dtype == np.float32
        # float32(1 / f) and the product: two roundings of 2^-24 relative each; x - u is exact
        assert np.all(np.abs(got - want) <= np.abs(want) * 2.0 ** -22)
        assert np.array_equal(got, R.analytic_rays(8, 12, CAMERA, np.float32))
    assert np.array_equal(R.pixel_map32(AugmentParams(TRANSLATE), H, W, CAMERA, stride=1), R.plain_map32(H, W, CAMERA)[0])
    assert np.abs(R.analytic_rays(8, 12, CAMERA) - want).max() <= 2.0 ** -22


MAX_LEFT_OUT = 0.03
# angles chosen on the CPU so that the exclusion stays under the cap (it leaves out 0.8 - 2.6 % at these, 3.3 - 5.2 % at -23)
PIXMAP_CASES = [(64, 96, ENLARGE, 11.0), (64, 96, SHRINK, -19.0), (72, 104, ENLARGE, -7.0), (72, 104, SHRINK, 29.0),
                (64, 96, ENLARGE, 0.0), (72, 104, SHRINK, 0.0)]


@pytest.mark.parametrize('case', PIXMAP_CASES, ids=['%dx%d-mode%d-%g' % c for c in PIXMAP_CASES])
def test_float32_pixel_map_against_the_fp64_passes(case):
    """Left out: only output pixels with a tap whose rotation source lies within 1e-3 of a half-integer (DESIGN.md 6c's
    exclusion), at most 3 % of them.  The bound, per value v of the map with V = max |v|, S = max(H, W), k = max(1/fx, 1/fy):
    a tap is two rounded operations (2 V 2^-24), the three interpolation steps are six more at magnitude <= V (6 V 2^-24),
    and each interpolation weight carries the error of in = o + i d, three operations at magnitude <= S (3 S 2^-24), times the
    difference D of the two values it blends -- two live taps are at most two source pixels apart after the rotation (2 k),
    but a fill tap (0) stands beside a live one at the rim of the rotated image (V): D = max(V, 2 k) -- in both steps (x 2):
    2^-24 (8 V + 6 S D)."""
    H, W, mode, angle = case
    p = AugmentParams(mode, angle, 0.07, 0.12, 0.83) if mode == ENLARGE else AugmentParams(mode, angle, ratio=0.87)
    want, left_out = R.pixel_map64(p, H, W, CAMERA)
    got = R.pixel_map32(p, H, W, CAMERA, stride=1)
    share = float(left_out.mean())
    V = float(np.abs(R.plain_map32(H, W, CAMERA)).max())
    bound = 2.0 ** -24 * (8.0 * V + 6.0 * max(H, W) * max(V, 2.0 * max(1.0 / CAMERA.fx, 1.0 / CAMERA.fy)))
    err = np.abs(got.astype(np.float64) - want).max(-1)
    print('%dx%d mode %d angle %g: left out %.2f %%, worst error %.3e, bound %.3e' % (H, W, mode, angle, 100 * share,
                                                                                    err[~left_out].max(), bound))
    assert share <= MAX_LEFT_OUT
    assert err[~left_out].max() <= bound
    assert np.array_equal(R.pixel_map32(p, H, W, CAMERA, stride=8), got[::8, ::8])
    assert np.abs(want).max() > 0.1 and (want == 0.0).all(-1).any() == (mode == SHRINK or angle != 0.0)


# -- 3. the exports --------------------------------------------------------------------------------------------------------------
def test_exports_are_in_the_binding_and_the_header_and_the_abi_number_stays():
    lib = _lib.load()
    assert lib.kfn_abi_version() == 13 == _lib.ABI_VERSION
    header = open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()
    for name in ('kfn_reproj_loss_grad', 'kfn_augment_pixel_map'):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert 'int %s(' % name in header
    assert 'KFNet/KFNet.py:405-428' in header and '#define KFN_ABI_VERSION 13' in header


def test_reproj_export_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    ARG = -1
    a = np.zeros(4096, np.float32)
    b = np.full(4096, 3.0, np.float32)
    buf, out = a.ctypes.data, b.ctypes.data
    assert buf % 16 == 0 and out % 16 == 0

    def call(B=1, h=2, w=3, stride=8, outputs=((buf, 4, out, 16, 1.0),), count=None, M=buf, labels=buf, pm=None, nll=buf, index=3,
             stats=out, **fields):
        d = reproj.descriptor(CAMERA, B, h, w, stride, list(outputs))
        if count is not None:
            d.outputs = count
        for k, v in fields.items():
            setattr(d, k, v)
        return lib.kfn_reproj_loss_grad(C.byref(d), M, labels, pm, nll, index, stats, None)
    assert call(struct_size=8) == ARG and b'struct_size' in lib.kfn_last_error()
    assert call(struct_size=C.sizeof(_lib.ReprojDesc) + 8) == ARG
    assert call(count=0) == ARG and b'outputs' in lib.kfn_last_error()
    assert call(count=4) == ARG
    assert call(outputs=()) == ARG
    for kw in (dict(M=None), dict(labels=None), dict(nll=None), dict(stats=None)):
        assert call(**kw) == ARG and b'null' in lib.kfn_last_error(), kw
    assert call(outputs=((None, 4, out, 16, 1.0),)) == ARG and call(outputs=((buf, 4, None, 16, 1.0),)) == ARG
    assert call(outputs=((buf, 4, out, 16, 1.0), (buf, 4, None, 4, 1.0))) == ARG            # the second output lacks its buffer
    assert call(outputs=((buf, 2, out, 16, 1.0),)) == ARG and b'strides' in lib.kfn_last_error()
    assert call(outputs=((buf, 4, out, 2, 1.0),)) == ARG
    for stride in (0, 2, 4, 16):
        assert call(stride=stride) == ARG and b'label_stride' in lib.kfn_last_error(), stride
    for size in (dict(B=0), dict(h=0), dict(w=-1), dict(B=4096, h=64, w=64)):
        assert call(**size) == ARG and b'grid' in lib.kfn_last_error(), size
    assert call(index=-1) == ARG
    assert call(M=buf + 4) == ARG and b'aligned' in lib.kfn_last_error()
    assert lib.kfn_reproj_loss_grad(None, buf, buf, None, buf, 3, out, None) == ARG
    assert not a.any() and np.all(b == 3.0)                                  # nothing was written

    def pm_call(p=AugmentParams(ENLARGE, 10.0, 0.1, 0.1, 0.85), size=(1, 8, 8), stride=8, dst=out, **fields):
        d = descriptor(p, size[0], size[1], size[2], stride)
        for k, v in fields.items():
            setattr(d, k, v)
        return lib.kfn_augment_pixel_map(C.byref(d), 4.0, 4.0, 0.1, 0.1, dst, None)
    for size in ((1, 8, 12), (1, 0, 8), (0, 8, 8), (1, 8, 7)):
        assert pm_call(size=size) == ARG and b'multiples of 8' in lib.kfn_last_error(), size
    for stride in (0, 2, 16):
        assert pm_call(stride=stride) == ARG and b'label_stride' in lib.kfn_last_error()
    assert pm_call(dst=None) == ARG and pm_call(dst=out + 4) == ARG
    assert pm_call(struct_size=8) == ARG and pm_call(mode=3) == ARG
    assert pm_call(p=AugmentParams(SHRINK, 0.0, ratio=0.9), new_h=9) == ARG
    assert lib.kfn_augment_pixel_map(None, 4.0, 4.0, 0.1, 0.1, out, None) == ARG
    assert np.all(b == 3.0)


# -- 4. command lines, printed lines, sources ------------------------------------------------------------------------------
def _cli(module, *args):
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    return subprocess.run([sys.executable, '-m', module] + list(args), cwd=ROOT, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=120)


def test_flags_of_the_three_training_programs():
    from kfnet_amd.KFNet.train import REPROJ_WEIGHTS, build_parser as stage3
    from kfnet_amd.OFlowNet.train import build_parser as stage2
    from kfnet_amd.SCoordNet.train import build_parser as stage1
    assert stage1().parse_args([]).reproj is None
    assert stage1().parse_args(['--reproj']).reproj == 50.0 == reproj.STAGE1_WEIGHT
    assert stage1().parse_args(['--reproj', '12.5', '--focal_x', '500']).reproj == 12.5
    a = stage3().parse_args(['--fix_flownet'])
    assert a.reproj is False and a.reproj_weights is None
    assert stage3().parse_args(['--joint', '--reproj']).reproj is True
    assert stage3().parse_args(['--joint', '--reproj_weights', '1', '2', '3', '--u', '300']).reproj_weights == [1.0, 2.0, 3.0]
    assert REPROJ_WEIGHTS == (50.0, 10.0, 10.0) == reproj.STAGE3_WEIGHTS
    with pytest.raises(SystemExit):
        stage3().parse_args(['--joint', '--reproj', '5'])               # stage 3's flag takes no number
    with pytest.raises(SystemExit):
        stage2().parse_args(['--reproj'])                               # stage 2 has no reprojection term
    for module in ('kfnet_amd.SCoordNet.train', 'kfnet_amd.KFNet.train'):
        r = _cli(module, '--help')
        assert r.returncode == 0 and '--reproj' in r.stdout and 'KFNet/KFNet.py:405-428' in r.stdout and '--focal_x' in r.stdout
    assert '--reproj_weights' in _cli('kfnet_amd.KFNet.train', '--help').stdout


def test_command_lines_refuse_a_negative_weight_and_a_folder_without_poses(tmp_path):
    common = ['--scene', 'fire', '--model_folder', str(tmp_path / 'm'), '--input_folder', str(tmp_path), '--height', '64', '--width', '96']
    r = _cli('kfnet_amd.SCoordNet.train', *(common + ['--reproj', '-1']))
    assert r.returncode == 1 and r.stderr.strip().count('\n') == 0 and '--reproj' in r.stderr
    r = _cli('kfnet_amd.KFNet.train', *(common + ['--fix_flownet', '--reproj_weights', '1', '-2', '3']))
    assert r.returncode == 1 and r.stderr.strip().count('\n') == 0 and '--reproj_weights' in r.stderr
    (tmp_path / 'image_list.txt').write_text(''.join(str(tmp_path / ('%d.png' % i)) + '\n' for i in range(4)))
    (tmp_path / 'label_list.txt').write_text(''.join(str(tmp_path / ('%d.bin' % i)) + '\n' for i in range(4)))
    (tmp_path / 'transform.txt').write_text('1 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 0 1\n')
    for module, extra in (('kfnet_amd.SCoordNet.train', ['--reproj']), ('kfnet_amd.KFNet.train', ['--fix_flownet', '--reproj']),
                          ('kfnet_amd.KFNet.train', ['--joint', '--reproj_weights', '5', '0', '0'])):
        r = _cli(module, *(common + extra))
        assert r.returncode == 1 and 'pose_list.txt' in r.stderr and r.stderr.strip().count('\n') == 0, (module, r.stderr)
        assert not (tmp_path / 'm').exists()


def test_printed_lines_with_and_without_the_term():
    from kfnet_amd.KFNet.train import format_line as line3
    from kfnet_amd.SCoordNet.train import format_line as line1
    s = dict(loss=1.5, l_measure=1.0, l_smooth=0.01, a_measure=0.25, pixels=90.0, lr=1e-4)
    plain = line1('now', 0, 3, 9, s, 0.5)
    assert 'l_reproj' not in plain and plain.endswith('(0.500 sec/step)')
    on = line1('now', 0, 3, 9, dict(s, l_reproj=0.12345), 0.5)
    assert on == plain + ', l_reproj=0.123'
    both = line1('now', 0, 3, 9, dict(s, l_reproj=0.5, loss_scale=1024.0, skipped=2), 0.5)
    assert both == plain + ', loss_scale=1024, skipped=2, l_reproj=0.500'
    s3 = dict(loss=1.5, l_measure=1.0, l_temp=1.1, l_KF=0.9, a_measure=0.25, a_temp=0.2, a_KF=0.3, pixels=90.0, lr=1e-4)
    plain = line3('now', 0, 3, 9, [4, 5, 6, 7], s3, 0.5)
    assert 'l_reproj' not in plain
    on = line3('now', 0, 3, 9, [4, 5, 6, 7], dict(s3, l_reproj_measure=0.1, l_reproj_temp=0.2, l_reproj_kf=0.3), 0.5)
    assert on == plain + ', l_reproj=0.100~0.200~0.300'


def test_step_stats_keys_and_trainer_keywords():
    import inspect
    from kfnet_amd.train import SCoordNetTrainer, StepStats
    from kfnet_amd.train_kfnet import KFNetTrainer, StepStats as StepStats3
    z = torch.zeros(16)
    assert StepStats(z, 1e-4).keys() == list(StepStats.KEYS) and 'l_reproj' not in StepStats.KEYS
    r = torch.tensor([0.25, 0.0, 0.0, 12.5, 9.0, 0.0, 0.0, 0.0])
    s = StepStats(torch.tensor([1.0, 0.0, 0.5, 8.0, 2.0, 0.0, 0.0, 0.0]), 1e-4, None, r)
    assert s.keys() == list(StepStats.KEYS) + ['l_reproj'] and s['l_reproj'] == 0.25 and s['loss'] == 14.5 and s['pixels'] == 7.0
    s3 = StepStats3(z, 1e-4, 4)
    assert s3.keys() == list(StepStats3.KEYS)
    z3 = torch.zeros(16)
    z3[0] = 2.0
    s3 = StepStats3(z3, 1e-4, 4, torch.tensor([0.1, 0.2, 0.3, 1.5, 9.0, 0.0, 0.0, 0.0]))
    assert s3.keys()[-3:] == ['l_reproj_measure', 'l_reproj_temp', 'l_reproj_kf']
    assert (np.float32(s3['l_reproj_measure']), np.float32(s3['l_reproj_temp']), np.float32(s3['l_reproj_kf'])) == \
        (np.float32(0.1), np.float32(0.2), np.float32(0.3)) and s3['loss'] == 3.5
    p = inspect.signature(SCoordNetTrainer.__init__).parameters
    assert p['reproj_weight'].default == 0.0 and p['camera'].default is None
    p = inspect.signature(KFNetTrainer.__init__).parameters
    assert p['reproj_weights'].default is None and p['camera'].default is None
    assert hasattr(SCoordNetTrainer, 'set_poses') and hasattr(KFNetTrainer, 'set_poses')
    assert reproj.check_weights(50, 1) == (50.0,) and reproj.check_weights([1, 2, 3], 3) == (1.0, 2.0, 3.0)
    for bad, n in ((-1.0, 1), (float('nan'), 1), ([1, 2], 3), ([1, -2, 3], 3)):
        with pytest.raises(ValueError):
            reproj.check_weights(bad, n)


def _write_pose(path, P):
    np.savetxt(str(path), P)


def test_sources_carry_the_poses(tmp_path):
    from kfnet_amd.batches import LabelFileSource, SyntheticSource
    from kfnet_amd.synth import synthetic_poses
    src = SyntheticSource(6, (64, 96))
    assert src.poses.shape == (6, 4, 4) and np.array_equal(src.poses, synthetic_poses(6))
    for P in src.poses:                                                  # rigid
        assert np.abs(P[:3, :3] @ P[:3, :3].T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(P[:3, :3]) - 1.0) <= 1e-12
        assert np.array_equal(P[3], [0.0, 0.0, 0.0, 1.0])
    assert np.array_equal(synthetic_poses(2, start=3), synthetic_poses(6)[3:5]) and not np.array_equal(src.poses[0], src.poses[1])
    (tmp_path / 'image_list.txt').write_text(''.join(str(tmp_path / ('%d.png' % i)) + '\n' for i in range(3)))
    (tmp_path / 'label_list.txt').write_text(''.join(str(tmp_path / ('%d.bin' % i)) + '\n' for i in range(3)))
    (tmp_path / 'transform.txt').write_text('1 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 0 1\n')
    assert LabelFileSource(str(tmp_path), (64, 96)).poses is None         # not asked to: the file is not looked for
    with pytest.raises(ValueError, match='pose_list.txt'):
        LabelFileSource(str(tmp_path), (64, 96), needs_poses=True)
    rng = np.random.default_rng(5)
    poses = np.stack([_rigid(rng) for _ in range(3)])
    for i, P in enumerate(poses):
        _write_pose(tmp_path / ('%d.pose.txt' % i), P)
    (tmp_path / 'pose_list.txt').write_text(''.join(str(tmp_path / ('%d.pose.txt' % i)) + '\n' for i in range(3)))
    got = LabelFileSource(str(tmp_path), (64, 96), needs_poses=True).poses
    assert got.shape == (3, 4, 4) and np.abs(got - poses).max() <= 1e-6
    (tmp_path / 'pose_list.txt').write_text(''.join(str(tmp_path / ('%d.pose.txt' % i)) + '\n' for i in range(2)))
    with pytest.raises(ValueError, match='lists 2 poses for 3 images'):
        LabelFileSource(str(tmp_path), (64, 96), needs_poses=True)
