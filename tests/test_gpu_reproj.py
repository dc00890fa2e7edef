"""The reprojection loss of DESIGN.md 6i on the device: kfn_reproj_loss_grad against the fp64 restatement under 6e's rule, its
exact properties, kfn_augment_pixel_map against the float32 restatement bit for bit, and whole steps of stages 1 and 3 with
the term against the existing references plus the term, under those tests' own criteria."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import augment_ref as A
import kf_train_ref as KR
import reproj_ref as RR
import test_gpu_joint_train as J3
import test_gpu_kfnet_train as K3
import test_gpu_train as G1
import test_gpu_train_f16 as H1
import train_f16_ref as HR
import train_ref as R
from gpu_util import dev, stream, sync
from kfnet_amd import _lib, reproj
from kfnet_amd.augment import ENLARGE, SHRINK, TRANSLATE, AugmentParams, descriptor
from kfnet_amd.labels import DepthCamera
from kfnet_amd.synth import synthetic_poses

pytestmark = pytest.mark.gpu

CAMERA = DepthCamera(fx=85.0, fy=80.0, u=47.5, v=31.0)          # a camera that fits the small test images
FLOOR_MARGIN = 1e-6
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def bound(e32):
    """DESIGN.md 6e's rule."""
    return max(8.0 * e32, 1e-6)


# -- the launch ------------------------------------------------------------------------------------------------------------------
def run_reproj(xs, M, labels, pm, valid, weights, ld_x, ld_dx, stride, priors=None, valid_index=3, camera=CAMERA):
    """xs: list of [B,h,w,3] float32; labels [B,h s,w s,4]; priors: list of [B,h,w,ld_dx] or None (zeros).  Returns (stats[8],
    [dx [B,h,w,ld_dx]]).  x lives in an ld_x-wide buffer whose other channels hold 7; guard rows behind every buffer."""
    lib = _lib.load()
    B, h, w, _ = xs[0].shape
    GUARD = 8
    xd, dd = [], []
    for o, x in enumerate(xs):
        xb = np.full((B * h * w + GUARD, ld_x), 7.0, np.float32)
        xb[:B * h * w, :3] = x.reshape(-1, 3)
        xd.append(dev(xb))
        db = np.zeros((B * h * w + GUARD, ld_dx), np.float32)
        if priors is not None:
            db[:B * h * w] = priors[o].reshape(-1, ld_dx)
        db[B * h * w:] = -123.0
        dd.append(dev(db))
    nll = np.full(16, -1.0, np.float32)
    nll[valid_index] = valid
    Md, ld_, nd, sd = dev(M), dev(labels), dev(nll), dev(np.full(8, -9.0, np.float32))
    pd = None if pm is None else dev(pm)
    d = reproj.descriptor(camera, B, h, w, stride, [(xd[o].data_ptr(), ld_x, dd[o].data_ptr(), ld_dx, weights[o]) for o in range(len(xs))])
    _lib.check(lib.kfn_reproj_loss_grad(C.byref(d), Md.data_ptr(), ld_.data_ptr(), None if pd is None else pd.data_ptr(),
                                        nd.data_ptr(), valid_index, sd.data_ptr(), stream()), 'kfn_reproj_loss_grad')
    sync()
    out = []
    for o in range(len(xs)):
        got = dd[o].cpu().numpy()
        assert np.all(got[B * h * w:] == -123.0), 'kfn_reproj_loss_grad wrote past the last cell'
        assert np.array_equal(xd[o].cpu().numpy()[:, 3:], np.full((B * h * w + GUARD, ld_x - 3), 7.0, np.float32))
        out.append(got[:B * h * w].reshape(B, h, w, ld_dx))
    return sd.cpu().numpy(), out


def _rigid(rng, t_scale=1.0):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = Q, t_scale * rng.normal(size=3)
    return P


def make_case(B, h, w, outputs, seed, floor_cell=True):
    """(xs float32, M float32 [B,12], mask [B,h,w], index of the cell below the floor or None).  Frame 0's camera centre sits
    at the origin of the prediction space (G c = 0), so M_0 has no translation and a tiny prediction IS a tiny camera-frame
    point, without cancellation: cell (0, 0, 1) of output 0 gets sum cam^2 = 2.9e-13 < 1e-12.  Every other point lies 0.5 .. 3
    in front of its camera, off its ray by a few degrees."""
    rng = np.random.default_rng([seed, B, h, w, outputs])
    G = _rigid(rng, 0.3)
    poses = np.stack([_rigid(rng) for _ in range(B)])
    poses[0, :3, 3] = np.linalg.inv(G)[:3, 3]
    M = reproj.pose_matrices(poses, G)
    M[0, 3::4] = 0.0                                                     # the fp64 residue of G c, ~1e-17
    M64 = M.reshape(B, 3, 4).astype(np.float64)
    rays = RR.analytic_rays(h, w, CAMERA)
    xs = []
    for o in range(outputs):
        depth = rng.uniform(0.5, 3.0, size=(B, h, w, 1))
        cam = depth * (np.concatenate([np.broadcast_to(rays, (B, h, w, 2)), np.ones((B, h, w, 1))], -1) +
                       rng.normal(scale=0.08, size=(B, h, w, 3)))
        Rm, t = M64[:, :, :3], M64[:, :, 3]
        x = np.einsum('bji,bhwj->bhwi', Rm, cam - t[:, None, None, :])    # R^T (cam - t): M is rigid
        xs.append(x.astype(np.float32))
    mask = (rng.uniform(size=(B, h, w)) < 0.7).astype(np.float32)
    mask.reshape(-1)[:4] = 1.0                                           # at least four live cells
    cell = None
    if floor_cell:
        cell = (0, 0, 1)
        xs[0][cell] = np.array([3e-7, -2e-7, 4e-7], np.float32)
    return xs, M, mask, cell


def make_labels(mask, stride, seed=0):
    """[B,h s,w s,4]: the mask at (s r, s c), ones at every other pixel (a wrong stride would count them), junk coordinates."""
    B, h, w = mask.shape
    rng = np.random.default_rng(seed)
    lab = rng.normal(size=(B, h * stride, w * stride, 4)).astype(np.float32)
    lab[..., 3] = 1.0
    lab[:, ::stride, ::stride, 3] = mask
    return lab


def sum_cam2(xs, M):
    M64 = M.reshape(-1, 3, 4).astype(np.float64)
    out = []
    for x in xs:
        cam = np.einsum('bij,bhwj->bhwi', M64[:, :, :3], x.astype(np.float64)) + M64[:, None, None, :, 3]
        out.append((cam * cam).sum(-1))
    return out


def reference(xs, M, rays, mask, weights, dtype):
    """([R per output], [weight * dR/dx per output]) by autograd in `dtype`, as float64 arrays."""
    M3 = M.reshape(-1, 3, 4)
    Rs, gs = [], []
    for x, wgt in zip(xs, weights):
        xt = torch.from_numpy(x.astype(np.float64)).to(dtype).requires_grad_(True)
        Rv, _ = RR.reproj_loss(xt, torch.from_numpy(M3.astype(np.float64)).to(dtype), torch.from_numpy(np.asarray(rays, np.float64)).to(dtype),
                               torch.from_numpy(mask.astype(np.float64)).to(dtype))
        g, = torch.autograd.grad(wgt * Rv, xt)
        Rs.append(float(Rv.item()))
        gs.append(g.to(torch.float64).numpy())
    return Rs, gs


def check_case(B, h, w, stride, ld_x, ld_dx, outputs, with_map, seed=0, rows=None):
    xs, M, mask, cell = make_case(B, h, w, outputs, seed)
    s2 = sum_cam2(xs, M)
    live = mask == 1.0
    for o in range(outputs):                             # every live cell clear of the floor, but the one placed below it
        away = np.abs(s2[o] - 1e-12) >= FLOOR_MARGIN
        if o == 0:
            assert s2[0][cell] < 1e-12 and live[cell]
            away[cell] = True
        assert away[live].all()
    pm = None
    rays = RR.analytic_rays(h, w, CAMERA)
    if with_map:
        pm = RR.pixel_map32(AugmentParams(ENLARGE, 11.0, 0.07, 0.12, 0.83), 8 * h, 8 * w, CAMERA)
        rays = pm.astype(np.float64)
    weights = [50.0, 2.0, 6.0][:outputs]
    valid = float(mask.sum() + 1.0)
    stats, dxs = run_reproj(xs, M, make_labels(mask, stride, seed), pm, valid, weights, ld_x, ld_dx, stride,
                            valid_index=3 if outputs == 1 else 10)
    R64, g64 = reference(xs, M, rays, mask, weights, torch.float64)
    R32, g32 = reference(xs, M, rays, mask, weights, torch.float32)
    assert stats[4] == valid + 1.0 and not stats[5:].any() and not stats[outputs:3].any()
    total64 = sum(wt * r for wt, r in zip(weights, R64))
    worst = (0.0, 0.0)
    for o in range(outputs):
        e, e32 = abs(stats[o] - R64[o]) / abs(R64[o]), abs(np.float32(R32[o]) - R64[o]) / abs(R64[o])
        assert e <= bound(e32), ('R', o, e, e32)
        keep = np.ones((B, h, w), bool)
        if o == 0:                                       # the cell below the floor has a gradient ~1e6 times the others':
            keep[cell] = False                           # it is compared apart, so that it does not set the scale for them
            parts = [(keep, 'cells'), (~keep, 'floor cell')]
        else:
            parts = [(keep, 'cells')]
        for sel, what in parts:
            scale = np.abs(g64[o][sel]).max()
            e = float(np.abs(dxs[o][..., :3].astype(np.float64) - g64[o])[sel].max() / scale)
            e32 = float(np.abs(g32[o] - g64[o])[sel].max() / scale)
            assert e <= bound(e32), (what, o, e, e32)
            if what == 'cells':
                worst = max(worst, (e, e32))
        assert not dxs[o][..., 3:].any()                 # channel 3 and the padding: zeros stayed zeros
        assert not dxs[o][~live].any()
    e, e32 = abs(stats[3] - total64) / abs(total64), abs(np.float32(sum(wt * r for wt, r in zip(weights, R32))) - total64) / abs(total64)
    assert e <= bound(e32)
    if rows is not None:
        rows.append((B, h, w, stride, ld_x, ld_dx, outputs, int(with_map), worst[0], worst[1]))


GRIDS = [(B, h, w) for (h, w) in ((2, 3), (5, 7), (9, 13)) for B in (1, 2)]


@pytest.mark.parametrize('grid', GRIDS, ids=['%dx%dx%d' % g for g in GRIDS])
def test_loss_and_gradients_against_fp64_autograd(grid):
    B, h, w = grid
    rows = []
    for stride in (1, 8):
        for ld_x in (4, 16):
            for ld_dx in (4, 16):
                for outputs in (1, 3):
                    for with_map in (False, True):
                        check_case(B, h, w, stride, ld_x, ld_dx, outputs, with_map, rows=rows)
    check_case(B, h, w, 1, 3, 5, 3, False, rows=rows)            # strides that rule out 16-byte words: the scalar path
    e, e32 = max(r[8] for r in rows), max(r[9] for r in rows)
    print('%dx%dx%d: %d launches, worst e device %.3e, worst e torch-fp32 %.3e' % (B, h, w, len(rows), e, e32))
    for r in rows[::11]:
        print('  B%d %dx%d stride %d ld %d/%d outputs %d map %d: e device %.3e  e torch-fp32 %.3e' % r)


def test_loss_and_gradients_where_the_workgroup_makes_several_passes():
    rows = []
    check_case(4, 60, 80, 1, 4, 16, 3, False, rows=rows)         # 19200 cells: 19 passes of the 1024 threads
    check_case(4, 60, 80, 8, 4, 4, 1, True, rows=rows)
    for r in rows:
        print('B%d %dx%d stride %d ld %d/%d outputs %d map %d: e device %.3e  e torch-fp32 %.3e' % r)


def test_gradients_are_added_to_what_the_buffers_hold_and_nothing_else_is_touched():
    B, h, w = 2, 9, 13
    for ld_x, ld_dx, stride in ((4, 16, 8), (4, 4, 1), (3, 5, 1)):
        xs, M, mask, _ = make_case(B, h, w, 3, 5)
        labels = make_labels(mask, stride)
        valid = float(mask.sum() + 1.0)
        weights = [10.0, 2.0, 2.0]
        rng = np.random.default_rng(9)
        priors = [rng.normal(size=(B, h, w, ld_dx)).astype(np.float32) for _ in range(3)]
        s0, term = run_reproj(xs, M, labels, None, valid, weights, ld_x, ld_dx, stride, None, valid_index=10)
        s1, got = run_reproj(xs, M, labels, None, valid, weights, ld_x, ld_dx, stride, priors, valid_index=10)
        s2, again = run_reproj(xs, M, labels, None, valid, weights, ld_x, ld_dx, stride, priors, valid_index=10)
        assert np.array_equal(bits(s0), bits(s1)) and np.array_equal(bits(s1), bits(s2))          # two launches, the same bits
        for o in range(3):
            assert np.abs(term[o][..., :3]).max() > 0
            want = priors[o].copy()
            want[..., :3] = priors[o][..., :3] + term[o][..., :3]                                   # one fp32 addition
            assert np.array_equal(bits(got[o][..., :3]), bits(want[..., :3]))
            assert np.array_equal(bits(got[o][..., 3:]), bits(priors[o][..., 3:]))                  # channel 3, padding
            assert np.array_equal(bits(got[o][mask != 1.0]), bits(priors[o][mask != 1.0]))          # dead cells, every channel
            assert np.array_equal(bits(again[o]), bits(got[o]))


def test_an_all_masked_batch_gives_zero_and_leaves_the_buffers():
    xs, M, mask, _ = make_case(2, 5, 7, 3, 3)
    rng = np.random.default_rng(4)
    priors = [rng.normal(size=(2, 5, 7, 16)).astype(np.float32) for _ in range(3)]
    for stride in (1, 8):
        labels = make_labels(np.zeros_like(mask), stride)
        stats, got = run_reproj(xs, M, labels, None, 1.0, [50.0, 10.0, 10.0], 4, 16, stride, priors, valid_index=10)
        assert np.array_equal(stats, np.array([0, 0, 0, 0, 2, 0, 0, 0], np.float32))
        for o in range(3):
            assert np.array_equal(bits(got[o]), bits(priors[o]))
    # a mask value other than 1 is dead, as in the NLL launch (mask == 1)
    labels = make_labels(np.full_like(mask, 0.5), 1)
    stats, _ = run_reproj(xs, M, labels, None, 1.0, [50.0, 10.0, 10.0], 4, 16, 1, priors, valid_index=10)
    assert stats[3] == 0.0


# -- the augmented pixel map -------------------------------------------------------------------------------------------------
def run_pixel_map(p, H, W, stride, camera=CAMERA):
    lib = _lib.load()
    h, w = H // stride, W // stride
    out = torch.full((h * w + 16, 2), -5.0, device='cuda')
    d = descriptor(p, 3, H, W, stride)
    u, v, ifx, ify = reproj.camera_constants(camera)
    _lib.check(lib.kfn_augment_pixel_map(C.byref(d), u, v, ifx, ify, out.data_ptr(), stream()), 'kfn_augment_pixel_map')
    sync()
    got = out.cpu().numpy()
    assert np.all(got[h * w:] == -5.0), 'kfn_augment_pixel_map wrote past the last pixel'
    return got[:h * w].reshape(h, w, 2)


PIXMAP_PARAMS = [AugmentParams(TRANSLATE, 25.0, 0.1, 0.1, 0.85), AugmentParams(ENLARGE, 19.0, 0.06, 0.12, 0.85),
                 AugmentParams(ENLARGE, 0.0, 0.15, 0.02, 0.8), AugmentParams(SHRINK, -11.0, ratio=0.86),
                 AugmentParams(SHRINK, 30.0, ratio=0.8), AugmentParams(ENLARGE, -30.0, 0.2, 0.2, 0.8)]


@pytest.mark.parametrize('size', [(64, 96), (72, 104)], ids=['64x96', '72x104'])
def test_augmented_pixel_map_equals_the_float32_restatement_bit_for_bit(size):
    H, W = size
    for p in PIXMAP_PARAMS:
        for stride in (1, 8):
            got, want = run_pixel_map(p, H, W, stride), RR.pixel_map32(p, H, W, CAMERA, stride)
            assert got.shape == want.shape
            diff = bits(got) != bits(want)
            assert not diff.any(), (p, stride, int(diff.sum()))
    default = DepthCamera()                               # the 7-Scenes intrinsics, whose centre lies outside these images
    assert np.array_equal(bits(run_pixel_map(PIXMAP_PARAMS[1], H, W, 8, default)), bits(RR.pixel_map32(PIXMAP_PARAMS[1], H, W, default, 8)))


def test_augmenter_makes_the_map_and_checks_its_buffer():
    from kfnet_amd.augment import Augmenter
    aug = Augmenter(2, 64, 96, label_stride=8)
    out = torch.zeros((8, 12, 2), device='cuda')
    aug.pixel_map(PIXMAP_PARAMS[3], CAMERA, out, stream())
    sync()
    assert np.array_equal(bits(out.cpu().numpy()), bits(RR.pixel_map32(PIXMAP_PARAMS[3], 64, 96, CAMERA, 8)))
    with pytest.raises(ValueError):
        aug.pixel_map(PIXMAP_PARAMS[3], CAMERA, torch.zeros((8, 12, 4), device='cuda'), stream())


# -- stage 1: a whole step ---------------------------------------------------------------------------------------------------
W_R = 50.0
AUGMENT = AugmentParams(ENLARGE, 19.0, 0.06, 0.12, 0.85, delta=9.5, factor=0.9)
# DESIGN.md 6f's rule for the augmented step, whose frames the existing tests' seeds do not cover: synthetic_sequence(seed)
# through AUGMENT with initial_weights(seed); of seeds 1..40 the ones whose smallest fp64 |pre-activation| over every ReLU unit
# (joint_train_ref.recorded_relu_inputs, found on the CPU) is largest: 1.9e-8 and 1.4e-8.  The plain steps run on the inputs
# of tests/test_gpu_train.py's whole step: the term leaves the forward pass, and so the pre-activations, as they are.
AUGMENTED_SEEDS = {(64, 96): 8, (72, 104): 25}


def _stage1_inputs(size, augment, seed=1):
    """(frames and labels as the trainer gets them, frames and grid labels as the network sees them, rays, M, W, poses)."""
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    from kfnet_amd.train import synthetic_labels
    from kfnet_amd.weights import initial_weights
    h, w = size[0] // 8, size[1] // 8
    frames = synthetic_sequence(2, size[0], size[1], seed=seed)
    M = synthetic_transform().astype(np.float32)
    if augment is None:
        labels = synthetic_labels(2, (h, w))
        seen_f, seen_l, rays = frames, labels, RR.analytic_rays(h, w, CAMERA)
    else:
        labels = synthetic_labels(2, size)
        seen_f, seen_l = A.augment32(frames, labels, augment, label_stride=8)
        rays = RR.pixel_map32(augment, size[0], size[1], CAMERA).astype(np.float64)
    return frames, labels, seen_f, seen_l, rays, M, initial_weights(seed if seed != 1 else 2), synthetic_poses(2)


def stage1_reference(seen_f, seen_l, rays, M, W, poses, dtype, weight=W_R, network=R.network):
    Wt = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)).to(dtype).requires_grad_(True) for k, v in W.items()
          if k.startswith('ScoreNet/')}
    pred = network(seen_f, Wt)
    h, w = pred.shape[1:3]
    lab = R.grid_labels(seen_l, (h, w))
    L, nll, sm, acc, valid = R.coord_loss(pred, lab, np.asarray(seen_f)[:, ::8, ::8][:, :h, :w], M)
    Mb = reproj.pose_matrices(poses, M).reshape(-1, 3, 4)
    Rv, _ = RR.reproj_loss(pred[..., :3], Mb, rays, (lab[..., 3] == 1.0))
    L = L + weight * Rv
    names = sorted(Wt)
    grads = torch.autograd.grad(L, [Wt[n] for n in names])
    return dict(loss=L.item(), l_reproj=Rv.item()), {n: g.detach().to(torch.float64).numpy() for n, g in zip(names, grads)}


def _worst(g, g32, g64):
    e_dev = max(float(np.abs(g[n] - g64[n]).max() / np.abs(g64[n]).max()) for n in g64)
    e_32 = max(float(np.abs(g32[n] - g64[n]).max() / np.abs(g64[n]).max()) for n in g64)
    return e_dev, e_32


@pytest.mark.parametrize('augmented', [False, True], ids=['plain', 'augmented'])
@pytest.mark.parametrize('size', [(64, 96), (72, 104)], ids=['64x96', '72x104'])
def test_stage_1_step_with_the_term_against_fp64(size, augmented):
    """The criterion of tests/test_gpu_train.py's whole step: worst e over the variables <= 4 x torch-CPU fp32's."""
    from kfnet_amd.train import SCoordNetTrainer
    p = AUGMENT if augmented else None
    frames, labels, seen_f, seen_l, rays, M, W, poses = _stage1_inputs(size, p, seed=AUGMENTED_SEEDS[size] if augmented else 1)
    tr = SCoordNetTrainer(W, image_size=size, batch=2, transform=M, base_lr=1e-4, weight_decay=1e-4, reproj_weight=W_R, camera=CAMERA)
    with pytest.raises(ValueError):
        tr.step(frames, labels, augment=p)                # no poses
    assert tr.global_step == 0
    tr.set_poses(poses)
    stats = dict(tr.step(frames, labels, augment=p))
    g = tr.gradients()
    s64, g64 = stage1_reference(seen_f, seen_l, rays, M, W, poses, torch.float64)
    s32, g32 = stage1_reference(seen_f, seen_l, rays, M, W, poses, torch.float32)
    _, plain = R.loss_and_grads(seen_f, seen_l, W, M)
    e_dev, e_32 = _worst(g, g32, g64)
    print('loss device %.7g fp64 %.7g; l_reproj device %.7g fp64 %.7g; worst e: device %.3e, torch-CPU fp32 %.3e, bound %.3e; '
          'the term moves the gradient by %.3e' % (stats['loss'], s64['loss'], stats['l_reproj'], s64['l_reproj'], e_dev, e_32,
                                                   4 * e_32, _worst(plain, plain, g64)[0]))
    assert e_dev <= 4.0 * e_32
    assert _worst(plain, plain, g64)[0] > 1e-2             # the term matters: the gradients differ from the plain loss's
    assert abs(stats['loss'] - s64['loss']) <= 1e-4 * abs(s64['loss'])
    assert abs(stats['l_reproj'] - s64['l_reproj']) <= 1e-4 * abs(s64['l_reproj'])
    assert sorted(stats) == sorted(['loss', 'l_measure', 'l_smooth', 'a_measure', 'pixels', 'lr', 'l_reproj'])
    with pytest.raises(ValueError):
        tr.step(frames, labels, augment=p)                # the poses served one step
    assert tr.global_step == 1


def test_stage_1_fp16_step_with_the_term_against_the_emulation():
    """The criterion of tests/test_gpu_train_f16.py: worst e <= 4 x the emulation's in torch-CPU fp32, with that
    test's seed and loss scale."""
    from kfnet_amd.train import SCoordNetTrainer
    size = (64, 96)
    seed, scale = H1.STEP_SEEDS[size], 2 ** 15
    frames, labels, seen_f, seen_l, rays, M, W, poses = _stage1_inputs(size, None, seed=seed)
    net = lambda f, Wt: HR.network(f, Wt, scale)
    s64, g64 = stage1_reference(seen_f, seen_l, rays, M, W, poses, torch.float64, network=net)
    s32, g32 = stage1_reference(seen_f, seen_l, rays, M, W, poses, torch.float32, network=net)
    tr = SCoordNetTrainer(W, image_size=size, batch=2, transform=M, base_lr=1e-4, weight_decay=1e-4, precision='fp16',
                          loss_scale=scale, reproj_weight=W_R, camera=CAMERA)
    tr.set_poses(poses)
    stats = dict(tr.step(frames, labels))
    e_dev, e_32 = _worst(tr.gradients(), g32, g64)
    print('fp16: loss device %.7g emulation fp64 %.7g; worst e: device %.3e, emulation in torch-CPU fp32 %.3e, bound %.3e' %
          (stats['loss'], s64['loss'], e_dev, e_32, 4 * e_32))
    assert stats['skipped'] == 0 and stats['loss_scale'] == scale
    assert e_dev <= 4.0 * e_32
    assert abs(stats['l_reproj'] - s64['l_reproj']) <= 1e-3 * abs(s64['l_reproj'])
    assert list(stats)[-3:] == ['loss_scale', 'skipped', 'l_reproj']


def test_stage_1_with_weight_zero_is_todays_trainer_bit_for_bit():
    from kfnet_amd.train import SCoordNetTrainer
    frames, labels, M = G1._batch((64, 96))
    W = G1._weights('initial')
    kw = dict(image_size=(64, 96), batch=2, transform=M, base_lr=1e-3)
    a, b = SCoordNetTrainer(W, **kw), SCoordNetTrainer(W, reproj_weight=0.0, camera=CAMERA, **kw)
    assert b.reproj is None and b.pixel_map is None
    b.set_poses(synthetic_poses(2))                       # not looked at
    for _ in range(2):
        sa, sb = dict(a.step(frames, labels)), dict(b.step(frames, labels))
        assert sorted(sa) == sorted(sb) and all(np.float64(sa[k]).tobytes() == np.float64(sb[k]).tobytes() for k in sa)
        ga, gb = a.gradients(), b.gradients()
        assert all(np.array_equal(bits(ga[k]), bits(gb[k])) for k in ga)
    wa, wb = a.weights(), b.weights()
    assert all(np.array_equal(bits(wa[k]), bits(wb[k])) for k in wa)


# -- stage 3: a whole step, OFlowNet fixed and joint ---------------------------------------------------------------------------
W3 = (50.0, 10.0, 10.0)


def _reproj_terms(pred, temp, kf, lab, M, poses, rays):
    Mb = reproj.pose_matrices(poses, M).reshape(-1, 3, 4)
    m = (lab[..., 3] == 1.0)
    return [RR.reproj_loss(t[..., :3], Mb, rays, m)[0] for t in (pred, temp, kf)]


def fixed_reference(frames, labels, W, flow, st, M, poses, rays, dtype):
    """kf_train_ref.loss_and_grads plus the three terms."""
    Wt = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)).to(dtype).requires_grad_(True) for k, v in W.items()
          if k.startswith('ScoreNet/')}
    pred = R.network(frames, Wt)
    B, h, w, _ = pred.shape
    lab = R.grid_labels(labels, (h, w))
    temp, kf = KR.filter_forward(KR.measurement(pred).reshape(1, B, h, w, 4), np.asarray(flow).reshape(1, B, h, w, 2),
                                 np.asarray(st).reshape(1, B, h, w))
    temp, kf = temp.reshape(B, h, w, 4), kf.reshape(B, h, w, 4)
    L, _, _ = KR.filter_loss(pred, temp, kf, lab, np.asarray(frames)[:, ::8, ::8][:, :h, :w], M)
    Rs = _reproj_terms(pred, temp, kf, lab, M, poses, rays)
    L = L + sum(lw * rw * r for lw, rw, r in zip(KR.LOSS_WEIGHTS, W3, Rs))
    names = sorted(Wt)
    grads = torch.autograd.grad(L, [Wt[n] for n in names])
    return dict(loss=L.item(), R=[r.item() for r in Rs]), {n: g.detach().to(torch.float64).numpy() for n, g in zip(names, grads)}


def test_stage_3_fixed_step_with_the_terms_against_fp64():
    """The criterion of tests/test_gpu_kfnet_train.py's whole step, on its inputs."""
    from kfnet_amd.train_kfnet import KFNetTrainer
    size = (64, 96)
    frames, labels, M = K3._data(size, 4)
    W = K3._weights()
    poses = synthetic_poses(4)
    rays = RR.analytic_rays(8, 12, CAMERA)
    tr = KFNetTrainer(W, image_size=size, transform=M, base_lr=1e-4, weight_decay=1e-4, reproj_weights=W3, camera=CAMERA)
    with pytest.raises(ValueError):
        tr.step(frames, labels)
    tr.set_poses(poses)
    stats = dict(tr.step(frames, labels))
    g = tr.gradients()
    dbg = tr.engine.debug(4)
    flow, st = dbg['flow'], dbg['sigma_trans']
    s64, g64 = fixed_reference(frames, labels, W, flow, st, M, poses, rays, torch.float64)
    s32, g32 = fixed_reference(frames, labels, W, flow, st, M, poses, rays, torch.float32)
    _, plain = KR.loss_and_grads(frames, labels, W, 1, 4, flow, st, M)
    e_dev, e_32 = _worst(g, g32, g64)
    print('loss device %.7g fp64 %.7g; R device %.6g %.6g %.6g fp64 %s; worst e: device %.3e, torch-CPU fp32 %.3e, bound %.3e' %
          (stats['loss'], s64['loss'], stats['l_reproj_measure'], stats['l_reproj_temp'], stats['l_reproj_kf'], s64['R'], e_dev, e_32,
           K3.bound(e_32)))
    assert e_dev <= K3.bound(e_32)
    assert _worst(plain, plain, g64)[0] > 1e-2
    assert abs(stats['loss'] - s64['loss']) <= 1e-4 * abs(s64['loss'])
    for k, want in zip(('l_reproj_measure', 'l_reproj_temp', 'l_reproj_kf'), s64['R']):
        assert abs(stats[k] - want) <= 1e-4 * abs(want)
    assert s64['R'][0] != s64['R'][1] != s64['R'][2]


def joint_reference(frames, labels, W, S, M, poses, rays, dtype):
    """joint_train_ref.loss_and_grads plus the three terms."""
    import flow_train_ref as FR
    import joint_train_ref as JR
    T = 4
    Ws = {k: JR.tensor(v, dtype, True) for k, v in W.items() if k.startswith('ScoreNet/')}
    Wf = FR.tensors(W, dtype, grad=True)
    flow, st = JR.flow_forward(frames, Wf, S, T)
    pred = R.network(frames, Ws)
    B, h, w, _ = pred.shape
    lab = R.grid_labels(labels, (h, w))
    temp, kf = JR.filter_forward(KR.measurement(pred).reshape(S, T, h, w, 4), flow, st)
    temp, kf = temp.reshape(B, h, w, 4), kf.reshape(B, h, w, 4)
    L, _, _ = KR.filter_loss(pred, temp, kf, lab, np.asarray(frames)[:, ::8, ::8][:, :h, :w], M)
    Rs = _reproj_terms(pred, temp, kf, lab, M, poses, rays)
    L = L + sum(lw * rw * r for lw, rw, r in zip(KR.LOSS_WEIGHTS, W3, Rs))
    Wall = dict(Ws)
    Wall.update(Wf)
    names = sorted(Wall)
    grads = torch.autograd.grad(L, [Wall[n] for n in names])
    return dict(loss=L.item(), R=[r.item() for r in Rs]), {n: g.detach().to(torch.float64).numpy() for n, g in zip(names, grads)}


def test_stage_3_joint_step_with_the_terms_against_fp64():
    """The criterion of tests/test_gpu_joint_train.py's whole step, per scope, on its inputs and seed."""
    size = (64, 96)
    S, frames, labels, M, W = J3._step_inputs(size)
    poses = synthetic_poses(4 * S)
    rays = RR.analytic_rays(8, 12, CAMERA)
    tr = J3._trainer(size, W, S, M, train_flownet=True, reproj_weights=W3, camera=CAMERA)
    tr.set_poses(poses)
    stats = dict(tr.step(frames, labels))
    g = tr.gradients()
    s64, g64 = joint_reference(frames, labels, W, S, M, poses, rays, torch.float64)
    s32, g32 = joint_reference(frames, labels, W, S, M, poses, rays, torch.float32)
    assert sorted(g) == sorted(g64)
    assert abs(stats['loss'] - s64['loss']) <= 1e-4 * abs(s64['loss'])
    for scope in ('ScoreNet', 'Temporal'):
        names = [n for n in g64 if n.startswith(scope + '/') and n != J3.ZERO_BY_SYMMETRY]
        e_dev, e_32 = _worst(g, g32, {n: g64[n] for n in names})
        print('%s worst e: device %.3e, torch-CPU fp32 %.3e, bound %.3e' % (scope, e_dev, e_32, K3.bound(e_32)))
        assert e_dev <= K3.bound(e_32), scope


@pytest.mark.parametrize('joint', [False, True], ids=['fixed', 'joint'])
def test_stage_3_with_weights_zero_is_todays_trainer_bit_for_bit(joint):
    size = (64, 96)
    S, frames, labels, M, W = J3._step_inputs(size)
    a = J3._trainer(size, W, S, M, train_flownet=joint)
    b = J3._trainer(size, W, S, M, train_flownet=joint, reproj_weights=(0.0, 0.0, 0.0), camera=CAMERA)
    assert b.reproj is None
    for _ in range(2):
        sa, sb = dict(a.step(frames, labels)), dict(b.step(frames, labels))
        assert sorted(sa) == sorted(sb) and all(np.float64(sa[k]).tobytes() == np.float64(sb[k]).tobytes() for k in sa)
    wa, wb = a.weights(), b.weights()
    assert all(np.array_equal(bits(wa[k]), bits(wb[k])) for k in wa)


# -- runs ----------------------------------------------------------------------------------------------------------------------
def test_ten_steps_with_the_term_follow_the_fp64_run():
    """As the existing ten-step tests: the device's loss after ten updates on one batch within 5 % of the fp64 run's."""
    from kfnet_amd.train import SCoordNetTrainer, learning_rate
    size = (64, 96)
    frames, labels, seen_f, seen_l, rays, M, W, poses = _stage1_inputs(size, None)
    tr = SCoordNetTrainer(W, image_size=size, batch=2, transform=M, base_lr=1e-4, weight_decay=1e-4, reproj_weight=W_R, camera=CAMERA)
    dev_losses = []
    for _ in range(11):
        tr.set_poses(poses)
        dev_losses.append(tr.step(frames, labels))
    dev_losses = [s['loss'] for s in dev_losses]
    ref = {k: v.copy() for k, v in W.items()}
    m = {k: np.zeros_like(v) for k, v in W.items()}
    v_ = {k: np.zeros_like(v) for k, v in W.items()}
    ref_losses = []
    for t in range(1, 12):
        s, g = stage1_reference(seen_f, seen_l, rays, M, ref, poses, torch.float64)
        ref_losses.append(s['loss'])
        lr = learning_rate(1e-4, 0.5, 80000, t - 1)
        for k in ref:
            ref[k], m[k], v_[k] = R.adam_step(ref[k], m[k], v_[k], g[k].astype(np.float32), lr, t, 1e-4)
    for i in (0, 1, 5, 10):
        print('after %2d updates: device loss %.6f, fp64 run %.6f' % (i, dev_losses[i], ref_losses[i]))
    assert ref_losses[10] < ref_losses[0]
    assert abs(dev_losses[0] - ref_losses[0]) <= 1e-4 * abs(ref_losses[0])
    assert abs(dev_losses[10] - ref_losses[10]) <= 0.05 * abs(ref_losses[10])


def test_train_command_line_with_the_term_then_eval_reads_its_snapshot_and_a_resumed_run_continues(tmp_path):
    from kfnet_amd.weights import load_npz
    one, two, out = tmp_path / 'one', tmp_path / 'two', tmp_path / 'o'
    out.mkdir()
    small = ['--height', '64', '--width', '96', '--batch', '2', '--scene', 'fire']
    run = ['--synthetic', '8', '--reproj', '--snapshot', '4', '--display', '1'] + small
    log = G1._cli('kfnet_amd.SCoordNet.train', ['--model_folder', str(one), '--max_steps', '4'] + run)
    assert sorted(os.listdir(str(one))) == ['kfnet_train_state-4.npz', 'kfnet_weights-4.npz']
    lines = [ln for ln in log.splitlines() if 'step ' in ln and 'loss=' in ln]
    assert len(lines) == 4 and all(', l_reproj=' in ln.split('sec/step)')[1] for ln in lines)
    G1._cli('kfnet_amd.SCoordNet.eval', ['--model_folder', str(one), '--synthetic', '4', '--output_folder', str(out)] + small)
    assert os.path.exists(str(out / 'coord_3.npy'))
    # two steps, then a second command that resumes and runs the other two: the same arrays
    G1._cli('kfnet_amd.SCoordNet.train', ['--model_folder', str(two), '--max_steps', '2', '--snapshot', '2'] + run[:3] + run[5:])
    log = G1._cli('kfnet_amd.SCoordNet.train', ['--model_folder', str(two), '--max_steps', '4'] + run)
    assert 'current step:  2' in log and 'Adam slots restored' in log
    a, b = load_npz(str(one / 'kfnet_weights-4.npz')), load_npz(str(two / 'kfnet_weights-4.npz'))
    assert sorted(a) == sorted(b) and all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)
