"""Training SCoordNet on the device (DESIGN.md "Training"): every new entry point against fp64 (torch-CPU autograd through
the oracle's conv_same, tests/train_ref.py), the whole network's gradients and Adam step, learning on a fixed batch,
bit-reproducibility, resuming from snapshots, and the command line."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import conv_tol
import train_ref as R
from gpu_util import dev, stream, sync
from kfnet_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (64, 96)


# -- 1. weight gradients ---------------------------------------------------------------------------------------------------
def wgrad_bound(x, dz, pixels):
    """tests/conv_tol's model with the pixel count as the accumulation length."""
    rx = float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))
    rz = float(np.sqrt(np.mean(np.square(np.asarray(dz, np.float64)))))
    return conv_tol.A['direct'] * np.sqrt(1.0 + pixels / 256.0) * conv_tol.EPS32 * np.sqrt(pixels) * rx * rz + 1e-9


def run_wgrad(x, dz, k, stride, ldx_pad, ldz_pad):
    import torch
    lib = _lib.load()
    n, h, w, ci = x.shape
    _, ho, wo, co = dz.shape
    ldx, ldz = ci + ldx_pad, co + ldz_pad
    xb = np.full((n * h * w, ldx), 7.0, np.float32)
    xb[:, :ci] = x.reshape(-1, ci)
    zb = np.full((n * ho * wo, ldz), -3.0, np.float32)
    zb[:, :co] = dz.reshape(-1, co)
    d = _lib.ConvDesc(N=n, H=h, W=w, Cin=ci, ldx=ldx, Cout=co, cout_pad=-(-co // 32) * 32, ldy=ldz, kh=k, kw=k, stride=stride)
    nb = C.c_size_t()
    _lib.check(lib.kfn_conv2d_grad_weights_workspace_bytes(C.byref(d), C.byref(nb)), 'workspace bytes')
    G = 64
    ws = torch.full((nb.value // 4 + G,), -9.0, device='cuda')
    dw = torch.full((k * k * ci * co + G,), -5.0, device='cuda')
    db = torch.full((co + G,), -5.0, device='cuda')
    xd, zd = dev(xb), dev(zb)
    _lib.check(lib.kfn_conv2d_grad_weights(C.byref(d), xd.data_ptr(), zd.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                           stream()), 'kfn_conv2d_grad_weights')
    sync()
    dwh, dbh, wsh = dw.cpu().numpy(), db.cpu().numpy(), ws.cpu().numpy()
    assert np.all(dwh[-G:] == -5.0) and np.all(dbh[-G:] == -5.0), 'wrote past dw / db'
    assert np.all(wsh[-G:] == -9.0), 'wrote past the workspace'
    return dwh[:-G].reshape(k, k, ci, co), dbh[:-G]


# (layer, kernel, Cin, Cout, stride, input H, W at 480x640)
WGRAD_LAYERS = [('conv1b', 3, 64, 64, 1, 480, 640), ('conv2a', 3, 64, 256, 2, 480, 640), ('conv3b', 3, 512, 512, 1, 120, 160),
                ('conv4b', 3, 1024, 1024, 1, 60, 80), ('conv7', 1, 256, 128, 1, 60, 80), ('prediction', 1, 128, 4, 1, 60, 80)]


@pytest.mark.parametrize('small', [True, False], ids=['9x13', '480x640'])
@pytest.mark.parametrize('layer', WGRAD_LAYERS, ids=[l[0] for l in WGRAD_LAYERS])
def test_conv_weight_gradient_against_fp64(layer, small):
    name, k, ci, co, s, h, w = layer
    n = 1
    if small:
        n, h, w = 2, 9, 13
    rng = np.random.default_rng([WGRAD_LAYERS.index(layer), int(small)])
    x = rng.normal(size=(n, h, w, ci)).astype(np.float32)
    x = np.maximum(x, 0) if name != 'conv1b' else x                    # layer inputs are post-ReLU
    ho, wo = -(-h // s), -(-w // s)
    dz = rng.normal(size=(n, ho, wo, co)).astype(np.float32)
    # wider buffers; the small cases also take the unaligned dZ path (ldz % 4 != 0)
    dw, db = run_wgrad(x, dz, k, s, 16, 3 if small else 4)
    rw, rb = R.conv_grad_weights(x, dz, (k, k, ci, co), s)
    P = n * ho * wo
    bound = wgrad_bound(x, dz, P)
    err = float(np.abs(dw - rw).max())
    conv_tol.record('wgrad', '%s %dx%dx%d' % (name, n, h, w), err, bound)
    assert err <= bound
    bb = wgrad_bound(np.ones(1), dz, P)
    eb = float(np.abs(db - rb).max())
    conv_tol.record('wgrad', '%s %dx%dx%d bias' % (name, n, h, w), eb, bb)
    assert eb <= bb


@pytest.mark.parametrize('shape', [(1, 480, 640), (2, 9, 13)], ids=['480x640', '9x13'])
def test_first_conv_weight_gradient_against_fp64(shape):
    import torch
    lib = _lib.load()
    n, h, w = shape
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, size=(n, h, w, 3)).astype(np.uint8)
    dz = rng.normal(size=(n, h, w, 64)).astype(np.float32)
    nb = C.c_size_t()
    _lib.check(lib.kfn_first_conv_u8_grad_weights_workspace_bytes(n, h, w, 64, C.byref(nb)), 'workspace bytes')
    G = 64
    ws = torch.full((nb.value // 4 + G,), -9.0, device='cuda')
    dw = torch.full((27 * 64 + G,), -5.0, device='cuda')
    db = torch.full((64 + G,), -5.0, device='cuda')
    imd, zd = dev(img), dev(dz)
    _lib.check(lib.kfn_first_conv_u8_grad_weights(imd.data_ptr(), n, h, w, zd.data_ptr(), 64, dw.data_ptr(), db.data_ptr(),
                                                  ws.data_ptr(), stream()), 'kfn_first_conv_u8_grad_weights')
    sync()
    dwh, dbh = dw.cpu().numpy(), db.cpu().numpy()
    assert np.all(dwh[-G:] == -5.0) and np.all(dbh[-G:] == -5.0) and np.all(ws.cpu().numpy()[-G:] == -9.0)
    x = (img.astype(np.float64) - 128.0) * 0.00625
    rw, rb = R.conv_grad_weights(x, dz, (3, 3, 3, 64), 1)
    P = n * h * w
    bound = wgrad_bound(x, dz, P)
    err = float(np.abs(dwh[:-G].reshape(3, 3, 3, 64) - rw).max())
    conv_tol.record('wgrad', 'conv1a %dx%dx%d' % shape, err, bound)
    assert err <= bound
    bb = wgrad_bound(np.ones(1), dz, P)
    eb = float(np.abs(dbh[:-G] - rb).max())
    conv_tol.record('wgrad', 'conv1a %dx%dx%d bias' % shape, eb, bb)
    assert eb <= bb


def test_relu_gradient_in_wider_buffers():
    import torch
    lib = _lib.load()
    rng = np.random.default_rng(5)
    P, Cc = 1000, 48
    y = np.maximum(rng.normal(size=(P, Cc + 8)), 0).astype(np.float32)
    g = rng.normal(size=(P, Cc + 4)).astype(np.float32)
    yd, gd = dev(y), dev(g)
    _lib.check(lib.kfn_relu_grad(yd.data_ptr(), Cc + 8, gd.data_ptr(), Cc + 4, P, Cc, stream()), 'kfn_relu_grad')
    sync()
    want = g.copy()
    want[:, :Cc] = np.where(y[:, :Cc] > 0, g[:, :Cc], 0)
    assert np.array_equal(gd.cpu().numpy(), want)


# -- 2. input gradients on the forward kernels, with the device-made packs ---------------------------------------------------
def run_input_grad(dz, w, stride, in_hw):
    """d/dx of conv_same(x, w) for dz [N,Ho,Wo,co]: kfn_pack_conv_weights + kfn_conv2d_nhwc, as kfnet_amd.train does."""
    import torch
    lib = _lib.load()
    k, _, ci, co = w.shape
    n, ho, wo, _ = dz.shape
    c16 = -(-co // 16) * 16
    kind = _lib.PACK_INPUT_GRAD_S2 if stride == 2 else _lib.PACK_INPUT_GRAD_S1
    nf = C.c_size_t()
    _lib.check(lib.kfn_pack_conv_weights_floats(k, k, ci, co, kind, C.byref(nf)), 'pack floats')
    G = 64
    pack = torch.full((nf.value + G,), -7.0, device='cuda')
    wd = dev(w)
    _lib.check(lib.kfn_pack_conv_weights(wd.data_ptr(), k, k, ci, co, kind, pack.data_ptr(), stream()), 'kfn_pack_conv_weights')
    zb = np.zeros((n * ho * wo, c16), np.float32)
    zb[:, :co] = dz.reshape(-1, co)
    zd = dev(zb)
    H, Wd = in_hw
    out = torch.full((n * H * Wd + G, ci), -5.0, device='cuda')
    d = _lib.ConvDesc(N=n, H=ho, W=wo, Cin=c16, ldx=c16, Cout=ci, cout_pad=-(-ci // 32) * 32, ldy=ci, kh=k, kw=k,
                      stride=stride, transposed=int(stride == 2))
    _lib.check(lib.kfn_conv2d_nhwc(C.byref(d), zd.data_ptr(), pack.data_ptr(), None, out.data_ptr(), stream()), 'kfn_conv2d_nhwc')
    sync()
    assert np.all(pack.cpu().numpy()[-G:] == -7.0), 'the pack kernel wrote past its matrix'
    oh = out.cpu().numpy()
    assert np.all(oh[n * H * Wd:] == -5.0)
    return oh[:n * H * Wd].reshape(n, H, Wd, ci)


def test_forward_pack_equals_the_host_pack():
    import torch
    from kfnet_amd.graph import pack_conv_kernel
    lib = _lib.load()
    rng = np.random.default_rng(1)
    for k, ci, co in ((3, 64, 256), (1, 128, 4), (3, 16, 40)):
        w = rng.normal(size=(k, k, ci, co)).astype(np.float32)
        want = pack_conv_kernel(w)
        out = torch.full((want.size,), -1.0, device='cuda')
        _lib.check(lib.kfn_pack_conv_weights(dev(w).data_ptr(), k, k, ci, co, _lib.PACK_FORWARD, out.data_ptr(), stream()), 'pack')
        sync()
        assert np.array_equal(out.cpu().numpy().reshape(want.shape), want)


@pytest.mark.parametrize('case', [(3, 64, 64, 1, 24, 40), (3, 256, 128, 1, 15, 20), (3, 64, 256, 2, 16, 24), (3, 256, 512, 2, 30, 40),
                                  (1, 256, 128, 1, 15, 20), (1, 128, 4, 1, 15, 20)],
                         ids=['s1-64', 's1-256', 's2-64', 's2-256', '1x1-256', '1x1-prediction'])
def test_input_gradient_against_fp64(case):
    k, ci, co, s, H, Wd = case
    rng = np.random.default_rng(k * 1000 + ci + co + s)
    w = (rng.normal(size=(k, k, ci, co)) / np.sqrt(k * k * ci)).astype(np.float32)
    dz = rng.normal(size=(2, H // s, Wd // s, co)).astype(np.float32)
    got = run_input_grad(dz, w, s, (H, Wd))
    ref = R.conv_grad_input(dz, w, (H, Wd), s)
    # the accumulation runs over kh*kw*Cout: conv_tol's transposed form reads that from an HWIO kernel
    conv_tol.assert_close(got, ref, dz, w, 'direct', 'input gradient k%d %d->%d s%d' % (k, ci, co, s), transposed=True)


@pytest.mark.parametrize('stride', [1, 2])
def test_input_gradient_of_border_impulses_is_exact(stride):
    """One non-zero dZ entry at each border and corner: every input-gradient value is a single product 1 * w, so the result
    must EQUAL the fp64 one -- a shifted or dropped padding tap shows at once."""
    rng = np.random.default_rng(7)
    ci, co, H, Wd = 32, 16, 16, 24
    w = rng.normal(size=(3, 3, ci, co)).astype(np.float32)
    ho, wo = H // stride, Wd // stride
    spots = [(0, 0), (0, wo - 1), (ho - 1, 0), (ho - 1, wo - 1), (0, wo // 2), (ho - 1, wo // 2), (ho // 2, 0), (ho // 2, wo - 1)]
    dz = np.zeros((len(spots), ho, wo, co), np.float32)
    for i, (r, c) in enumerate(spots):
        dz[i, r, c, i % co] = 1.0
    got = run_input_grad(dz, w, stride, (H, Wd))
    ref = R.conv_grad_input(dz, w, (H, Wd), stride)
    assert np.array_equal(got.astype(np.float64), ref)
    assert np.count_nonzero(ref) > 0


# -- 3. loss ---------------------------------------------------------------------------------------------------------------
def run_loss(pred, labels, frames, M, clip, smooth_weight, ld_pred=4, ld_dpred=16):
    import torch
    lib = _lib.load()
    B, h, w, _ = pred.shape
    pb = np.full((B * h * w, ld_pred), 3.0, np.float32)
    pb[:, :4] = pred.reshape(-1, 4)
    d = _lib.CoordLossDesc(B=B, h=h, w=w, ld_pred=ld_pred, ld_dpred=ld_dpred, label_stride=labels.shape[1] // h,
                           img_stride=frames.shape[1] // h, has_transform=int(M is not None), has_loss_clip=int(clip is not None),
                           loss_clip=clip or 0.0, smooth_weight=smooth_weight, dist_threshold=0.05, min_uncertainty=1e-5)
    if M is not None:
        d.transform = (C.c_float * 12)(*[float(v) for v in np.asarray(M, np.float32)[:3].reshape(-1)])
    g = torch.full((B * h * w, ld_dpred), -5.0, device='cuda')
    st = torch.full((8,), -1.0, device='cuda')
    pd, ld, fd = dev(pb), dev(labels.astype(np.float32)), dev(frames)
    _lib.check(lib.kfn_coord_loss_grad(C.byref(d), pd.data_ptr(), ld.data_ptr(), fd.data_ptr(), g.data_ptr(), st.data_ptr(),
                                       stream()), 'kfn_coord_loss_grad')
    sync()
    gh = g.cpu().numpy()
    assert np.all(gh[:, 4:] == -5.0), 'the loss wrote outside its four gradient channels'
    return st.cpu().numpy(), gh[:, :4].reshape(B, h, w, 4)


def _loss_inputs(seed, B=2, h=8, w=12, full_res=False):
    rng = np.random.default_rng(seed)
    pred = rng.normal(size=(B, h, w, 4)).astype(np.float32)
    pred[..., 3] = rng.uniform(-2.0, 0.3, size=(B, h, w))
    s = 8 if full_res else 1
    labels = rng.normal(size=(B, h * s, w * s, 4)).astype(np.float32)
    labels[..., 3] = (rng.uniform(size=labels.shape[:3]) < 0.8)
    labels[0, 0, 0, 3] = 0.5
    frames = rng.integers(0, 256, size=(B, h * 8, w * 8, 3)).astype(np.uint8)
    frames[:, :, 40:] = frames[:, :, 40:41]            # a flat region: smoothness weights of 1 beside tiny ones
    M = np.eye(4, dtype=np.float32)
    M[:3, :3] += (0.1 * rng.normal(size=(3, 3))).astype(np.float32)
    M[:3, 3] = rng.normal(size=3)
    return pred, labels, frames, M


THR2 = float(np.float32(0.05 * 0.05))       # what the kernel subtracts: the reference's double product, rounded once to fp32
THR_MARGIN = 1e-6


def _assert_clear_of_the_threshold(pred, labels, M):
    """The condition on the inputs that lets the fp64 reference alone decide the accuracy count: no masked pixel whose squared
    distance lies within 1e-6 of the squared threshold (the fp32 d of the kernel is off by ~1e-9 there)."""
    B, h, w, _ = pred.shape
    lab = R.grid_labels(labels, (h, w)).astype(np.float64)
    gt = lab[..., :3]
    if M is not None:
        M64 = np.asarray(M, np.float64)
        gt = gt @ M64[:3, :3].T + M64[:3, 3]
    d = ((pred[..., :3].astype(np.float64) - gt) ** 2).sum(-1)
    assert not np.any((lab[..., 3] == 1.0) & (np.abs(d - THR2) < THR_MARGIN))
    return d


def _check_loss(pred, labels, frames, M, clip, sw, what):
    import torch
    st, g = run_loss(pred, labels, frames, M, clip, sw)
    B, h, w, _ = pred.shape
    p = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
    L, nll, sm, acc, valid = R.coord_loss(p, R.grid_labels(labels, (h, w)), frames[:, ::8, ::8].astype(np.float64), M, clip, sw)
    g64, = torch.autograd.grad(L, [p], allow_unused=True)
    g64 = np.zeros_like(pred, dtype=np.float64) if g64 is None else g64.numpy()
    want = [nll.item(), sm.item(), acc.item(), valid.item(), L.item()]
    for i, name in enumerate(('L_nll', 'L_smooth', 'accuracy', 'valid', 'L')):
        print('%s %s: device %.9g fp64 %.9g' % (what, name, st[i], want[i]))
        assert abs(st[i] - want[i]) <= 1e-5 * abs(want[i]), (what, name)
    scale = float(np.abs(g64).max())
    err = float(np.abs(g - g64).max())
    print('%s gradient: max err %.3g of max-abs %.3g' % (what, err, scale))
    assert err <= 1e-5 * scale, what
    return g64


def test_coord_loss_and_gradient_against_fp64_autograd():
    pred, labels, frames, M = _loss_inputs(1)
    _check_loss(pred, labels, frames, M, None, 50.0, 'masked')
    _check_loss(pred, labels, frames, None, None, 0.0, 'no transform, no smoothness')
    full = labels.copy()
    full[..., 3] = 1.0
    _check_loss(pred, full, frames, M, None, 50.0, 'without a mask')
    pred8, labels8, frames8, M8 = _loss_inputs(2, full_res=True)
    _check_loss(pred8, labels8, frames8, M8, None, 50.0, 'full-resolution labels')


def _vertical_weights(frames):
    """exp(-0.625 mean_c |img(r, c) - img(r + 1, c)|) on the frames' grid [B,h-1,w] (fp64); _horizontal_weights alike."""
    img = frames[:, ::8, ::8].astype(np.float64)
    return np.exp(-0.625 * np.abs(img[:, :-1] - img[:, 1:]).mean(-1))


def _horizontal_weights(frames):
    img = frames[:, ::8, ::8].astype(np.float64)
    return np.exp(-0.625 * np.abs(img[:, :, :-1] - img[:, :, 1:]).mean(-1))


def _flatten_upper_half(frames):
    """_loss_inputs' frames are flat along the rows only (columns 40..), so every VERTICAL edge weight is exp(-0.625 * ~85) = 0
    and the r + 1 / r - 1 reads of the kernel would go unchecked.  The upper half of each frame becomes flat down the columns:
    vertical weights 1 there, and 1 in both directions where the two flat regions meet.  Asserted: at least 10 % of the vertical
    and of the horizontal edges carry a weight above 0.1 (where the grid has such edges at all)."""
    H = frames.shape[1]
    frames[:, :(H + 1) // 2] = frames[:, :1]
    for wts in (_vertical_weights(frames), _horizontal_weights(frames)):
        assert wts.size == 0 or (wts > 0.1).mean() >= 0.1
    return frames


def _clip_inputs(seed, flat=False, **grid):
    """Inputs on both sides of loss_clip = -2 and of the 5 cm threshold; also returns the fp64 loss map l."""
    pred, labels, frames, M = _loss_inputs(seed, **grid)
    if flat:
        _flatten_upper_half(frames)
    rng = np.random.default_rng(seed + 1)
    pred[..., 3] = rng.uniform(-2.5, -0.5, size=pred.shape[:3])
    # labels a few centimetres from the prediction in the transformed frame: 3 log u in [-7.5, -1.5] decides the branch
    target = pred[..., :3].astype(np.float64) + 0.03 * rng.normal(size=pred.shape[:3] + (3,))
    M64 = M.astype(np.float64)
    labels[..., :3] = ((target - M64[:3, 3]) @ np.linalg.inv(M64[:3, :3]).T).astype(np.float32)
    gt = labels[..., :3].astype(np.float64) @ M64[:3, :3].T + M64[:3, 3]
    for _ in range(20):                                  # no pixel within 1e-3 of the clip, none within 1e-6 of (5 cm)^2
        sig = np.exp(pred[..., 3].astype(np.float64))
        d = ((pred[..., :3].astype(np.float64) - gt) ** 2).sum(-1)
        l = 3 * np.log(sig) + d / (2 * sig * sig)
        near = np.abs(l + 2.0) < 1e-3
        edge = np.abs(d - THR2) < THR_MARGIN
        if not near.any() and not edge.any():
            break
        pred[..., 3][near] += np.float32(0.05)
        pred[..., 0][edge] += np.float32(0.01)
    assert not near.any() and not edge.any()
    m = labels[..., 3] == 1.0
    assert (l[m] > -2.0).sum() > 10 and (l[m] < -2.0).sum() > 10
    assert (d[m] > THR2).sum() > 10 and (d[m] < THR2).sum() > 10
    return pred, labels, frames, M, l, m


def test_coord_loss_clip_with_both_branches():
    pred, labels, frames, M, l, m = _clip_inputs(3)
    g64 = _check_loss(pred, labels, frames, M, -2.0, 0.0, 'loss_clip -2')
    assert np.all(g64[(l > -2.0)] == 0.0) and np.any(g64[(l < -2.0) & m] != 0.0)
    _check_loss(pred, labels, frames, M, -2.0, 50.0, 'loss_clip -2 with smoothness')


def test_coord_loss_below_the_uncertainty_floor_and_with_an_empty_mask():
    pred, labels, frames, M = _loss_inputs(5)
    pred[0, 2:4, :, 3] = -13.0                             # sigma = 2.3e-6 < 1e-5: u is the floor, no gradient to channel 3
    g64 = _check_loss(pred, labels, frames, M, None, 50.0, 'sigma below 1e-5')
    assert np.all(g64[0, 2:4, :, 3] == 0.0)
    st, g = run_loss(pred, labels, frames, M, None, 50.0)
    assert np.all(g[0, 2:4, :, 3] == 0.0)
    empty = labels.copy()
    empty[..., 3] = 0.0
    _check_loss(pred, empty, frames, M, None, 50.0, 'all-zero mask')
    st, g = run_loss(pred, empty, frames, M, None, 50.0)
    assert st[3] == 1.0 and st[0] == 0.0 and st[1] == 0.0 and st[2] == 1.0 and not g.any()


# the loss beyond one pass of its 1024-thread loop `for (i = t; i < P; i += 1024)`; the tests above stop at 192 pixels
LOSS_GRIDS = [(1, 1, 1024), (1, 1, 1025),      # one row: no vertical neighbours; the second pass holds one pixel
              (1, 1025, 1),                    # one column
              (3, 17, 23),                     # 1173 pixels, odd, frame boundaries inside a pass
              (4, 60, 80), (2, 68, 120)]       # the production batch (19 passes) and the second product grid


def _grid_inputs(grid, full_res=False):
    B, h, w = grid
    pred, labels, frames, M = _loss_inputs(100 + LOSS_GRIDS.index(grid) + 10 * int(full_res), B=B, h=h, w=w, full_res=full_res)
    _flatten_upper_half(frames)
    _assert_clear_of_the_threshold(pred, labels, M)
    _assert_clear_of_the_threshold(pred, labels, None)
    return pred, labels, frames, M


def _seam_inputs():
    """B = 3 frames of 17x23 = 391 pixels, so frame boundaries fall inside a pass of the 1024-thread loop.  The last row of
    frame b and the first row of frame b + 1 lie 100 apart in every coordinate, all seam pixels are masked in, and the image
    rows under grid rows 0, 1, h-2 and h-1 are one and the same row in every frame: the vertical edge weight is 1 between rows
    0-1 and (h-2)-(h-1) inside a frame, and would be 1 between row h-1 of frame b and row 0 of frame b + 1.
    Returns the inputs and `tol`, _check_loss's tolerance 1e-5 max|g64|.  Asserted here, on the host: the within-frame weights
    at the seam rows are 1, and the term a neighbour from across the seam would add to the gradient,
    smooth_weight (2/3) / valid * weight * |x(b, h-1) - x(b+1, 0)|, exceeds 100 tol at EVERY seam pixel and coordinate."""
    import torch
    pred, labels, frames, M = _loss_inputs(200, B=3, h=17, w=23)
    B, h, w, _ = pred.shape
    pred[:, -1, :, :3] += 50.0
    pred[:, 0, :, :3] -= 50.0
    labels[:, (0, 1, -2, -1), :, 3] = 1.0
    for r in (0, 1, h - 2, h - 1):
        frames[:, 8 * r] = frames[0, 0]
    _assert_clear_of_the_threshold(pred, labels, M)
    wv = _vertical_weights(frames)
    assert np.all(wv[:, 0] == 1.0) and np.all(wv[:, -1] == 1.0)
    img = frames[:, ::8, ::8].astype(np.float64)
    w_cross = np.exp(-0.625 * np.abs(img[:-1, -1] - img[1:, 0]).mean(-1))                   # [B-1,w]
    assert np.all(w_cross == 1.0)
    p = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
    L, _, _, _, valid = R.coord_loss(p, labels, img, M, None, 50.0)
    g64, = torch.autograd.grad(L, [p])
    tol = 1e-5 * float(g64.abs().max())
    cross = 50.0 * (2.0 / 3.0) / valid.item() * w_cross[..., None] * np.abs(pred[:-1, -1, :, :3].astype(np.float64) - pred[1:, 0, :, :3])
    assert cross.min() > 100.0 * tol, (cross.min(), tol)
    return pred, labels, frames, M, tol


@pytest.mark.parametrize('grid', LOSS_GRIDS, ids=['%dx%dx%d' % g for g in LOSS_GRIDS])
def test_coord_loss_beyond_one_pass_against_fp64_autograd(grid):
    pred, labels, frames, M = _grid_inputs(grid)
    for m in (M, None):
        for sw in (50.0, 0.0):
            _check_loss(pred, labels, frames, m, None, sw, '%dx%dx%d%s, smooth_weight %g' % (grid + (' transform' if m is not None else '', sw)))


def test_coord_loss_on_the_production_batch_with_full_resolution_labels_and_with_the_clip():
    grid = (4, 60, 80)
    pred, labels, frames, M = _grid_inputs(grid, full_res=True)
    assert labels.shape == (4, 480, 640, 4)
    _check_loss(pred, labels, frames, M, None, 50.0, '4x60x80, labels at stride 8')
    pred, labels, frames, M, l, m = _clip_inputs(7, flat=True, B=4, h=60, w=80)
    g64 = _check_loss(pred, labels, frames, M, -2.0, 50.0, '4x60x80, loss_clip -2 with smoothness')
    g64 = _check_loss(pred, labels, frames, M, -2.0, 0.0, '4x60x80, loss_clip -2')
    assert np.all(g64[(l > -2.0)] == 0.0) and np.any(g64[(l < -2.0) & m] != 0.0)


def test_coord_loss_smoothness_does_not_reach_across_a_frame_seam():
    """_seam_inputs: edge weights of 1 on both sides of every frame seam and across it, the rows there 100 apart.  A vertical
    neighbour taken from the next (or previous) frame would move the gradient of those rows by more than 100 times the tolerance
    of _check_loss (asserted on the host by _seam_inputs); the legitimate neighbours, 50 away with weight 1, are checked by
    the same comparison."""
    pred, labels, frames, M, tol = _seam_inputs()
    g64 = _check_loss(pred, labels, frames, M, None, 50.0, 'frame seam')
    assert 1e-5 * float(np.abs(g64).max()) == pytest.approx(tol, rel=1e-9)


def test_coord_loss_counts_a_pixel_exactly_five_centimetres_off_as_inaccurate():
    """No transform, labels at the origin with mask 1, predictions (0.05f, 0, 0) on k pixels and the float below 0.05f on the
    others, 1173 pixels (the k pixels lie in both passes).  d = 0.05f^2 = 0x3B23D70B exceeds the reference's float32(0.05 * 0.05) =
    0x3B23D70A: accuracy = (valid - k) / valid.  With the threshold squared in fp32 it was 1."""
    B, h, w = 3, 17, 23
    P = B * h * w
    rng = np.random.default_rng(12)
    at = rng.permutation(P)[:P // 3]
    assert (at < 1024).any() and (at >= 1024).any()
    pred = np.zeros((P, 4), np.float32)
    pred[:, 0] = np.nextafter(np.float32(0.05), np.float32(0))
    pred[at, 0] = np.float32(0.05)
    pred[:, 3] = -1.0
    labels = np.zeros((B, h, w, 4), np.float32)
    labels[..., 3] = 1.0
    frames = np.zeros((B, h * 8, w * 8, 3), np.uint8)
    st, _ = run_loss(pred.reshape(B, h, w, 4), labels, frames, None, None, 0.0)
    valid = P + 1.0
    assert st[3] == valid
    assert st[2] == np.float32((valid - at.size) / valid), (st[2], at.size)


# -- 4. Adam ---------------------------------------------------------------------------------------------------------------
def test_adam_step_against_the_numpy_formula_over_three_steps():
    lib = _lib.load()
    rng = np.random.default_rng(9)
    n = 5003
    w = rng.normal(size=n).astype(np.float32) * np.float32(0.1)
    w[:500] = 0.0                                                   # biases start at zero
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    wd_, md, vd = dev(w), dev(m), dev(v)
    worst = 0.0
    for t in (1, 2, 3):
        g = (rng.normal(size=n) * 10.0 ** rng.uniform(-4, 0, size=n)).astype(np.float32)
        lr = 1e-4 * 0.5 ** (t / 7.0)
        gd = dev(g)
        _lib.check(lib.kfn_adam_step(wd_.data_ptr(), md.data_ptr(), vd.data_ptr(), gd.data_ptr(), n, R.adam_lr_t(lr, t), R.BETA1,
                                     R.BETA2, R.EPSILON, 1e-4, stream()), 'kfn_adam_step')
        sync()
        w, m, v = R.adam_step(w, m, v, g, lr, t, 1e-4)
        for name, got, want in (('w', wd_, w), ('m', md, m), ('v', vd, v)):
            u = float(R.ulp_distance(got.cpu().numpy(), want).max())
            print('adam step %d %s: %.2f ulp' % (t, name, u))
            worst = max(worst, u)
    assert worst <= 2.0


# -- 5. - 7. the whole network -----------------------------------------------------------------------------------------------
def _batch(size, B=2, seed=1):
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    from kfnet_amd.train import synthetic_labels
    frames = synthetic_sequence(B, size[0], size[1], seed=seed)
    labels = synthetic_labels(B, (size[0] // 8, size[1] // 8))
    return frames, labels, synthetic_transform().astype(np.float32)


def _weights(kind, seed=2):
    from kfnet_amd.weights import initial_weights, synthetic_weights
    if kind == 'initial':
        return initial_weights(seed)
    return {k: v for k, v in synthetic_weights(seed, init='he').items() if k.startswith('ScoreNet/')}


@pytest.mark.parametrize('kind', ['initial', 'he'])
@pytest.mark.parametrize('size', [(64, 96), (72, 104)], ids=['64x96', '72x104'])
def test_one_step_gradients_and_update_against_fp64(size, kind):
    import torch
    from kfnet_amd.train import SCoordNetTrainer
    frames, labels, M = _batch(size)
    W = _weights(kind)
    tr = SCoordNetTrainer(W, image_size=size, batch=2, transform=M, base_lr=1e-4, weight_decay=1e-4)
    stats = dict(tr.step(frames, labels))
    g = tr.gradients()
    s64, g64 = R.loss_and_grads(frames, labels, W, M)
    s32, g32 = R.loss_and_grads(frames, labels, W, M, dtype=torch.float32)
    print('loss: device %.7g torch-fp32 %.7g fp64 %.7g' % (stats['loss'], s32['loss'], s64['loss']))
    e_dev, e_32 = {}, {}
    for name in sorted(g64):
        scale = np.abs(g64[name]).max()
        e_dev[name] = float(np.abs(g[name] - g64[name]).max() / scale)
        e_32[name] = float(np.abs(g32[name] - g64[name]).max() / scale)
        print('%-28s e device %.3e  e torch-fp32 %.3e' % (name, e_dev[name], e_32[name]))
    worst_dev, worst_32 = max(e_dev.values()), max(e_32.values())
    print('worst e: device %.3e, torch-CPU fp32 %.3e, bound %.3e' % (worst_dev, worst_32, 4 * worst_32))
    assert worst_dev <= 4.0 * worst_32
    assert stats['pixels'] == float((labels[..., 3] == 1.0).sum()) and stats['lr'] == 1e-4
    # the update: numpy Adam on the device's own gradients
    after = tr.weights()
    st = tr.state()
    assert int(st['global_step']) == 1 and int(st['adam_t']) == 1
    worst = 0.0
    for name in sorted(W):
        z = np.zeros_like(W[name])
        w1, m1, v1 = R.adam_step(W[name], z, z, g[name], 1e-4, 1, 1e-4)
        worst = max(worst, float(R.ulp_distance(after[name], w1).max()), float(R.ulp_distance(st['adam_m/' + name], m1).max()),
                    float(R.ulp_distance(st['adam_v/' + name], v1).max()))
    print('weights after the step against numpy Adam: %.2f ulp' % worst)
    assert worst <= 2.0


def test_twenty_steps_on_one_batch_lower_the_loss_like_the_fp64_run():
    from kfnet_amd.train import SCoordNetTrainer, learning_rate
    frames, labels, M = _batch(SIZE)
    W = _weights('initial')
    tr = SCoordNetTrainer(W, image_size=SIZE, batch=2, transform=M, base_lr=1e-4, weight_decay=1e-4)
    dev_losses = [tr.step(frames, labels) for _ in range(21)]          # queued; entry i = the loss after i updates
    dev_losses = [s['loss'] for s in dev_losses]
    ref = {k: v.copy() for k, v in W.items()}
    m = {k: np.zeros_like(v) for k, v in W.items()}
    v_ = {k: np.zeros_like(v) for k, v in W.items()}
    ref_losses = []
    for t in range(1, 22):
        s, g = R.loss_and_grads(frames, labels, ref, M)
        ref_losses.append(s['loss'])
        lr = learning_rate(1e-4, 0.5, 80000, t - 1)
        for k in ref:
            ref[k], m[k], v_[k] = R.adam_step(ref[k], m[k], v_[k], g[k].astype(np.float32), lr, t, 1e-4)
    for i in (0, 1, 5, 10, 20):
        print('after %2d updates: device loss %.6f, fp64 run %.6f' % (i, dev_losses[i], ref_losses[i]))
    assert ref_losses[20] < ref_losses[0]
    assert abs(dev_losses[0] - ref_losses[0]) <= 1e-4 * abs(ref_losses[0])
    assert dev_losses[20] < 0.5 * (dev_losses[0] + ref_losses[20])


def _run_steps(tr, frames, labels, first, count):
    from kfnet_amd.train import batch_indices
    for s in range(first, first + count):
        idx = batch_indices(s, 2, frames.shape[0])
        tr.step(frames[idx], labels[idx])


def test_runs_are_bit_identical_and_resume_from_snapshot_files(tmp_path):
    from kfnet_amd.train import SCoordNetTrainer, restore
    frames, labels, M = _batch(SIZE, B=4)
    W = _weights('initial')
    kw = dict(image_size=SIZE, batch=2, transform=M, base_lr=1e-3, stepvalue=3)
    runs = []
    for _ in range(2):
        tr = SCoordNetTrainer(W, **kw)
        _run_steps(tr, frames, labels, 0, 4)
        runs.append(tr.weights())
    for k in W:
        assert np.array_equal(runs[0][k].view(np.uint32), runs[1][k].view(np.uint32)), k
        assert not np.array_equal(runs[0][k], W[k]), k
    tr = SCoordNetTrainer(W, **kw)
    _run_steps(tr, frames, labels, 0, 2)
    wp, sp = tr.save(str(tmp_path))
    assert os.path.basename(wp) == 'kfnet_weights-2.npz' and os.path.basename(sp) == 'kfnet_train_state-2.npz'
    del tr
    W2, state, step = restore(str(tmp_path), verbose=False)
    assert step == 2 and state is not None and sorted(W2) == sorted(W)
    tr = SCoordNetTrainer(W2, **kw)
    tr.load_state(state)
    assert tr.global_step == 2 and tr.adam_t == 2
    _run_steps(tr, frames, labels, 2, 2)
    resumed = tr.weights()
    for k in W:
        assert np.array_equal(resumed[k].view(np.uint32), runs[0][k].view(np.uint32)), k


# -- 8. the command line -------------------------------------------------------------------------------------------------------
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
    from kfnet_amd.engine import SCoordNetEngine
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    from kfnet_amd.train import SCoordNetTrainer, batch_indices, synthetic_labels
    from kfnet_amd.weights import initial_weights, load_npz
    model, out = tmp_path / 'm', tmp_path / 'o'
    out.mkdir()
    small = ['--height', '64', '--width', '96', '--batch', '2', '--scene', 'fire']
    log = _cli('kfnet_amd.SCoordNet.train', ['--model_folder', str(model), '--synthetic', '8', '--max_steps', '3', '--snapshot', '3',
                                             '--display', '1'] + small)
    assert sorted(os.listdir(str(model))) == ['kfnet_train_state-3.npz', 'kfnet_weights-3.npz']
    assert 'step 3/3' in log and 'starting from untrained weights' in log and 'l_measure=' in log
    # the same three steps in this process
    frames, labels = synthetic_sequence(8, 64, 96), synthetic_labels(8, (8, 12))
    tr = SCoordNetTrainer(initial_weights(0), image_size=SIZE, batch=2, transform=synthetic_transform(), stepvalue=30000)
    for s in range(3):
        idx = batch_indices(s, 2, 8)
        tr.step(frames[idx], labels[idx])
    W = tr.weights()
    saved = load_npz(str(model / 'kfnet_weights-3.npz'))
    assert sorted(saved) == sorted(W)
    for k in W:
        assert np.array_equal(saved[k].view(np.uint32), W[k].view(np.uint32)), k
    _cli('kfnet_amd.SCoordNet.eval', ['--model_folder', str(model), '--synthetic', '4', '--output_folder', str(out)] + small)
    eng = SCoordNetEngine(W, image_size=SIZE, batch=2, transform=np.linalg.inv(synthetic_transform()), max_chunk=4)
    want = eng.process(eng.upload_frames(synthetic_sequence(4, 64, 96))).cpu().numpy()
    got = np.stack([np.load(str(out / ('coord_%d.npy' % i))) for i in range(4)])
    assert np.array_equal(got, want)
    # a second run resumes at step 3 and has nothing left to do
    log = _cli('kfnet_amd.SCoordNet.train', ['--model_folder', str(model), '--synthetic', '8', '--max_steps', '3'] + small)
    assert 'current step:  3' in log and 'Adam slots restored' in log
