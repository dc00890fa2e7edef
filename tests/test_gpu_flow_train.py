"""Training OFlowNet on the device (stage 2): the four launches of kfn_train_flow.hip, the convolution launches
of stage 1 in the roles the Temporal scope gives them (weight gradients over windows of 8x8 .. 1x1 pixels, the transposed
layers as the input gradient of a stride-2 convolution), the whole step of kfnet_amd.train_flow.OFlowNetTrainer (forward,
gradients, Adam, reproducibility, resuming, learning) and the command line, against tests/flow_train_ref.py.

The rule of every comparison with fp64 autograd: e = max|g - g64| / max|g64| passes at e <= max(8 e_fp32, 1e-6),
e_fp32 being torch-CPU fp32 autograd of the same restatement on the same inputs; the seeds are those for which e_fp32 <= 1e-3,
so that no ReLU or floor kink decides a case."""
import ctypes as C

import numpy as np
import pytest
import torch

import flow_train_ref as FR
from gpu_util import dev, stream, sync
from kfnet_amd import _lib
from oracle.kfnet_oracle_torch import conv_same, deconv_same

pytestmark = pytest.mark.gpu

GRIDS = [(2, 3), (5, 7), (9, 13)]        # the window mostly outside; in between; the smallest with whole windows inside
GUARD = 64


def passes(what, got, g64, g32):
    e, e32 = FR.rel_err(got, g64), FR.rel_err(g32, g64)
    print('%-46s e = %.3e   e_fp32 = %.3e' % (what, e, e32))
    assert e32 <= 1e-3, (what, 'a kink decides this case: choose another seed', e32)
    assert e <= max(8.0 * e32, 1e-6), (what, e, e32)


def guarded(n, fill=-5.0):
    return torch.full((n + GUARD,), fill, device='cuda')


def taken(buf, n, fill=-5.0):
    h = buf.cpu().numpy()
    assert np.all(h[n:] == fill), 'wrote past the end of a buffer'
    return h[:n]


# -- 1. the cost volume's transpose ----------------------------------------------------------------------------------------------
def run_cvb(d_vol, grid, Cc):
    lib = _lib.load()
    P, h, w = grid
    n = P * h * w * Cc
    d2, d1 = guarded(n), guarded(n)
    vd = dev(d_vol.astype(np.float32))
    _lib.check(lib.kfn_cost_volume_backward(vd.data_ptr(), d2.data_ptr(), d1.data_ptr(), P, h, w, Cc, stream()),
               'kfn_cost_volume_backward')
    sync()
    return taken(d2, n).reshape(P, h, w, Cc), taken(d1, n).reshape(P, h, w, Cc)


@pytest.mark.parametrize('Cc', [32, 16])
@pytest.mark.parametrize('P', [1, 2])
@pytest.mark.parametrize('grid', GRIDS, ids=['%dx%d' % g for g in GRIDS])
def test_cost_volume_backward_equals_the_sequential_float32_sums_bit_for_bit(grid, P, Cc):
    rng = np.random.default_rng([grid[0], P, Cc])
    g = (P,) + grid
    d_vol = rng.normal(size=(P * grid[0] * grid[1], 8, 8, Cc)).astype(np.float32)
    got2, got1 = run_cvb(d_vol, g, Cc)
    want2, want1 = FR.cost_volume_backward(d_vol, g, np.float32)
    assert np.array_equal(got2, want2) and np.array_equal(got1, want1)
    again2, again1 = run_cvb(d_vol, g, Cc)
    assert np.array_equal(again2.view(np.uint32), got2.view(np.uint32)) and np.array_equal(again1.view(np.uint32), got1.view(np.uint32))
    # on integers every sum is exact: the gathers read the cells the fp64 transpose reads, across the frame seam none
    ints = rng.integers(-8, 9, size=d_vol.shape).astype(np.float32)
    got2, got1 = run_cvb(ints, g, Cc)
    want2, want1 = FR.cost_volume_backward(ints, g, np.float64)
    assert np.array_equal(got2, want2) and np.array_equal(got1, want1)


# -- 2. the flow head --------------------------------------------------------------------------------------------------------------
def head_ref(logits, pre, g_flow, g_sigma, dtype):
    lg = torch.from_numpy(logits.astype(np.float64)).to(dtype).requires_grad_(True)
    pr = torch.from_numpy(pre.astype(np.float64)).to(dtype).requires_grad_(True)
    _, flow, st = FR.flow_head(lg, pr)
    s = (flow * torch.from_numpy(g_flow.astype(np.float64)).to(dtype)).sum() + (st * torch.from_numpy(g_sigma.astype(np.float64)).to(dtype)).sum()
    a, b = torch.autograd.grad(s, [lg, pr])
    return a.to(torch.float64).numpy(), b.to(torch.float64).numpy()


@pytest.mark.parametrize('N', [6, 70, 234], ids=['1x2x3', '2x5x7', '2x9x13'])
def test_flow_head_backward_against_fp64_autograd(N):
    lib = _lib.load()
    rng = np.random.default_rng(N)
    logits = (3.0 * rng.normal(size=(N, 64))).astype(np.float32)
    pre = rng.normal(size=(N,)).astype(np.float32)
    g_flow = rng.normal(size=(N, 2)).astype(np.float32)
    g_sigma = rng.normal(size=(N,)).astype(np.float32)
    with torch.no_grad():                                   # the forward's fp32 outputs are what the launch reads
        prob, _, st = FR.flow_head(torch.from_numpy(logits), torch.from_numpy(pre))
    LD = 16
    dl, dp = guarded(N * 64 * LD), guarded(N * LD)
    bufs = [dev(a) for a in (g_flow, prob.numpy(), g_sigma, st.numpy())]
    _lib.check(lib.kfn_flow_head_backward(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(),
                                          dl.data_ptr(), LD, dp.data_ptr(), LD, N, stream()), 'kfn_flow_head_backward')
    sync()
    dlh, dph = taken(dl, N * 64 * LD).reshape(N, 64, LD), taken(dp, N * LD).reshape(N, LD)
    assert not dlh[..., 1:].any() and not dph[:, 1:].any()          # the padding channels are zeroed
    a64, b64 = head_ref(logits, pre, g_flow, g_sigma, torch.float64)
    a32, b32 = head_ref(logits, pre, g_flow, g_sigma, torch.float32)
    passes('flow head N=%d d_logits' % N, dlh[..., 0], a64, a32)
    passes('flow head N=%d d_pre' % N, dph[:, 0], b64, b32)


# -- 3. the L2 normalisation -----------------------------------------------------------------------------------------------------
def l2_ref(x, g, dtype):
    xt = torch.from_numpy(x.astype(np.float64)).to(dtype).requires_grad_(True)
    gx, = torch.autograd.grad((FR.l2_normalize(xt) * torch.from_numpy(g.astype(np.float64)).to(dtype)).sum(), [xt])
    return gx.to(torch.float64).numpy()


@pytest.mark.parametrize('pixels', [12, 70, 1001])
def test_l2norm_backward_against_fp64_autograd_with_an_all_zero_pixel(pixels):
    lib = _lib.load()
    rng = np.random.default_rng(pixels)
    x = rng.normal(size=(pixels, 32)).astype(np.float32)
    x[3] = 0.0                                              # under the floor: dx = 1e6 g
    x[5] *= np.float32(1e-8)                                # under it too, with a direction
    g = rng.normal(size=(pixels, 32)).astype(np.float32)
    xb = np.full((pixels, 40), 7.0, np.float32); xb[:, :32] = x
    gb = np.full((pixels, 36), 7.0, np.float32); gb[:, :32] = g
    out = guarded(pixels * 48)
    xd, gd = dev(xb), dev(gb)
    _lib.check(lib.kfn_l2norm_backward(xd.data_ptr(), 40, gd.data_ptr(), 36, out.data_ptr(), 48, pixels, 32, stream()),
               'kfn_l2norm_backward')
    sync()
    oh = taken(out, pixels * 48).reshape(pixels, 48)
    assert np.all(oh[:, 32:] == -5.0)
    got = oh[:, :32]
    r64, r32 = l2_ref(x, g, torch.float64), l2_ref(x, g, torch.float32)
    assert np.array_equal(got[3], np.float32(1e6) * g[3]) and np.array_equal(got[5], np.float32(1e6) * g[5])
    passes('l2norm %d pixels' % pixels, got, r64, r32)
    live = np.ones(pixels, bool); live[[3, 5]] = False      # the two floor pixels are 1e6 times the others: judge those alone too
    passes('l2norm %d pixels, above the floor' % pixels, got[live], r64[live], r32[live])


# -- 4. the loss -------------------------------------------------------------------------------------------------------------------
def loss_inputs(grid, P, seed, masked=False):
    h, w = grid
    rng = np.random.default_rng([seed, h, P])
    lab = rng.normal(size=(2 * P, h, w, 4)).astype(np.float32)
    lab[..., 0:3] *= np.float32(0.02)                      # a scene of centimetres: distances on both sides of the 5 cm threshold
    lab[..., 3] = (rng.uniform(size=(2 * P, h, w)) < 0.9).astype(np.float32)
    if h * w < 20:                                          # a 2x3 grid has two sets of corners: mask one cell of frame a, not a tenth
        lab[0::2, ..., 3] = 1.0
        lab[0::2, h - 1, 0, 3] = 0.0
    lab[1, 0, 0, 3] = 2.0                                   # only mask == 1 counts
    lab[1::2, ..., 0:3] = lab[0::2, ..., 0:3] + 0.03 * rng.normal(size=(P, h, w, 3)).astype(np.float32)   # some within 5 cm
    if masked:
        lab[1::2, ..., 3] = 0.0
    # every warped position at least 0.01 from an integer: no floor decides a corner
    # a step of -2 .. 1 cells; three cells in four are held to corners inside the grid, the fourth may leave it
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    cell = np.stack([xs, ys], -1)[None]
    step = cell + rng.integers(-2, 2, size=(P, h, w, 2))
    held = np.clip(step, 0, np.array([w - 2, h - 2]))
    free = (np.arange(P * h * w).reshape(P, h, w, 1) % 4) == 3
    step = np.where(free, step, held) - cell
    flow = (step + rng.uniform(0.01, 0.99, size=(P, h, w, 2))).astype(np.float32)
    st = (10.0 ** rng.uniform(-3, -1, size=(P, h, w))).astype(np.float32)
    st.reshape(-1)[::5] = np.float32(3e-6)                  # below the variance floor: no gradient
    return lab, flow, st


def run_loss(lab, flow, st, grid, P, stride, clip):
    lib = _lib.load()
    h, w = grid
    if stride > 1:                                          # full-resolution labels: cell (r, c) reads pixel (8 r, 8 c)
        full = np.full((2 * P, h * stride, w * stride, 4), np.nan, np.float32)
        full[:, ::stride, ::stride] = lab
        lab = full
    n = P * h * w
    gf, gs, stats = guarded(2 * n), guarded(n), guarded(16)
    d = _lib.FlowLossDesc(P=P, h=h, w=w, label_stride=stride, has_loss_clip=int(clip is not None),
                          loss_clip=0.0 if clip is None else clip, dist_threshold=0.05, min_uncertainty=1e-5)
    fd, sd, ld = dev(flow), dev(st), dev(lab)
    _lib.check(lib.kfn_flow_loss_grad(C.byref(d), fd.data_ptr(), sd.data_ptr(), ld.data_ptr(), gf.data_ptr(), gs.data_ptr(),
                                      stats.data_ptr(), stream()), 'kfn_flow_loss_grad')
    sync()
    return taken(stats, 16), taken(gf, 2 * n).reshape(P, h, w, 2), taken(gs, n).reshape(P, h, w)


def cell_terms(lab, flow, st):
    """(M, d, l) per cell in fp64, to keep the cases clear of the threshold and the clip."""
    xm, va, mb = FR.warp_labels(torch.from_numpy(flow.astype(np.float64)), lab)
    d = ((xm.numpy() - lab[1::2, ..., 0:3].astype(np.float64)) ** 2).sum(-1)
    s = st.astype(np.float64)
    u = np.sqrt(FR.EPS2 + np.maximum(s * s, FR.EPS2))
    return (va * mb).numpy(), d, 3 * np.log(u) + d / (2 * u * u)


@pytest.mark.parametrize('stride', [1, 8])
@pytest.mark.parametrize('clip', [False, True], ids=['noclip', 'clip'])
@pytest.mark.parametrize('P', [1, 2])
@pytest.mark.parametrize('grid', GRIDS, ids=['%dx%d' % g for g in GRIDS])
def test_flow_loss_and_gradients_against_fp64_autograd(grid, P, clip, stride):
    lab, flow, st = loss_inputs(grid, P, seed=8)       # a seed that leaves every grid four live cells or more
    M, d, l = cell_terms(lab, flow, st)
    thr2 = 0.05 * 0.05
    assert np.abs(d[M > 0] - thr2).min() > 1e-4 * thr2
    clip_at = None
    if clip:                                                # half of the live cells above the clip, none within 1e-3 of it
        ls = np.sort(l[M > 0])
        clip_at = float(np.float32(0.5 * (ls[len(ls) // 2 - 1] + ls[len(ls) // 2])))
        assert np.abs(l[M > 0] - clip_at).min() > 1e-3 * abs(clip_at) and ls[0] < clip_at < ls[-1]
    stats, gf, gs = run_loss(lab, flow, st, grid, P, stride, clip_at)
    s64, f64, g64 = FR.loss_grads(flow, st, lab, clip_at, torch.float64)
    s32, f32, g32 = FR.loss_grads(flow, st, lab, clip_at, torch.float32)
    what = 'loss %dx%dx%d%s stride %d' % ((P,) + grid + (' clip' if clip else '', stride))
    assert stats[2] == s64[2] == M.sum() + 1 and stats[3] == s64[3] and s64[3] > 0      # counts are exact
    assert stats[1] == np.float32(s64[1]) and 0 < s64[1] < 1
    assert not stats[4:].any()
    passes(what + ' L', stats[0], s64[0], s32[0])
    passes(what + ' d_flow', gf, f64, f32)
    passes(what + ' d_sigma', gs, g64, g32)
    assert not gf[M == 0].any() and not gs[M == 0].any() and not gs.reshape(-1)[::5].any()
    again = run_loss(lab, flow, st, grid, P, stride, clip_at)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(again, (stats, gf, gs)))


@pytest.mark.parametrize('grid', GRIDS, ids=['%dx%d' % g for g in GRIDS])
def test_flow_loss_of_an_all_masked_batch_is_zero_with_zero_gradients(grid):
    lab, flow, st = loss_inputs(grid, 2, seed=5, masked=True)
    stats, gf, gs = run_loss(lab, flow, st, grid, 2, 1, None)
    assert stats[0] == 0.0 and stats[1] == 1.0 and stats[2] == 1.0 and not gf.any() and not gs.any()


def test_flow_loss_beyond_one_pass_of_the_workgroup():
    """60x80 with two pairs: 9600 cells, more than nine passes of the 1024 threads."""
    grid, P = (60, 80), 2
    lab, flow, st = loss_inputs(grid, P, seed=6)
    stats, gf, gs = run_loss(lab, flow, st, grid, P, 1, None)
    s64, f64, g64 = FR.loss_grads(flow, st, lab, None, torch.float64)
    s32, f32, g32 = FR.loss_grads(flow, st, lab, None, torch.float32)
    assert stats[2] == s64[2] and stats[3] == s64[3]
    passes('loss 2x60x80 L', stats[0], s64[0], s32[0])
    passes('loss 2x60x80 d_flow', gf, f64, f32)
    passes('loss 2x60x80 d_sigma', gs, g64, g32)


# -- 5. stage 1's launches in the roles of the Temporal scope ------------------------------------------------------------------------
def conv_vjp(x, w, dz, stride, dtype):
    """(dW, db, dx) of conv_same(x, w) + b for x [N,H,W,ci], dz [N,Ho,Wo,co] by autograd in `dtype`."""
    xt = torch.from_numpy(x.astype(np.float64)).to(dtype).permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.from_numpy(w.astype(np.float64)).to(dtype).requires_grad_(True)
    b = torch.zeros(w.shape[3], dtype=dtype, requires_grad=True)
    y = conv_same(xt, wt, b, stride, False).permute(0, 2, 3, 1)
    gw, gb, gx = torch.autograd.grad((y * torch.from_numpy(dz.astype(np.float64)).to(dtype)).sum(), [wt, b, xt])
    return [t.to(torch.float64).numpy() for t in (gw, gb, gx.permute(0, 2, 3, 1))]


def deconv_vjp(x, w, dy, dtype):
    """(y, dW, dx) of deconv_same(x, w) for x [N,h,w,ci], w [k,k,co,ci], dy [N,2h,2w,co] by autograd in `dtype`."""
    xt = torch.from_numpy(x.astype(np.float64)).to(dtype).permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.from_numpy(w.astype(np.float64)).to(dtype).requires_grad_(True)
    y = deconv_same(xt, wt, None, 2, False).permute(0, 2, 3, 1)
    gw, gx = torch.autograd.grad((y * torch.from_numpy(dy.astype(np.float64)).to(dtype)).sum(), [wt, xt])
    return [t.detach().to(torch.float64).numpy() for t in (y, gw, gx.permute(0, 2, 3, 1))]


def run_wgrad(x, dz, k, stride):
    lib = _lib.load()
    n, h, w, ci = x.shape
    co = dz.shape[3]
    d = _lib.ConvDesc(N=n, H=h, W=w, Cin=ci, ldx=ci, Cout=co, cout_pad=-(-co // 32) * 32, ldy=co, kh=k, kw=k, stride=stride)
    nb = C.c_size_t()
    _lib.check(lib.kfn_conv2d_grad_weights_workspace_bytes(C.byref(d), C.byref(nb)), 'workspace bytes')
    ws = guarded(nb.value // 4, -9.0)
    dw, db = guarded(k * k * ci * co), guarded(co)
    xd, zd = dev(x), dev(dz)
    _lib.check(lib.kfn_conv2d_grad_weights(C.byref(d), xd.data_ptr(), zd.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                           stream()), 'kfn_conv2d_grad_weights')
    sync()
    taken(ws, nb.value // 4, -9.0)
    return taken(dw, k * k * ci * co).reshape(k, k, ci, co), taken(db, co)


def run_packed_conv(x, w_hwio, kind, stride, transposed, out_hw):
    """kfn_pack_conv_weights(kind) of the HWIO kernel + kfn_conv2d_nhwc on x [N,H,W,c] (c padded to 16): as kfnet_amd.train runs
    its input gradients (transposed = 1, KFN_PACK_INPUT_GRAD_S2) and its forward layers (KFN_PACK_FORWARD)."""
    lib = _lib.load()
    k, _, ci, co = w_hwio.shape
    n, h, w, cx = x.shape
    c_out = ci if transposed else co
    assert cx == (co if transposed else ci)
    c16 = -(-cx // 16) * 16
    nf = C.c_size_t()
    _lib.check(lib.kfn_pack_conv_weights_floats(k, k, ci, co, kind, C.byref(nf)), 'pack floats')
    pack = guarded(nf.value, -7.0)
    wd = dev(w_hwio)
    _lib.check(lib.kfn_pack_conv_weights(wd.data_ptr(), k, k, ci, co, kind, pack.data_ptr(), stream()), 'kfn_pack_conv_weights')
    xb = np.zeros((n * h * w, c16), np.float32)
    xb[:, :cx] = x.reshape(-1, cx)
    xd = dev(xb)
    H, Wd = out_hw
    out = guarded(n * H * Wd * c_out)
    d = _lib.ConvDesc(N=n, H=h, W=w, Cin=c16 if transposed else ci, ldx=c16, Cout=c_out, cout_pad=-(-c_out // 32) * 32, ldy=c_out,
                      kh=k, kw=k, stride=stride, transposed=int(transposed))
    _lib.check(lib.kfn_conv2d_nhwc(C.byref(d), xd.data_ptr(), pack.data_ptr(), None, out.data_ptr(), stream()), 'kfn_conv2d_nhwc')
    sync()
    taken(pack, nf.value, -7.0)
    return taken(out, n * H * Wd * c_out).reshape(n, H, Wd, c_out)


# (layer, kernel, Cin, Cout, stride, window): the U-Net's convolutions at every window size, and the dense head as 1x1
WINDOW_LAYERS = [('conv0', 3, 32, 32, 1, 8), ('conv1a', 3, 32, 32, 2, 8), ('conv6', 3, 48, 16, 1, 8), ('prediction', 3, 16, 1, 1, 8),
                 ('conv1b', 3, 32, 32, 1, 4), ('conv2a', 3, 32, 64, 2, 4), ('conv5', 3, 64, 32, 1, 4), ('conv2b', 3, 64, 64, 1, 2),
                 ('conv3a', 3, 64, 128, 2, 2), ('conv4', 3, 128, 64, 1, 2), ('conv3b', 3, 128, 128, 1, 1), ('fc1', 1, 128, 64, 1, 1),
                 ('uncertainty', 1, 32, 1, 1, 1)]


@pytest.mark.parametrize('N', [6, 70], ids=['1x2x3', '2x5x7'])
@pytest.mark.parametrize('layer', WINDOW_LAYERS, ids=['%s-%dx%d' % (l[0], l[5], l[5]) for l in WINDOW_LAYERS])
def test_weight_gradient_over_windows_against_fp64_autograd(layer, N):
    name, k, ci, co, s, win = layer
    rng = np.random.default_rng([WINDOW_LAYERS.index(layer), N])
    x = np.maximum(rng.normal(size=(N, win, win, ci)), 0).astype(np.float32)          # layer inputs are post-ReLU
    if name == 'conv0':
        x = rng.normal(size=x.shape).astype(np.float32)                              # the cost volume is signed
    wo = -(-win // s)
    dz = rng.normal(size=(N, wo, wo, co)).astype(np.float32)
    w0 = np.zeros((k, k, ci, co), np.float32)
    dw, db = run_wgrad(x, dz, k, s)
    w64, b64, _ = conv_vjp(x, w0, dz, s, torch.float64)
    w32, b32, _ = conv_vjp(x, w0, dz, s, torch.float32)
    passes('wgrad %s %dx%dx%d' % (name, N, win, win), dw, w64, w32)
    passes('wgrad %s %dx%dx%d bias' % (name, N, win, win), db, b64, b32)


# (layer, Cin, Cout, input window)
UPCONVS = [('upconv2', 128, 64, 1), ('upconv1', 64, 32, 2), ('upconv0', 32, 16, 4)]


@pytest.mark.parametrize('N', [6, 70], ids=['1x2x3', '2x5x7'])
@pytest.mark.parametrize('layer', UPCONVS, ids=[l[0] for l in UPCONVS])
def test_transposed_layer_as_the_input_gradient_of_a_stride_2_convolution(layer, N):
    """y = deconv(x, w[k,k,Cout,Cin]) is d/dX of conv_s2(X [2h,2w,Cout], w as HWIO) at dZ = x.  So the forward is the input-gradient
    launch (KFN_PACK_INPUT_GRAD_S2), the layer's input gradient a plain stride-2 convolution (KFN_PACK_FORWARD), and its weight
    gradient kfn_conv2d_grad_weights with the layer's output gradient as input and the layer's input as dZ -- in TF's layout."""
    name, ci, co, win = layer
    rng = np.random.default_rng([UPCONVS.index(layer), N, 1])
    x = np.maximum(rng.normal(size=(N, win, win, ci)), 0).astype(np.float32)
    w = (rng.normal(size=(3, 3, co, ci)) / np.sqrt(9 * ci)).astype(np.float32)
    dy = rng.normal(size=(N, 2 * win, 2 * win, co)).astype(np.float32)
    y64, w64, x64 = deconv_vjp(x, w, dy, torch.float64)
    y32, w32, x32 = deconv_vjp(x, w, dy, torch.float32)
    y = run_packed_conv(x, w, _lib.PACK_INPUT_GRAD_S2, 2, True, (2 * win, 2 * win))
    passes('%s N=%d forward' % (name, N), y, y64, y32)
    dx = run_packed_conv(dy, w, _lib.PACK_FORWARD, 2, False, (win, win))
    passes('%s N=%d input gradient' % (name, N), dx, x64, x32)
    dw, _ = run_wgrad(dy, x, 3, 2)
    assert dw.shape == w.shape
    passes('%s N=%d weight gradient' % (name, N), dw, w64, w32)


# -- 6. the whole step: kfnet_amd.train_flow.OFlowNetTrainer -----------------------------------------------------------------------
# synthetic_sequence(seed) with synthetic_weights(100 + seed).  A ReLU unit whose fp64 pre-activation lies within fp32 rounding of
# zero (one ulp of an O(1) activation is 1.2e-7) has its mask, and with it the gradient, decided by the last rounding of whoever
# computes it: of seeds 1..40 these are the ones whose smallest |pre-activation| over all units is largest (3.1e-7 and 1.9e-7;
# seed 1 has units at 1.4e-8 and 1.7e-8).  e_fp32 <= 3.6e-6 for every variable.
STEP_SEEDS = {(64, 96): 39, (72, 104): 7}
ZERO_BY_SYMMETRY = 'Temporal/prediction/bias'      # the softmax ignores a shift of all 64 logits: this gradient is 0


def _step_inputs(size, P=2):
    from kfnet_amd.synth import synthetic_sequence
    from kfnet_amd.train import synthetic_labels
    from kfnet_amd.weights import synthetic_weights
    seed = STEP_SEEDS[size]
    frames = synthetic_sequence(2 * P, size[0], size[1], seed=seed)
    labels = synthetic_labels(2 * P, (size[0] // 8, size[1] // 8))
    W = {k: v for k, v in synthetic_weights(seed=100 + seed).items() if k.startswith('Temporal/')}
    return frames, labels, W


def _trainer(W, size, P=2, **kw):
    from kfnet_amd.train_flow import OFlowNetTrainer
    return OFlowNetTrainer(W, image_size=size, pairs=P, **kw)


def _one_pass(tr, frames, labels):
    tr.stage(frames, labels)
    tr.forward()
    tr.loss()
    tr.backward()
    sync()
    return tr.stats.cpu().numpy().copy(), tr.gradients()


@pytest.mark.parametrize('size', [(64, 96), (72, 104)], ids=['64x96', '72x104'])
def test_one_step_forward_gradients_and_update_against_fp64(size):
    import train_ref as R
    from kfnet_amd.engine import OFlowNetEngine
    frames, labels, W = _step_inputs(size)
    tr = _trainer(W, size)
    stats, grads = _one_pass(tr, frames, labels)
    # forward: no further from the fp64 restatement than twice the eval engine is, on the same frames and weights
    with torch.no_grad():
        _, f64, s64 = FR.forward(frames, FR.tensors(W, torch.float64))
    f64, s64 = f64.numpy().reshape(-1, 2), s64.numpy().reshape(-1)
    eng = OFlowNetEngine(W, image_size=size, batch=2)
    rec = np.concatenate([eng.process(eng.upload_frames(frames[2 * p:2 * p + 2])).cpu().numpy()[1:2] for p in range(2)])
    e_flow, e_sig = np.abs(rec[..., 0:2].reshape(-1, 2) - f64).max(), np.abs(1.0 / rec[..., 2].reshape(-1) - s64).max()
    t_flow, t_sig = np.abs(tr.flow.cpu().numpy() - f64).max(), np.abs(tr.sigma.cpu().numpy().reshape(-1) - s64).max()
    print('forward %dx%d: flow trainer %.3e engine %.3e, sigma_trans trainer %.3e engine %.3e' % (size + (t_flow, e_flow, t_sig, e_sig)))
    assert t_flow <= max(2 * e_flow, 1e-6) and t_sig <= max(2 * e_sig, 1e-6)
    # gradients of every Temporal/* variable
    L64, g64 = FR.step_loss_and_grads(frames, labels, W)
    L32, g32 = FR.step_loss_and_grads(frames, labels, W, dtype=torch.float32)
    passes('step %dx%d L' % size, stats[0], L64, L32)
    assert sorted(grads) == sorted(g64) == sorted(W)
    for name in sorted(g64):
        if name == ZERO_BY_SYMMETRY:
            scale = np.abs(g64['Temporal/prediction/kernel']).max()
            print('%-46s |g| = %.3e beside %.3e' % (name, np.abs(grads[name]).max(), scale))
            assert np.abs(grads[name]).max() <= 1e-6 * scale and np.abs(g64[name]).max() <= 1e-12 * scale
            continue
        passes('step %dx%d %s' % (size + (name,)), grads[name], g64[name], g32[name])
    # Adam on the device's gradients equals the numpy formula bit for bit
    before = tr.weights()
    lr = tr.apply_gradients()
    sync()
    after, st = tr.weights(), tr.state()
    for name in sorted(W):
        w1, m1, v1 = R.adam_step(before[name], np.zeros_like(before[name]), np.zeros_like(before[name]), grads[name], lr, 1, 1e-4)
        assert np.array_equal(after[name], w1) and np.array_equal(st['adam_m/' + name], m1) and np.array_equal(st['adam_v/' + name], v1), name
    # a second trainer repeats the first bit for bit
    stats2, grads2 = _one_pass(_trainer(W, size), frames, labels)
    assert np.array_equal(stats2.view(np.uint32), stats.view(np.uint32))
    assert all(np.array_equal(grads2[n].view(np.uint32), grads[n].view(np.uint32)) for n in grads)


def test_a_run_interrupted_at_a_snapshot_resumes_to_the_same_arrays(tmp_path):
    from kfnet_amd.weights import load_npz
    size = (64, 96)
    frames, labels, W = _step_inputs(size)
    a = _trainer(W, size)
    for _ in range(4):
        a.step(frames, labels)
    b = _trainer(W, size)
    for _ in range(2):
        b.step(frames, labels)
    wp, sp = b.save(str(tmp_path))
    assert wp.endswith('kfnet_weights-2.npz') and sp.endswith('kfnet_train_state-2.npz')
    saved = load_npz(wp)
    assert sorted(saved) == sorted(W)
    c = _trainer(saved, size)
    with np.load(sp) as z:
        c.load_state({k: z[k] for k in z.files})
    for _ in range(2):
        c.step(frames, labels)
    sync()
    wa, wc, sa, sc = a.weights(), c.weights(), a.state(), c.state()
    assert c.global_step == a.global_step == 4
    assert all(np.array_equal(wa[n].view(np.uint32), wc[n].view(np.uint32)) for n in wa)
    assert all(np.array_equal(np.asarray(sa[n]), np.asarray(sc[n])) for n in sa)


def test_ten_steps_on_one_batch_follow_the_fp64_run():
    import train_ref as R
    from kfnet_amd.train import learning_rate
    size = (64, 96)
    frames, labels, W = _step_inputs(size)
    tr = _trainer(W, size, base_lr=1e-4)
    dev_losses = [tr.step(frames, labels)['loss'] for _ in range(10)]
    Wr = {k: v.copy() for k, v in W.items()}
    m = {k: np.zeros_like(v) for k, v in W.items()}
    v = {k: np.zeros_like(x) for k, x in W.items()}
    ref_losses = []
    for t in range(1, 11):
        L, g = FR.step_loss_and_grads(frames, labels, Wr)
        ref_losses.append(L)
        for k in Wr:
            Wr[k], m[k], v[k] = R.adam_step(Wr[k], m[k], v[k], g[k].astype(np.float32), learning_rate(1e-4, 0.5, 100000, t - 1), t, 1e-4)
    print('ten steps: device %s\n           fp64   %s' % (['%.4f' % x for x in dev_losses], ['%.4f' % x for x in ref_losses]))
    assert ref_losses[-1] < ref_losses[0] and dev_losses[-1] < dev_losses[0]
    for a, b in zip(dev_losses, ref_losses):
        assert abs(a - b) <= 0.05 * abs(b), (dev_losses, ref_losses)


# -- 7. the command line -----------------------------------------------------------------------------------------------------------
def _cli(module, args, timeout=600):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT'):
        env.pop(k, None)
    env['PYTHONPATH'] = root + os.pathsep + env.get('PYTHONPATH', '')
    r = subprocess.run([sys.executable, '-m', module] + args, cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_train_command_line_then_the_engine_and_stage_3_read_its_snapshot(tmp_path):
    import os
    from kfnet_amd.engine import OFlowNetEngine
    from kfnet_amd.synth import synthetic_sequence
    from kfnet_amd.weights import initial_weights, load_npz
    model, kf = tmp_path / 'm', tmp_path / 'kf'
    small = ['--height', '64', '--width', '96']
    log = _cli('kfnet_amd.OFlowNet.train', ['--model_folder', str(model), '--synthetic', '6', '--max_steps', '4', '--snapshot', '2',
                                            '--display', '2'] + small)
    assert sorted(os.listdir(str(model))) == ['kfnet_train_state-2.npz', 'kfnet_train_state-4.npz', 'kfnet_weights-2.npz',
                                              'kfnet_weights-4.npz']
    assert 'step 4/4' in log and 'current step:  0' in log and 'starting from untrained weights' in log
    saved, start = load_npz(str(model / 'kfnet_weights-4.npz')), initial_weights(0, scopes=('Temporal',))
    assert sorted(saved) == sorted(start) and all(k.startswith('Temporal/') for k in saved)
    assert all(not np.array_equal(saved[k], start[k]) for k in start if k.endswith('kernel') and k != ZERO_BY_SYMMETRY)
    eng = OFlowNetEngine(saved, image_size=(64, 96), batch=2)
    rec = eng.process(eng.upload_frames(synthetic_sequence(2, 64, 96))).cpu().numpy()
    assert rec.shape == (2, 8, 12, 3) and np.isfinite(rec[1]).all()
    # a second run resumes at step 4 with its Adam slots and has nothing left to do
    log = _cli('kfnet_amd.OFlowNet.train', ['--model_folder', str(model), '--synthetic', '6', '--max_steps', '4'] + small)
    assert 'current step:  4' in log and 'Adam slots restored' in log
    log = _cli('kfnet_amd.KFNet.train', ['--model_folder', str(kf), '--synthetic', '8', '--fix_flownet', '--oflownet', str(model),
                                         '--max_steps', '1', '--scene', 'fire'] + small)
    assert 'step 1/1' in log and 'Restore from scope Temporal' in log
