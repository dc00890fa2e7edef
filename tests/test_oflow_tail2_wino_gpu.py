"""-m gpu: kfn_oflow_tail2 with conv6 as Winograd F(2x2,3x3) (csrc/kfn_oflow_fused.hip, fp32).

Exact cases pin the zero border inside the tiles' 4x4 patches and the tile -> cell map of both transforms: on data that
both transforms carry exactly the logits equal the oracle's bit for bit.  Random cases bound the round-off by the error
model of tests/conv_tol.py.  The CPU restatement of the scheme is tests/test_oflow_tail2_wino_host.py."""
import numpy as np
import pytest

from oracle import kfnet_oracle as O
from tests.conv_tol import conv_err_bound, record

pytestmark = pytest.mark.gpu


def _launch(T, Gp, N, H, W, d5, du, dbu, d6, db6, dwp, dbp, with_logits=True):
    import torch
    from tests.gpu_util import stream, sync
    from kfnet_amd import _lib
    lib = _lib.load()
    P = N * H * W
    flow = torch.full((P * 2 + 8,), -7.0, device='cuda')
    logits = torch.full((P * 64 + 8,), -7.0, device='cuda') if with_logits else None
    _lib.check(lib.kfn_oflow_tail2(T.data_ptr(), Gp.data_ptr(), N, H, W, 1, d5.data_ptr(), du.data_ptr(), dbu.data_ptr(),
                                   d6.data_ptr(), db6.data_ptr(), dwp.data_ptr(), dbp.data_ptr(), flow.data_ptr(),
                                   logits.data_ptr() if with_logits else None, stream()), 'oflow_tail2')
    sync()
    return flow, logits


# ---- exact cases -----------------------------------------------------------------------------------------------------------------
# P = 1 (N = H = W = 1).  conv0 of window cell (ci, cj), channel k, from the factored maps (include/kfnet_hip.h,
# kfn_cost_volume_gather): relu(T[class(ci, cj)][k] - Gp[ci - 2, cj - 2][class][k]), the G term 0 outside the 5x5 extended map.
# upconv0's kernel gives input channel c the single tap c % 9 into output channel c % 16, so an impulse x5[i, j, c] lands in
# exactly one cell (2i + ky, 2j + kx): the four corners, one cell on each edge and one interior cell of the window.
IMPULSES = [  # (window cell, (i, j) of the 4x4 conv5 patch, tap (ky, kx))
    ((0, 0), (0, 0), (0, 0)), ((0, 7), (0, 3), (0, 1)), ((7, 0), (3, 0), (1, 0)), ((7, 7), (3, 3), (1, 1)),
    ((0, 3), (0, 1), (0, 1)), ((7, 4), (3, 1), (1, 2)), ((3, 0), (1, 0), (1, 0)), ((4, 7), (1, 3), (2, 1)),
    ((3, 4), (1, 2), (1, 0)),
]


def _exact_inputs():
    rng = np.random.default_rng(23)
    x5 = np.zeros((1, 4, 4, 32), np.float32)
    wu = np.zeros((3, 3, 16, 32), np.float32)                      # [kh,kw,Cout,Cin]
    for c in range(32):
        wu[(c % 9) // 3, (c % 9) % 3, c % 16, c] = 1
    for k, (cell, (i, j), (ky, kx)) in enumerate(IMPULSES):
        assert (2 * i + ky, 2 * j + kx) == cell
        for c in range(ky * 3 + kx, 32, 9):                        # every input channel that carries this tap
            x5[0, i, j, c] = 1 + (k + c) % 3
    bu = np.zeros(16, np.float32)
    T = rng.integers(-2, 3, size=(1, 1, 1, 288)).astype(np.float32)
    Gp = rng.integers(-2, 3, size=(1, 5, 5, 288)).astype(np.float32)
    conv0 = np.zeros((1, 8, 8, 32))
    for ci in range(8):
        for cj in range(8):
            cls = (0 if ci == 0 else 2 if ci == 7 else 1) * 3 + (0 if cj == 0 else 2 if cj == 7 else 1)
            g = Gp[0, ci - 2, cj - 2, cls * 32:cls * 32 + 32] if 2 <= ci < 7 and 2 <= cj < 7 else 0.0
            conv0[0, ci, cj] = np.maximum(T[0, 0, 0, cls * 32:cls * 32 + 32] - g, 0)
    # conv6: one tap per (input channel, output channel) -> U holds 0, +-1/4, +-1/2 and 1
    w6 = np.zeros((3, 3, 48, 16), np.float32)
    ci_, co_ = np.meshgrid(np.arange(48), np.arange(16), indexing='ij')
    tap = (5 * ci_ + 3 * co_) % 9
    w6[tap // 3, tap % 3, ci_, co_] = 1
    b6 = (np.arange(16) % 5 - 2).astype(np.float32)
    up = O.conv2d_transpose_same(x5.astype(np.float64), wu, bu, 2, True)
    for cell, _, _ in IMPULSES:
        assert up[0, cell[0], cell[1]].max() >= 1
    assert np.count_nonzero(up.max(-1)) == len(IMPULSES)            # impulses, and nothing else
    mid = O.conv2d_same(np.concatenate([up, conv0], -1), w6, b6, 1, True)      # [1,8,8,16], small integers
    return x5, wu, bu, T, Gp, w6, b6, mid


def test_oflow_tail2_wino_exact_borders():
    """Small integers through B^T d B, quarters through G w G^T, a one-hot centre tap as 'prediction': every product and sum
    is exact in fp32, so the logits equal the oracle's bit for bit, for each of conv6's 16 output channels."""
    from tests.gpu_util import dev
    from kfnet_amd.graph import pack_oflow_tail_kernel, pack_oflow_upconv_kernel
    x5, wu, bu, T, Gp, w6, b6, mid = _exact_inputs()
    assert np.abs(mid).max() < 2 ** 20 and mid.max() > 8
    d5, du, dbu, d6, db6 = dev(x5), dev(pack_oflow_upconv_kernel(wu)), dev(bu), dev(pack_oflow_tail_kernel(w6)), dev(b6)
    dT, dG = dev(T), dev(Gp)
    for n in range(16):
        wp = np.zeros((3, 3, 16), np.float32)
        wp[1, 1, n] = 1
        bp = np.array([n - 3.0], np.float32)
        flow, logits = _launch(dT, dG, 1, 1, 1, d5, du, dbu, d6, db6, dev(wp), dev(bp))
        got = logits.cpu().numpy()
        assert np.all(got[64:] == -7.0)
        ref = (mid[0, :, :, n] + bp[0]).reshape(64).astype(np.float32)
        assert np.array_equal(got[:64], ref), (n, np.argwhere(got[:64] != ref).ravel())
        assert np.all(np.isfinite(flow.cpu().numpy()[:2]))


# ---- random cases ----------------------------------------------------------------------------------------------------------------
def _random_case(shape):
    from tests.test_gpu_ops import _factored_maps, _oracle_conv0
    N, H, W = shape
    P = N * H * W
    rng = np.random.default_rng(57)                                  # drawn as in test_gpu_ops.py::test_oflow_tail2_vs_oracle
    f = rng.normal(size=(N + 1, H, W, 32)).astype(np.float32)
    w0 = (rng.normal(size=(3, 3, 32, 32)) / np.sqrt(9 * 32)).astype(np.float32)
    b0 = rng.normal(size=32).astype(np.float32)
    x5 = np.maximum(rng.normal(size=(P, 4, 4, 32)), 0).astype(np.float32)
    wu = (rng.normal(size=(3, 3, 16, 32)) * np.sqrt(2.0 / (4 * 32))).astype(np.float32)
    bu = (rng.normal(size=16) * 0.1).astype(np.float32)
    w6 = (rng.normal(size=(3, 3, 48, 16)) * np.sqrt(2.0 / (9 * 48))).astype(np.float32)
    b6 = (rng.normal(size=16) * 0.1).astype(np.float32)
    wp = (rng.normal(size=(3, 3, 16, 1)) * 0.5).astype(np.float32)
    bp = np.array([0.3], np.float32)
    T, Gp, keep = _factored_maps(f, w0, b0, N, H, W)
    up = O.conv2d_transpose_same(x5.astype(np.float64), wu, bu, 2, True)
    cat = np.concatenate([up, _oracle_conv0(f, w0, b0, N, H, W)], -1)
    mid = O.conv2d_same(cat, w6, b6, 1, True)
    ref_logits = O.conv2d_same(mid, wp, bp, 1, False)[..., 0].reshape(P, 64)
    # tolerance on the logits: conv6's error (K = 432, class F(2x2,3x3)) reaches a logit through the 144 taps of 'prediction',
    # at most scaled by their L1 norm; the prediction conv adds its own direct-class error (K = 144)
    tol = conv_err_bound(cat, w6, 'f23') * float(np.abs(wp).sum()) + conv_err_bound(mid, wp, 'direct')
    return dict(P=P, T=T, Gp=Gp, keep=keep, host=(x5, wu, bu, w6, b6, wp, bp), ref_logits=ref_logits, tol=tol)


@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 3, 5), (2, 7, 9)])
def test_oflow_tail2_wino_random(shape):
    """(1,1,1): fewer windows than waves; (1,3,5): a window count that is no multiple of 4; (2,7,9): two images."""
    import torch
    from tests.gpu_util import dev
    from kfnet_amd.graph import pack_oflow_tail_kernel, pack_oflow_upconv_kernel
    N, H, W = shape
    c = _random_case(shape)
    P, tol, ref_logits = c['P'], c['tol'], c['ref_logits']
    x5, wu, bu, w6, b6, wp, bp = c['host']
    args = (c['T'], c['Gp'], N, H, W, dev(x5), dev(pack_oflow_upconv_kernel(wu)), dev(bu), dev(pack_oflow_tail_kernel(w6)),
            dev(b6), dev(wp[..., 0]), dev(bp))
    flow, logits = _launch(*args)
    got_l, got_f = logits.cpu().numpy(), flow.cpu().numpy()
    assert np.all(got_l[P * 64:] == -7.0) and np.all(got_f[P * 2:] == -7.0)
    pr = O.softmax(ref_logits)
    offs = O.coord_volume(np.zeros((1, 2, 2, 1)), np.zeros((1, 2, 2, 1)), 8)[1]
    e_l = float(np.abs(got_l[:P * 64].reshape(P, 64) - ref_logits).max())
    e_f = float(np.abs(got_f[:P * 2].reshape(P, 2) - pr.dot(offs)).max())
    record('f23', 'oflow_tail2 logits %s' % (shape,), e_l, tol)
    record('f23', 'oflow_tail2 flow %s' % (shape,), e_f, 20 * tol)
    assert e_l <= tol, (e_l, tol)
    assert e_f <= 20 * tol, (e_f, 20 * tol)
    flow2, logits2 = _launch(*args)                                  # a second launch on the same inputs
    assert torch.equal(flow, flow2) and torch.equal(logits, logits2)
    flow3, _ = _launch(*args, with_logits=False)                     # without the optional logits output
    assert torch.equal(flow, flow3)
