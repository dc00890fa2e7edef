"""-m gpu: every launch branch of the Kalman scan, the direct convolution at kernel sizes other than 1x1 / 3x3, the first
convolution's other head widths, and window / pad parameters other than 8 / 2 (case table: tests/branches.py; its host checks:
tests/test_branches_host.py).  Each kernel against the plain reference of the same operation that tests/test_gpu_ops.py uses."""
import ctypes as C

import numpy as np
import pytest

from oracle import kfnet_oracle as O
from tests import branches as B
from tests.conv_tol import assert_close

pytestmark = pytest.mark.gpu


# ---- Kalman scan -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', B.SCAN_CASES, ids=B.scan_id)
def test_kalman_scan_form_vs_oracle_and_production_equals_debug(case):
    """One call WITH opt_temp / opt_nis (the instantiation that has the optional stores: 768 x 7 or 512 x 12 / 16 / 20 pixels per
    thread) against the fp32 numpy scan, tolerances of test_kalman_scan_vs_oracle; then the same scan from the same initial state
    with NO optional output (the production instantiation: 1024 x 5 / 6 / 8 / 10): records and final state bit for bit the first
    call's -- the per-pixel arithmetic is elementwise and unfused, so nothing may depend on the thread mapping, the ring depth or
    where the mid-frame barrier falls.  Gated grids: a record whose NIS sum lies within a relative 1e-5 of the gate in the
    REFERENCE is left out of the comparison with the reference (fewer than 0.1 % of them, asserted), not of the bit comparison."""
    import torch
    from kfnet_amd import _lib
    from kfnet_amd.synth import synthetic_transform
    from tests.gpu_util import dev, stream, sync
    from tests.test_gpu_ops import _scan_ref
    lib = _lib.load()
    S, T, H, W = B.SCAN_S, B.SCAN_T, case.H, case.W
    flow, sig, meas, state0 = B.scan_inputs(case)
    T4 = O.get_transform(synthetic_transform()) if case.use_transform else None
    d = _lib.KalmanDesc(S=S, T=T, H=H, W=W, t0=B.SCAN_T0, reset_period=B.SCAN_RESET, min_uncertainty=1e-5,
                        nis_gate=case.nis_gate, has_transform=int(case.use_transform))
    if case.use_transform:
        for i, v in enumerate(T4[:3].reshape(-1)):
            d.transform[i] = float(v)
    for with_opt in (0, 1):       # the launcher decides by the same function
        form, threads, ppt = C.c_int(), C.c_int(), C.c_int()
        _lib.check(lib.kfn_kalman_scan_plan(C.byref(d), with_opt, C.byref(form), C.byref(threads), C.byref(ppt)), 'plan')
        assert form.value == case.form and (threads.value, ppt.value) == B.SCAN_MAPPING[case.form][with_opt]
    need = C.c_size_t(99)
    _lib.check(lib.kfn_kalman_scan_scratch_bytes(C.byref(d), C.byref(need)), 'scratch bytes')
    assert need.value == (S * H * W * 16 if case.form == 5 else 0)
    GUARD = 64
    scratch = torch.full((need.value // 4 + GUARD,), -7.0, device='cuda') if need.value else None
    dfl, dsg, dme = dev(flow), dev(sig), dev(meas)

    def launch(debug):
        st = dev(state0)
        rec = torch.full((S * T * H * W * 4 + GUARD,), -7.0, device='cuda')
        tmp = torch.full((S * T * H * W * 4 + GUARD,), -7.0, device='cuda') if debug else None
        nis = torch.full((S * T * H * W * 3 + GUARD,), -7.0, device='cuda') if debug else None
        _lib.check(lib.kfn_kalman_scan(C.byref(d), dfl.data_ptr(), dsg.data_ptr(), dme.data_ptr(), st.data_ptr(), rec.data_ptr(),
                                       tmp.data_ptr() if debug else None, nis.data_ptr() if debug else None,
                                       scratch.data_ptr() if scratch is not None else None, stream()), 'scan')
        sync()
        for name, buf, n in (('records', rec, S * T * H * W * 4), ('temp', tmp, S * T * H * W * 4), ('nis', nis, S * T * H * W * 3)):
            if buf is not None:
                assert bool((buf[n:] == -7.0).all()), 'the scan wrote past the end of %s' % name
        if scratch is not None:
            assert bool((scratch[need.value // 4:] == -7.0).all()), 'the scan wrote past its scratch copy'
        return rec[:S * T * H * W * 4], st, tmp, nis

    rec, st, tmp, nis = launch(True)
    r_rec, r_tmp, r_nis, r_state = _scan_ref(flow, sig, meas, state0, T4, B.SCAN_T0, B.SCAN_RESET, case.nis_gate)
    g_rec = rec.cpu().numpy().reshape(r_rec.shape)
    g_state = st.cpu().numpy().reshape(r_state.shape)
    g_tmp = tmp.cpu().numpy()[:r_tmp.size].reshape(r_tmp.shape)
    g_nis = nis.cpu().numpy()[:r_nis.size].reshape(r_nis.shape)
    keep = np.ones(r_rec.shape[:4], bool)
    if case.nis_gate > 0:
        band = B.gate_band(r_nis, case.nis_gate)
        print('%s: %d of %d pixel-frames within %.0e of the gate' % (B.scan_id(case), band.sum(), band.size, B.GATE_BAND))
        assert band.mean() < B.GATE_BAND_MAX_FRACTION
        keep = ~band
    print('%s: max abs diff temp %.3g state %.3g records %.3g' % (
        B.scan_id(case), np.abs(g_tmp - r_tmp).max(), np.abs(g_state - r_state).max(), np.abs(g_rec - r_rec)[keep].max()))
    # elementwise fp32 with the same op order: a few ulps (transform matmul order aside)
    assert np.allclose(g_tmp, r_tmp, rtol=2e-6, atol=2e-6)
    assert np.allclose(g_state, r_state, rtol=4e-6, atol=4e-6)
    assert np.allclose(g_rec[keep][:, 0:3], r_rec[keep][:, 0:3], rtol=1e-5, atol=1e-5)
    assert np.allclose(g_rec[keep][:, 3], r_rec[keep][:, 3], rtol=1e-5)
    if case.nis_gate == 0.0:
        assert np.allclose(g_nis, r_nis, rtol=1e-4, atol=1e-6)
    # the production instantiation: same bits
    rec2, st2, _, _ = launch(False)
    assert torch.equal(rec2, rec), '%d record words differ between the two instantiations' % int((rec2 != rec).sum())
    assert torch.equal(st2, st), '%d state words differ between the two instantiations' % int((st2 != st).sum())


# ---- direct convolution at other kernel sizes --------------------------------------------------------------------------------
def _conv_operands(c):
    n, h, w = c.img
    rng = np.random.default_rng(B.conv_seed(c))
    K = c.kh * c.kw * c.cin
    if c.mode == 'x3':      # as test_conv_f16x3_split_operands: post-ReLU activations, He weights
        x = np.maximum(rng.normal(size=(n, h, w, c.cin)), 0).astype(np.float32) * 3
        wt = (rng.normal(size=(c.kh, c.kw, c.cin, c.cout)) * np.sqrt(2.0 / K)).astype(np.float32)
    else:
        x = rng.normal(size=(n, h, w, c.cin)).astype(np.float32)
        wt = (rng.normal(size=(c.kh, c.kw, c.cin, c.cout)) / np.sqrt(K)).astype(np.float32)
    b = rng.normal(size=c.cout).astype(np.float32)
    return x, wt, b


@pytest.mark.parametrize('case', B.CONV_F32_CASES, ids=B.conv_id)
def test_conv_kernel_sizes_fp32(case):
    """fp32 operands, bias and ReLU, against the fp64 SAME convolution (asymmetric padding for even sizes); conv_tol's 'direct'
    bound.  A 1x32 kernel used to return the bias alone at every pixel with all 32 columns live (a shift by 32 in the tap mask)."""
    from tests.gpu_util import run_conv
    x, wt, b = _conv_operands(case)
    y = run_conv(x, wt, b, case.stride, True)
    ref = O.conv2d_same(x.astype(np.float64), wt, b, case.stride, True)
    assert y.shape == ref.shape
    assert_close(y, ref, x, wt, 'direct', 'branch ' + B.conv_id(case))


@pytest.mark.parametrize('case', B.CONV_MODE_CASES, ids=B.conv_id)
def test_conv_kernel_sizes_operand_modes(case):
    """The other loaders at 5x5, 2x2 and 1x32.  'f16': against the fp64 convolution of the fp16-ROUNDED operands, 'direct' bound
    (test_conv_fp16_operands).  'x3': against the fp64 convolution of the original operands, 'f16x3' bound
    (test_conv_f16x3_split_operands).  'act16': the input holds halfs, the weights are rounded to halfs, the output is ONE rounding
    of the fp32 result to half: 'direct' bound + half an fp16 ulp of the result (2^-11 relative; test_conv_fp16_activations)."""
    from tests.gpu_util import run_conv
    x, wt, b = _conv_operands(case)
    label = 'branch ' + B.conv_id(case)
    if case.mode == 'f16':
        y = run_conv(x, wt, b, 1, True, f16=True)
        ref = O.conv2d_same(x.astype(np.float16).astype(np.float64), wt.astype(np.float16).astype(np.float64), b, 1, True)
        assert_close(y, ref, x, wt, 'direct', label)
        full = O.conv2d_same(x.astype(np.float64), wt, b, 1, True)
        assert np.abs(y - full).max() > 0      # it really is reduced precision
    elif case.mode == 'x3':
        y = run_conv(x, wt, b, 1, True, x3=True)
        ref = O.conv2d_same(x.astype(np.float64), wt, b, 1, True)
        assert_close(y, ref, x, wt, 'f16x3', label)
    else:
        x = x.astype(np.float16)
        y = run_conv(x, wt, b, 1, True, f16=True, x16=True, y16=True)
        ref = O.conv2d_same(x.astype(np.float64), wt.astype(np.float16).astype(np.float64), b, 1, True)
        assert_close(y, ref, x.astype(np.float32), wt, 'direct', label, extra=np.abs(ref) * 2.0 ** -11 + 1e-7)
    assert y.shape == ref.shape


@pytest.mark.parametrize('kernel', B.SELECTOR_KERNELS, ids=lambda k: '%dx%d' % k)
def test_conv_selector_weights_pick_exactly_one_tap(kernel):
    """Weights 1 at one tap (channel c -> channel c) and 0 at every other, for every tap in turn, on small integers: every product
    and sum is exact, so the output IS the input shifted by that tap -- a dropped, doubled or displaced tap is an O(1) error."""
    from tests.gpu_util import run_conv
    kh, kw = kernel
    rng = np.random.default_rng(kh * 100 + kw)
    x = rng.integers(-8, 9, size=(2, 7, 41, 16)).astype(np.float32)
    for ky in range(kh):
        for kx in range(kw):
            wt = np.zeros((kh, kw, 16, 16), np.float32)
            wt[ky, kx] = np.eye(16, dtype=np.float32)
            y = run_conv(x, wt, None, 1, False)
            want = B.shifted_input(x, kh, kw, ky, kx)
            assert np.array_equal(y, want), 'tap (%d,%d) of %dx%d: %d outputs differ' % (ky, kx, kh, kw, int((y != want).sum()))


@pytest.mark.parametrize('kernel', B.DECONV_REFUSED, ids=lambda k: '%dx%d' % k)
def test_transposed_conv_other_than_3x3_is_refused(kernel):
    """conv2d_transpose exists for the networks' 3x3 kernels only: another size is KFN_ERR_ARG with a message, and nothing is
    launched (the output keeps its sentinel)."""
    import torch
    from kfnet_amd import _lib
    from tests.gpu_util import dev, stream, sync
    lib = _lib.load()
    kh, kw = kernel
    x = dev(np.ones((2 * 4 * 5, 32), np.float32))
    w = dev(np.ones((32, kh * kw * 32), np.float32))
    y = torch.full((2 * 8 * 10 * 16 + 64,), -123.0, device='cuda')
    d = _lib.ConvDesc(N=2, H=4, W=5, Cin=32, ldx=32, Cout=16, cout_pad=32, ldy=16, kh=kh, kw=kw, stride=2, transposed=1, relu=1)
    assert lib.kfn_conv2d_nhwc(C.byref(d), x.data_ptr(), w.data_ptr(), None, y.data_ptr(), stream()) == -1
    msg = lib.kfn_last_error()
    assert b'transposed' in msg and b'3x3' in msg, msg
    sync()
    assert bool((y == -123.0).all())


# ---- first convolution: the other head widths -------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', B.FIRST_IMAGES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('widths', B.FIRST_WIDTHS, ids=lambda s: '%d+%d' % s)
def test_first_conv_other_head_widths(widths, hw):
    """kfn_first_conv_u8 at head widths (16,0), (32,0), (16,64), (32,16) against the fp64 convolution of the preprocessed image
    (bound of test_first_conv_u8), guard words behind both outputs; fp16 output at those widths is KFN_ERR_UNSUPPORTED and
    writes nothing."""
    import torch
    from kfnet_amd import _lib
    from tests.gpu_util import dev, stream, sync
    lib = _lib.load()
    (H, W), (C1, C2), N = hw, widths, 2
    rng = np.random.default_rng(C1 * 100 + C2 + H)
    img = rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)
    w1 = (rng.normal(size=(3, 3, 3, C1)) / 5).astype(np.float32)
    b1 = rng.normal(size=C1).astype(np.float32)
    w2 = (rng.normal(size=(3, 3, 3, max(C2, 1))) / 5).astype(np.float32)
    b2 = rng.normal(size=max(C2, 1)).astype(np.float32)
    n1, n2 = N * H * W * C1, N * H * W * C2
    y1 = torch.full((n1 + 256,), -3.0, device='cuda')
    y2 = torch.full((n2 + 256,), -3.0, device='cuda')
    di, dw1, db1 = dev(img), dev(w1.reshape(27, C1)), dev(b1)
    dw2, db2 = dev(w2.reshape(27, -1)), dev(b2)
    second = (dw2.data_ptr(), db2.data_ptr(), y2.data_ptr(), C2) if C2 else (None, None, None, 0)
    # fp16 output first: refused, both buffers keep their sentinel
    rc = lib.kfn_first_conv_u8_ex(di.data_ptr(), N, H, W, dw1.data_ptr(), db1.data_ptr(), y1.data_ptr(), C1, _lib.ACT_F16,
                                  *(second + (stream(),)))
    assert rc == -3 and b'fp16' in lib.kfn_last_error()
    sync()
    assert bool((y1 == -3.0).all()) and bool((y2 == -3.0).all())
    _lib.check(lib.kfn_first_conv_u8(di.data_ptr(), N, H, W, dw1.data_ptr(), db1.data_ptr(), y1.data_ptr(), C1,
                                     *(second + (stream(),))), 'first')
    sync()
    xp = O.preprocess(img, np.float64)
    g1, g2 = y1.cpu().numpy(), y2.cpu().numpy()
    assert np.all(g1[n1:] == -3.0) and np.all(g2[n2:] == -3.0)
    r1 = O.conv2d_same(xp, w1, b1, 1, True)
    e1 = np.abs(g1[:n1].reshape(r1.shape) - r1).max()
    e2 = 0.0
    if C2:
        r2 = O.conv2d_same(xp, w2, b2, 1, True)
        e2 = np.abs(g2[:n2].reshape(r2.shape) - r2).max()
    print('first conv %d+%d %dx%d: max err %.3g / %.3g' % (C1, C2, H, W, e1, e2))
    assert e1 < 2e-5 and e2 < 2e-5


# ---- windows and pads ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('window', B.WINDOWS)
def test_cost_volume_other_windows_bit_exact(window):
    import torch
    from kfnet_amd import _lib
    from tests.gpu_util import dev, stream, sync
    lib = _lib.load()
    rng = np.random.default_rng(40 + window)
    N, H, W, Cc = 2, 5, 7, 8
    f = rng.normal(size=(N + 1, H, W, Cc)).astype(np.float32)
    fd = dev(f)
    n = N * H * W * window * window * Cc
    vol = torch.full((n + 64,), -9.0, device='cuda')
    _lib.check(lib.kfn_cost_volume(fd.data_ptr(), fd.data_ptr() + H * W * Cc * 4, vol.data_ptr(), N, H, W, Cc, window, stream()), 'cv')
    sync()
    got = vol.cpu().numpy()
    assert np.all(got[n:] == -9.0)
    got = got[:n].reshape(N, H * W, window, window, Cc)
    for i in range(N):
        ref, _ = O.coord_volume(f[i:i + 1], f[i + 1:i + 2], window)
        assert np.array_equal(got[i], ref)   # subtraction only: bit exact


@pytest.mark.parametrize('window', B.WINDOWS)
def test_flow_softargmax_other_windows(window):
    """window^2 = 4 ... 256 cells on a 64-lane wave: fewer cells than lanes, and up to four trips of the k += 64 loop.  Probabilities
    within 1e-6 of the fp64 softmax, flow within 5e-6 * window / 8 (the bound at window 8 scaled by the largest offset that
    multiplies a probability), uniform logits exactly (-0.5, -0.5), the same flow bits without the probability output."""
    import torch
    from kfnet_amd import _lib
    from tests.gpu_util import dev, stream, sync
    lib = _lib.load()
    rng = np.random.default_rng(60 + window)
    P, A = 1003, window * window
    logits = (rng.normal(size=(P, A)) * 4).astype(np.float32)
    flow = torch.full((P * 2 + 64,), -9.0, device='cuda')
    flow2 = torch.full((P * 2 + 64,), -9.0, device='cuda')
    prob = torch.full((P * A + 64,), -9.0, device='cuda')
    dl = dev(logits)
    _lib.check(lib.kfn_flow_softargmax(dl.data_ptr(), flow.data_ptr(), prob.data_ptr(), P, window, stream()), 'flow')
    _lib.check(lib.kfn_flow_softargmax(dl.data_ptr(), flow2.data_ptr(), None, P, window, stream()), 'flow (no prob)')
    sync()
    pr = O.softmax(logits.astype(np.float64))
    offs = O.coord_volume(np.zeros((1, 2, 2, 1)), np.zeros((1, 2, 2, 1)), window)[1]
    g_prob, g_flow = prob.cpu().numpy(), flow.cpu().numpy()
    assert np.all(g_prob[P * A:] == -9.0) and np.all(g_flow[P * 2:] == -9.0)
    e_p = np.abs(g_prob[:P * A].reshape(P, A) - pr).max()
    e_f = np.abs(g_flow[:P * 2].reshape(P, 2) - pr.dot(offs)).max()
    print('softargmax window %d: prob err %.3g, flow err %.3g (bound %.3g)' % (window, e_p, e_f, 5e-6 * window / 8))
    assert e_p < 1e-6
    assert e_f < 5e-6 * window / 8
    assert torch.equal(flow2, flow)
    dl = dev(np.zeros((4, A), np.float32))
    _lib.check(lib.kfn_flow_softargmax(dl.data_ptr(), flow.data_ptr(), None, 4, window, stream()), 'flow (uniform)')
    sync()
    assert np.all(flow.cpu().numpy()[:8] == -0.5)


@pytest.mark.parametrize('pad', B.PADS)
def test_pad_nhwc_other_pads(pad):
    import torch
    from kfnet_amd import _lib
    from tests.gpu_util import dev, stream, sync
    lib = _lib.load()
    rng = np.random.default_rng(80 + pad)
    N, H, W, Cc = 2, 5, 7, 8
    x = rng.normal(size=(N, H, W, Cc)).astype(np.float32)
    n = N * (H + 2 * pad) * (W + 2 * pad) * Cc
    y = torch.full((n + 64,), -9.0, device='cuda')
    dx = dev(x)
    _lib.check(lib.kfn_pad_nhwc(dx.data_ptr(), y.data_ptr(), N, H, W, Cc, pad, stream()), 'pad')
    sync()
    got = y.cpu().numpy()
    assert np.all(got[n:] == -9.0)
    want = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    assert np.array_equal(got[:n].reshape(want.shape), want)
