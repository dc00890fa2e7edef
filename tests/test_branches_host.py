"""Host checks of the launch-branch case table (tests/branches.py): through kfn_kalman_scan_plan -- the function the scan's
launcher decides by -- that the table reaches every form of the scan in both variants and that every boundary grid lands on the
side the table states; that kfn_kalman_scan_scratch_bytes is non-zero exactly for form 5; that the reference puts almost no pixel
into the gate's band; the refusal of transposed convolutions other than 3x3; and the test's own selector reference."""
import ctypes as C

import numpy as np
import pytest

from kfnet_amd import _lib
from oracle import kfnet_oracle as O
from tests import branches as B


def _plan(lib, H, W, with_opt, S=B.SCAN_S):
    d = _lib.KalmanDesc(S=S, T=B.SCAN_T, H=H, W=W, t0=B.SCAN_T0, reset_period=B.SCAN_RESET, min_uncertainty=1e-5)
    form, threads, ppt = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    _lib.check(lib.kfn_kalman_scan_plan(C.byref(d), int(with_opt), C.byref(form), C.byref(threads), C.byref(ppt)), 'scan plan')
    need = C.c_size_t(77)
    _lib.check(lib.kfn_kalman_scan_scratch_bytes(C.byref(d), C.byref(need)), 'scratch bytes')
    return form.value, threads.value, ppt.value, need.value


def test_scan_table_reaches_every_form_in_both_variants():
    lib = _lib.load()
    seen = set()
    for c in B.SCAN_CASES:
        for with_opt in (0, 1):
            form, threads, ppt, need = _plan(lib, c.H, c.W, with_opt)
            assert form == c.form, (c, with_opt, form)
            assert (threads, ppt) == B.SCAN_MAPPING[form][with_opt], (c, with_opt, threads, ppt)
            if form < 5:
                assert threads * ppt >= c.H * c.W, 'one workgroup covers the grid'
                assert threads % 64 == 0 and threads <= 1024
            # a second copy of the state exactly when it cannot live in the LDS
            assert need == (B.SCAN_S * c.H * c.W * 16 if form == 5 else 0), (c, need)
            seen.add((form, with_opt))
    assert seen == {(f, v) for f in (1, 2, 3, 4, 5) for v in (0, 1)}
    # the two variants of a form are different instantiations (other thread counts), which is why both are launched
    assert all(B.SCAN_MAPPING[f][0] != B.SCAN_MAPPING[f][1] for f in (1, 2, 3, 4))


def test_scan_table_holds_both_sides_of_every_limit():
    """Every limit L of the dispatcher has the grid of exactly L pixels (last of its form) and of L + 1 (first of the next) in the
    table, the smallest admitted grid is there, and forms 2 and 4 -- launched by no other test -- have an interior grid too.
    Asserted on the whole list of sizes, so that a case taken out of the table fails here."""
    sizes = sorted((c.H * c.W, c.form, c.role) for c in B.SCAN_CASES)
    want = [(4, 1, 'low')]
    for form, limit in enumerate(B.SCAN_LIMITS, start=1):
        want += [(limit, form, 'high'), (limit + 1, form + 1, 'low')]
    want += [(72 * 80, 2, 'interior'), (80 * 120, 4, 'interior')]
    assert sizes == sorted(want)
    lib = _lib.load()
    for form, limit in enumerate(B.SCAN_LIMITS, start=1):      # the limits themselves, at a grid that is not in the table
        assert _plan(lib, 2, limit // 2, 0)[0] == form and _plan(lib, 2, limit // 2, 1)[0] == form
        assert _plan(lib, 2, limit // 2 + 1, 0)[0] == form + 1 and _plan(lib, 2, limit // 2 + 1, 1)[0] == form + 1
    # the settings of the cases: half with the transform, the gate on the interior grids only
    assert sum(c.use_transform for c in B.SCAN_CASES) == len(B.SCAN_CASES) // 2
    assert all((c.nis_gate == B.NIS_GATE) == (c.role == 'interior') and c.nis_gate in (0.0, B.NIS_GATE) for c in B.SCAN_CASES)
    assert len({c.seed for c in B.SCAN_CASES}) == len(B.SCAN_CASES)


def test_scan_plan_refuses_bad_arguments_and_touches_no_device():
    lib = _lib.load()
    d = _lib.KalmanDesc(S=1, T=1, H=1, W=5)
    f, t, p = C.c_int(), C.c_int(), C.c_int()
    assert lib.kfn_kalman_scan_plan(C.byref(d), 0, C.byref(f), C.byref(t), C.byref(p)) == -1
    assert b'shape' in lib.kfn_last_error()
    d = _lib.KalmanDesc(S=1, T=1, H=4, W=5)
    assert lib.kfn_kalman_scan_plan(C.byref(d), 0, None, C.byref(t), C.byref(p)) == -1
    assert lib.kfn_kalman_scan_plan(None, 0, C.byref(f), C.byref(t), C.byref(p)) == -1
    # S plays no part in the decision; any non-zero flag means "with optional outputs"
    assert _plan(lib, 68, 120, 0, S=1)[:3] == _plan(lib, 68, 120, 0, S=256)[:3] == (3, 1024, 8)
    assert _plan(lib, 68, 120, 5)[:3] == (3, 512, 16)


@pytest.mark.parametrize('case', [c for c in B.SCAN_CASES if c.nis_gate > 0], ids=B.scan_id)
def test_reference_puts_almost_no_pixel_into_the_gate_band(case):
    """The seeds of the gated grids are chosen so that the fp32 reference has fewer than 0.1 % of its pixels within a relative 1e-5
    of the gate (those records are left out of the GPU comparison), and so that the gate fires and spares on many pixels."""
    from tests.test_gpu_ops import _scan_ref
    from kfnet_amd.synth import synthetic_transform
    flow, sig, meas, state0 = B.scan_inputs(case)
    T4 = O.get_transform(synthetic_transform()) if case.use_transform else None
    _, _, nis, _ = _scan_ref(flow, sig, meas, state0, T4, B.SCAN_T0, B.SCAN_RESET, case.nis_gate)
    band = B.gate_band(nis, case.nis_gate)
    assert band.mean() < B.GATE_BAND_MAX_FRACTION, band.mean()
    s = (nis[..., 0] + nis[..., 1]) + nis[..., 2]
    live = s[:, [0, 2]]                       # the two recursion frames (frame 1 is the reset: NIS 0)
    assert 0.05 < (live > case.nis_gate).mean() < 0.95, 'the gate decides something'


def test_transposed_convolution_is_refused_unless_3x3():
    """kfn_conv2d_plan runs the descriptor checks of kfn_conv2d_nhwc without a device: transposed = 1 with a kernel other than 3x3
    is KFN_ERR_ARG and says why; 3x3 transposed and the same sizes forward are planned."""
    lib = _lib.load()
    cfg, bk, tiles = C.c_int(), C.c_int(), C.c_int()

    def plan(**kw):
        f = dict(N=2, H=4, W=5, Cin=32, ldx=32, Cout=16, cout_pad=32, ldy=16, kh=3, kw=3, stride=2, transposed=1, relu=1)
        f.update(kw)
        d = _lib.ConvDesc(**f)
        return lib.kfn_conv2d_plan(C.byref(d), C.byref(cfg), C.byref(bk), C.byref(tiles))
    assert plan() == 0
    for kh, kw in B.DECONV_REFUSED + ((1, 3), (3, 1), (1, 1)):
        assert plan(kh=kh, kw=kw) == -1, (kh, kw)
        msg = lib.kfn_last_error()
        assert b'transposed' in msg and b'3x3' in msg and ('%dx%d' % (kh, kw)).encode() in msg, msg
        assert plan(kh=kh, kw=kw, transposed=0) == 0, (kh, kw)
    # the forward promise stands: every kh*kw <= 32 of the table is planned, 33 taps are not
    for kh, kw in B.CONV_KERNELS:
        assert plan(kh=kh, kw=kw, transposed=0, stride=1) == 0
    assert plan(kh=3, kw=11, transposed=0) == -1 and plan(kh=1, kw=33, transposed=0) == -1


def test_selector_reference_equals_the_oracle_convolution():
    """tests/branches.shifted_input (pure indexing) against O.conv2d_same with the selector kernel, even and odd sizes, both
    strides: the GPU selector cases compare with the former."""
    rng = np.random.default_rng(2)
    x = rng.integers(-4, 5, size=(2, 5, 9, 3)).astype(np.float64)
    for (kh, kw), stride in (((4, 8), 1), ((1, 32), 1), ((2, 2), 2), ((5, 5), 2), ((2, 7), 1)):
        for ky, kx in ((0, 0), (kh - 1, kw - 1), (kh // 2, kw // 2), (0, kw - 1)):
            w = np.zeros((kh, kw, 3, 3))
            w[ky, kx] = np.eye(3)
            assert np.array_equal(B.shifted_input(x, kh, kw, ky, kx, stride), O.conv2d_same(x, w, None, stride, False))


def test_case_tables_are_what_the_gpu_tests_expect():
    assert len(B.CONV_F32_CASES) == 72 and len({B.conv_id(c) for c in B.CONV_F32_CASES}) == 72
    assert len(B.CONV_MODE_CASES) == 9 and {c.mode for c in B.CONV_MODE_CASES} == {'f16', 'x3', 'act16'}
    assert all(kh * kw <= 32 for kh, kw in B.CONV_KERNELS) and (1, 32) in B.CONV_KERNELS and (32, 1) in B.CONV_KERNELS
    assert all(img[2] >= 40 for img in B.CONV_IMAGES)
    assert all(c.cin % 32 == 0 for c in B.CONV_MODE_CASES)          # fp16 operands stage 32 channels
