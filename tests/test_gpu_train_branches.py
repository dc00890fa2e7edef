"""-m gpu: every launch branch of the weight gradients, the weight packs and the update launches that the op-level training
tests (test_gpu_train.py, test_gpu_train_f16.py, test_gpu_flow_train.py) never take (case table: tests/train_branches.py; its
host checks: tests/test_train_branches_host.py).  Equality wherever the arithmetic is exact -- small integers, impulses, packs,
masks -- and the existing bounds, unchanged, on random data."""
import ctypes as C

import numpy as np
import pytest

import conv_tol
import train_branches as TB
import train_f16_ref as HR
import train_ref as R
from gpu_util import dev, stream, sync
from kfnet_amd import _lib
from test_gpu_train import run_input_grad, wgrad_bound
from test_gpu_train_f16 import DeviceScale, h16

pytestmark = pytest.mark.gpu

G = 64                                   # guard words behind every output
WGRAD_RUNS = [(c, t) for c in TB.WGRAD_CASES for t in sorted(c.plans)]
RUN_IDS = ['%s-%s' % (TB.wgrad_id(c), 'f16' if t else 'f32') for c, t in WGRAD_RUNS]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Wgrad(object):
    """kfn_conv2d_grad_weights for one case and operand type: x and dz in buffers of the case's pixel strides (7.0 / -3.0 between
    the rows' live parts), sentinels in dw, db and the workspace with guard words behind each."""

    def __init__(self, case, dtype):
        import torch
        self.lib, self.c = _lib.load(), case
        self.d = _lib.ConvDesc(N=case.N, H=case.H, W=case.W, Cin=case.cin, ldx=case.cin + case.ldx_pad, Cout=case.cout,
                               cout_pad=-(-case.cout // 32) * 32, ldy=case.ldz, kh=case.k, kw=case.k, stride=case.stride, operand_dtype=dtype)
        tn, tm, tnn, sp, ch = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_long()
        _lib.check(self.lib.kfn_conv2d_grad_weights_plan(C.byref(self.d), C.byref(tn), C.byref(tm), C.byref(tnn), C.byref(sp), C.byref(ch)),
                   'plan')
        self.P = TB.out_pixels(case)
        assert (tn.value, tm.value, tnn.value, sp.value, ch.value, self.P - (sp.value - 1) * ch.value) == tuple(case.plans[dtype])
        self.chunk = ch.value
        nb = C.c_size_t()
        _lib.check(self.lib.kfn_conv2d_grad_weights_workspace_bytes(C.byref(self.d), C.byref(nb)), 'workspace bytes')
        self.n_ws, self.n_dw = nb.value // 4, case.k * case.k * case.cin * case.cout
        self.ws = torch.full((self.n_ws + G,), -9.0, device='cuda')

    def __call__(self, x, dz, bias=True):
        import torch
        c = self.c
        xb = np.full((c.N * c.H * c.W, c.cin + c.ldx_pad), 7.0, np.float32)
        xb[:, :c.cin] = x.reshape(-1, c.cin)
        zb = np.full((self.P, c.ldz), -3.0, np.float32)
        zb[:, :c.cout] = dz.reshape(-1, c.cout)
        dw = torch.full((self.n_dw + G,), -5.0, device='cuda')
        db = torch.full((c.cout + G,), -5.0, device='cuda')
        self.ws.fill_(-9.0)
        xd, zd = dev(xb), dev(zb)
        _lib.check(self.lib.kfn_conv2d_grad_weights(C.byref(self.d), xd.data_ptr(), zd.data_ptr(), dw.data_ptr(),
                                                    db.data_ptr() if bias else None, self.ws.data_ptr(), stream()), 'kfn_conv2d_grad_weights')
        sync()
        dwh, dbh, wsh = dw.cpu().numpy(), db.cpu().numpy(), self.ws.cpu().numpy()
        assert np.all(dwh[self.n_dw:] == -5.0), 'wrote past dw'
        assert np.all(wsh[self.n_ws:] == -9.0), 'wrote past the workspace'
        if bias:
            assert np.all(dbh[c.cout:] == -5.0), 'wrote past db'
        else:
            assert np.all(dbh == -5.0), 'db == NULL, and something was written to the buffer that would have been db'
        return dwh[:self.n_dw].reshape(c.k, c.k, c.cin, c.cout), dbh[:c.cout]


# ---- weight gradients ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,dtype', WGRAD_RUNS, ids=RUN_IDS)
def test_weight_gradient_of_small_integers_is_exact(case, dtype):
    """x in {0..3}, dz in {-2..2}: operands are exact halfs and every partial sum is an integer below 6 * 1710 < 2^24, so dw and
    db must EQUAL the integer reference with fp32 and with fp16 operands -- a pixel dropped or counted twice at a run or stage
    seam, a wrong column of a ragged tile or a lost bias row is off by an integer.  Cases of WGRAD_NO_BIAS once more with
    db == NULL: the same dw, nothing written where db would be."""
    run = Wgrad(case, dtype)
    x, dz = TB.integer_operands(np.random.default_rng([11, TB.WGRAD_CASES.index(case)]), case)
    dw, db = run(x, dz)
    rw, rb = TB.wgrad_ref(x, dz, case.k, case.stride)
    bad = np.argwhere(dw != rw)
    assert bad.size == 0, '%d of %d entries of dw differ, first at [kh,kw,ci,co] = %s' % (len(bad), rw.size, bad[0])
    assert np.array_equal(db, rb), 'db differs at channels %s' % np.flatnonzero(db != rb)[:8]
    assert np.count_nonzero(rw) >= rw.size // 16
    if case.name in TB.WGRAD_NO_BIAS:
        dw2, _ = run(x, dz, bias=False)
        assert np.array_equal(_bits(dw2), _bits(dw))


@pytest.mark.parametrize('case,dtype', WGRAD_RUNS, ids=RUN_IDS)
def test_weight_gradient_of_seam_impulses_is_exact(case, dtype):
    """dz = 1.0 at one pixel per output channel -- the pixels cycle through both ends of the first two runs, the last pixel, both
    sides of the first image seam and of the first stage seam -- and random x: every dw[kh][kw][ci][co] is ONE product 1 * x plus zeros, so it must
    EQUAL the x value under that tap (rounded once to half for fp16 operands), 0 in the padding, and db must be exactly 1."""
    run = Wgrad(case, dtype)
    per_image = run.P // case.N
    pixels = TB.seam_pixels(run.P, run.chunk, per_image, TB.STAGE[dtype])
    x = TB.signed_floats(np.random.default_rng([12, TB.WGRAD_CASES.index(case)]), (case.N, case.H, case.W, case.cin))
    dw, db = run(x, TB.impulse_dz(case, pixels))
    want = TB.impulse_wgrad_ref(h16(x) if dtype == TB.F16 else x, case, pixels)
    bad = np.argwhere(dw != want)
    assert bad.size == 0, '%d of %d entries of dw differ, first at [kh,kw,ci,co] = %s (impulses at %s)' % (len(bad), want.size, bad[0], pixels)
    assert np.all(db == 1.0)
    assert np.count_nonzero(want) > 0 and (case.k == 1 or np.any(want == 0.0))       # live taps, and for 3x3 taps in the padding


@pytest.mark.parametrize('case,dtype', WGRAD_RUNS, ids=RUN_IDS)
def test_weight_gradient_of_random_data_against_fp64(case, dtype):
    """fp32 operands: test_conv_weight_gradient_against_fp64's wgrad_bound.  fp16 operands: the criterion of
    test_f16_weight_gradient_against_fp64_on_the_rounded_operands -- the same bound against the fp64 gradient of the ROUNDED
    operands, and farther than that from the gradient of the unrounded ones."""
    run = Wgrad(case, dtype)
    rng = np.random.default_rng([13, TB.WGRAD_CASES.index(case)])
    x = np.maximum(rng.normal(size=(case.N, case.H, case.W, case.cin)), 0).astype(np.float32)          # layer inputs are post-ReLU
    ho, wo = TB.same_pad(case.H, case.k, case.stride)[0], TB.same_pad(case.W, case.k, case.stride)[0]
    dz = rng.normal(size=(case.N, ho, wo, case.cout)).astype(np.float32)
    dw, db = run(x, dz)
    kshape = (case.k, case.k, case.cin, case.cout)
    xo, zo = (h16(x), h16(dz)) if dtype == TB.F16 else (x, dz)
    rw, rb = R.conv_grad_weights(xo, zo, kshape, case.stride)
    label = 'branch %s%s' % (TB.wgrad_id(case), ' f16' if dtype == TB.F16 else '')
    bound = wgrad_bound(xo, zo, run.P)
    err = float(np.abs(dw - rw).max())
    conv_tol.record('wgrad', label, err, bound)
    bb = wgrad_bound(np.ones(1), zo, run.P)
    eb = float(np.abs(db - rb).max())
    conv_tol.record('wgrad', label + ' bias', eb, bb)
    assert err <= bound
    assert eb <= bb
    if dtype == TB.F16:
        fw, _ = R.conv_grad_weights(x, dz, kshape, case.stride)
        assert float(np.abs(dw - fw).max()) > bound


@pytest.mark.parametrize('name', TB.WGRAD_RELAUNCH)
def test_fp32_weight_gradient_launches_are_bit_identical(name):
    case = next(c for c in TB.WGRAD_CASES if c.name == name)
    run = Wgrad(case, TB.F32)
    rng = np.random.default_rng([14, TB.WGRAD_CASES.index(case)])
    x = rng.normal(size=(case.N, case.H, case.W, case.cin)).astype(np.float32)
    dz = rng.normal(size=(case.N, case.H, case.W, case.cout)).astype(np.float32)
    a, b = run(x, dz), run(x, dz)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_weight_gradient_whose_reduction_takes_a_second_pass_is_exact():
    """1x1, Cin 2048, Cout 1025, 40 pixels: 2049 x 1025 = 2.1 M sums, 3073 more than wgrad_reduce_kernel's 8192 x 256 threads;
    the last two rows of dw and the bias row lie in the second pass.  Small integers: equality."""
    case = TB.REDUCE_CASE
    run = Wgrad(case, TB.F32)
    assert TB.GRID_8192 < run.n_dw + case.cout < 2 * TB.GRID_8192
    x, dz = TB.integer_operands(np.random.default_rng(15), case)
    dw, db = run(x, dz)
    rw, rb = TB.wgrad_ref(x, dz, 1, 1)
    assert np.array_equal(dw, rw), '%d entries of dw differ' % int((dw != rw).sum())
    assert np.array_equal(db, rb)
    dw2, _ = run(x, dz, bias=False)
    assert np.array_equal(_bits(dw2), _bits(dw))


# ---- the first convolution's gradient --------------------------------------------------------------------------------------------
def _first_wgrad(img, dz, C1, bias=True):
    import torch
    lib = _lib.load()
    n, h, w, _ = img.shape
    nb = C.c_size_t()
    _lib.check(lib.kfn_first_conv_u8_grad_weights_workspace_bytes(n, h, w, C1, C.byref(nb)), 'workspace bytes')
    assert nb.value == -(-n * h * w // TB.FC_CHUNK) * 28 * C1 * 4
    ws = torch.full((nb.value // 4 + G,), -9.0, device='cuda')
    dw = torch.full((27 * C1 + G,), -5.0, device='cuda')
    db = torch.full((C1 + G,), -5.0, device='cuda')
    imd, zd = dev(img), dev(dz)
    _lib.check(lib.kfn_first_conv_u8_grad_weights(imd.data_ptr(), n, h, w, zd.data_ptr(), C1, dw.data_ptr(), db.data_ptr() if bias else None,
                                                  ws.data_ptr(), stream()), 'kfn_first_conv_u8_grad_weights')
    sync()
    dwh, dbh, wsh = dw.cpu().numpy(), db.cpu().numpy(), ws.cpu().numpy()
    assert np.all(dwh[27 * C1:] == -5.0) and np.all(wsh[nb.value // 4:] == -9.0)
    assert np.all(dbh[C1:] == -5.0) if bias else np.all(dbh == -5.0)
    return dwh[:27 * C1].reshape(27, C1), dbh[:C1]


@pytest.mark.parametrize('C1', TB.FIRST_WIDTHS)
@pytest.mark.parametrize('shape', TB.FIRST_IMAGES, ids=lambda s: '%dx%dx%d' % s)
def test_first_conv_weight_gradient_at_every_width(shape, C1):
    """kfn_first_conv_u8_grad_weights at C1 = 16, 32, 48 (threads hold fewer than 7 sums, some none) and 64, on images whose
    2048-pixel chunks and 64-pixel blocks do not end flush.  Random data: test_first_conv_weight_gradient_against_fp64's bound.
    Impulses (dz = 1.0 at one pixel per channel: image corners, both sides of the chunk seam and of an image seam, the last
    pixel): every dw[k][c] must EQUAL float32((float32(v) - 128) * 0.00625f) of the pixel under the tap, 0 in the padding --
    one rounded product, then additions of zeros -- and db must be 1.  db == NULL once: the same dw."""
    n, h, w = shape
    P = n * h * w
    rng = np.random.default_rng([16, TB.FIRST_IMAGES.index(shape), C1])
    img = rng.integers(0, 256, size=(n, h, w, 3)).astype(np.uint8)
    dz = rng.normal(size=(n, h, w, C1)).astype(np.float32)
    dw, db = _first_wgrad(img, dz, C1)
    x = (img.astype(np.float64) - 128.0) * 0.00625
    rw, rb = R.conv_grad_weights(x, dz, (3, 3, 3, C1), 1)
    label = 'branch conv1a %dx%dx%d C1=%d' % (n, h, w, C1)
    bound, bb = wgrad_bound(x, dz, P), wgrad_bound(np.ones(1), dz, P)
    err, eb = float(np.abs(dw - rw.reshape(27, C1)).max()), float(np.abs(db - rb).max())
    conv_tol.record('wgrad', label, err, bound)
    conv_tol.record('wgrad', label + ' bias', eb, bb)
    assert err <= bound and eb <= bb
    dw2, _ = _first_wgrad(img, dz, C1, bias=False)
    assert np.array_equal(_bits(dw2), _bits(dw))
    pixels = TB.first_pixels(shape)
    iz = np.zeros((P, C1), np.float32)
    for ch in range(C1):
        iz[pixels[ch % len(pixels)], ch] = 1.0
    dw, db = _first_wgrad(img, iz, C1)
    want = TB.first_impulse_ref(img, C1, pixels)
    bad = np.argwhere(dw != want)
    assert bad.size == 0, '%d of %d entries differ, first at [k, c] = %s (impulses at %s)' % (len(bad), want.size, bad[0], pixels)
    assert np.all(db == 1.0)


# ---- grid-stride second passes ---------------------------------------------------------------------------------------------------
def test_relu_gradient_beyond_one_pass_of_its_grid():
    """32769 x 64 elements: 64 past 8192 blocks x 256 threads.  Wider buffers on both sides; a NaN and a -0.0 in y zero their
    gradient (the kernel keeps dz where y > 0 and nowhere else).  The whole dz buffer must EQUAL the masked one."""
    lib = _lib.load()
    P, Cc, ldy, ldz = 32769, 64, 72, 68
    assert P * Cc == TB.GRID_8192 + 64
    rng = np.random.default_rng(17)
    y = np.maximum(rng.normal(size=(P, ldy)), 0).astype(np.float32)
    g = rng.normal(size=(P, ldz)).astype(np.float32)
    y[:, Cc:] = 0.0                                 # the pad columns of y would zero the pad columns of dz, were they read for them
    y[5, 7], y[P - 1, Cc - 1], y[P - 1, 3], y[P - 1, 4] = np.nan, np.nan, -0.0, 1.2e-38
    yd, gd = dev(y), dev(g)
    _lib.check(lib.kfn_relu_grad(yd.data_ptr(), ldy, gd.data_ptr(), ldz, P, Cc, stream()), 'kfn_relu_grad')
    sync()
    want = g.copy()
    want[:, :Cc] = np.where(y[:, :Cc] > 0, g[:, :Cc], np.float32(0))
    assert want[5, 7] == 0 and want[P - 1, Cc - 1] == 0 and want[P - 1, 3] == 0 and want[P - 1, 4] == g[P - 1, 4]
    got = gd.cpu().numpy()
    assert np.array_equal(got, want), '%d elements differ' % int((got != want).sum())


def _device_packs(w, kind):
    """(fp32 pack, fp16 pack) of kfn_pack_conv_weights / _f16, guard words checked."""
    import torch
    lib = _lib.load()
    kh, kw, ci, co = w.shape
    nf = C.c_size_t()
    _lib.check(lib.kfn_pack_conv_weights_floats(kh, kw, ci, co, kind, C.byref(nf)), 'pack floats')
    f32 = torch.full((nf.value + G,), -7.0, device='cuda')
    f16 = torch.full((nf.value + G,), -7.0, dtype=torch.float16, device='cuda')
    wd = dev(w)
    _lib.check(lib.kfn_pack_conv_weights(wd.data_ptr(), kh, kw, ci, co, kind, f32.data_ptr(), stream()), 'kfn_pack_conv_weights')
    _lib.check(lib.kfn_pack_conv_weights_f16(wd.data_ptr(), kh, kw, ci, co, kind, f16.data_ptr(), stream()), 'kfn_pack_conv_weights_f16')
    sync()
    a, b = f32.cpu().numpy(), f16.cpu().numpy()
    assert np.all(a[nf.value:] == -7.0) and np.all(b[nf.value:] == np.float16(-7.0)), 'wrote past the pack'
    return a[:nf.value], b[:nf.value]


@pytest.mark.parametrize('kind', [_lib.PACK_FORWARD, _lib.PACK_INPUT_GRAD_S1, _lib.PACK_INPUT_GRAD_S2], ids=['forward', 's1', 's2'])
def test_packs_beyond_one_pass_and_ragged_packs_equal_the_layout_formulas(kind):
    """3x3x512x512: 2.36 M elements, the second pass of pack_weights_kernel's 8192 x 256 grid, float and half, element by element
    against the numpy restatement of the header's layout (the half pack = that matrix rounded once).  3x3x48x70 and 1x1x16x1:
    rows padded to 32 and columns to 16, every padding element exactly 0 (the 'cin_pad' rows and 'cout16' columns)."""
    rng = np.random.default_rng(18 + kind)
    for shape in (TB.PACK_BIG,) + TB.PACK_RAGGED:
        w = (rng.normal(size=shape) * 10.0 ** rng.uniform(-6, 1, size=shape)).astype(np.float32)
        want, live = TB.pack_ref(w, kind)
        f32, f16 = _device_packs(w, kind)
        assert f32.size == want.size and (shape != TB.PACK_BIG or want.size > TB.GRID_8192)
        f32, f16 = f32.reshape(want.shape), f16.reshape(want.shape)
        assert np.array_equal(_bits(f32), _bits(want)), (shape, int((f32 != want).sum()))
        assert np.array_equal(f16.view(np.uint16), want.astype(np.float16).view(np.uint16)), shape
        assert not f32[~live].any() and not f16[~live].any()
        assert shape == TB.PACK_BIG or (~live).sum() > 0


def _big_n():
    return TB.GRID_16384 + 3


def test_adam_step_beyond_one_pass_of_its_grid():
    """n = 16384 x 256 + 3: the last three elements are the second pass.  Two steps against the numpy formula, 2 ulp as
    test_adam_step_against_the_numpy_formula_over_three_steps; the tail is judged by itself as well."""
    lib = _lib.load()
    n = _big_n()
    rng = np.random.default_rng(19)
    w = rng.normal(size=n).astype(np.float32) * np.float32(0.1)
    w[:500] = 0.0
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    wd_, md, vd = dev(w), dev(m), dev(v)
    for t in (1, 2):
        g = (rng.normal(size=n) * 10.0 ** rng.uniform(-4, 0, size=n)).astype(np.float32)
        lr = 1e-4 * 0.5 ** (t / 7.0)
        gd = dev(g)
        _lib.check(lib.kfn_adam_step(wd_.data_ptr(), md.data_ptr(), vd.data_ptr(), gd.data_ptr(), n, R.adam_lr_t(lr, t), R.BETA1, R.BETA2,
                                     R.EPSILON, 1e-4, stream()), 'kfn_adam_step')
        sync()
        before = w[-3:].copy()
        w, m, v = R.adam_step(w, m, v, g, lr, t, 1e-4)
        for name, got, want in (('w', wd_, w), ('m', md, m), ('v', vd, v)):
            u = R.ulp_distance(got.cpu().numpy(), want)
            print('adam step %d %s: %.2f ulp, tail %.2f ulp' % (t, name, float(u.max()), float(u[-3:].max())))
            assert float(u.max()) <= 2.0
        assert not np.array_equal(w[-3:], before), 'the reference moves the tail'


def test_loss_scale_launches_beyond_one_pass_of_their_grids():
    """kfn_loss_scale_apply, kfn_loss_scale_unscale_check and kfn_adam_step_guarded at n = 16384 x 256 + 3, judged as
    test_loss_scale_launches_against_the_numpy_restatement judges them at n = 1000: products by the power-of-two scale are
    exact, the state record equals the numpy one, applied steps within 2 ulp.  Step 2 holds ONE inf, in the last three elements:
    only a thread's second pass can raise the flag, and w, m, v must come back bit for bit."""
    lib = _lib.load()
    n, scale, interval = _big_n(), 2.0 ** 10, 2
    rng = np.random.default_rng(20)
    w = (rng.normal(size=n) * 0.1).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    wd_, md, vd = dev(w), dev(m), dev(v)
    ds, ref = DeviceScale(scale), HR.LossScale(scale, interval)
    for step in (1, 2, 3):
        g = (rng.normal(size=n) * 10.0 ** rng.uniform(-6, -2, size=n)).astype(np.float32)
        gd = dev(g)
        _lib.check(lib.kfn_loss_scale_apply(gd.data_ptr(), n, ds.ptr, stream()), 'kfn_loss_scale_apply')
        sync()
        gs = gd.cpu().numpy()
        assert np.array_equal(gs, g * ref.scale)
        if step == 2:
            gs[n - 2] = np.inf
            gd = dev(gs)
        lr = 1e-4 * 0.5 ** (step / 7.0)
        before = (w.copy(), m.copy(), v.copy(), ref.adam_t, float(ref.scale), ref.skipped)
        _lib.check(lib.kfn_loss_scale_unscale_check(gd.data_ptr(), n, ds.ptr, stream()), 'kfn_loss_scale_unscale_check')
        sync()
        assert ds.read().overflow == int(step == 2)
        _lib.check(lib.kfn_adam_step_guarded(wd_.data_ptr(), md.data_ptr(), vd.data_ptr(), gd.data_ptr(), n, lr, R.BETA1, R.BETA2,
                                             R.EPSILON, 1e-4, interval, ds.ptr, stream()), 'kfn_adam_step_guarded')
        sync()
        unscaled = gd.cpu().numpy()
        ok = np.isfinite(gs)
        assert np.array_equal(unscaled[ok], (gs * (np.float32(1.0) / np.float32(before[4])))[ok])
        w, m, v = ref.step(w, m, v, gs, lr, 1e-4)
        st = ds.read()
        assert st.scale == float(ref.scale) and st.good_steps == ref.good_steps and st.skipped == ref.skipped
        assert st.adam_t == ref.adam_t and st.overflow == 0
        assert st.beta1_power == float(ref.beta1_power) and st.beta2_power == float(ref.beta2_power)
        got = [t.cpu().numpy() for t in (wd_, md, vd)]
        if step == 2:
            for a, b in zip(got, before[:3]):
                assert np.array_equal(_bits(a), _bits(b))
            assert ref.adam_t == before[3] and float(ref.scale) == before[4] / 2 and ref.skipped == before[5] + 1
        else:
            assert ref.adam_t == before[3] + 1
            for name, a, b in zip('wmv', got, (w, m, v)):
                u = R.ulp_distance(a, b)
                print('guarded adam step %d %s: %.2f ulp, tail %.2f ulp' % (step, name, float(u.max()), float(u[-3:].max())))
                assert float(u.max()) <= 2.0
    st = ds.read()
    assert st.adam_t == 2 and st.skipped == 1 and st.scale == scale / 2      # halved at step 2; two good steps need one more to double


# ---- input gradients on ragged packs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layer', TB.INPUT_GRAD_RAGGED, ids=lambda l: 'k%d-%dto%d' % l)
def test_input_gradient_on_ragged_packs(layer):
    """run_input_grad's launch (kfn_pack_conv_weights + kfn_conv2d_nhwc) where Cin is no multiple of 32 and Cout none of 16: the
    pack's zero rows ('cin_pad') and zero columns ('cout16') are multiplied.  Border impulses by equality, as
    test_input_gradient_of_border_impulses_is_exact; random data within conv_tol's 'direct' bound."""
    k, ci, co = layer
    H, Wd = 9, 13
    rng = np.random.default_rng([21, k, ci, co])
    w = rng.normal(size=(k, k, ci, co)).astype(np.float32)
    spots = [(0, 0), (0, Wd - 1), (H - 1, 0), (H - 1, Wd - 1), (0, Wd // 2), (H - 1, Wd // 2), (H // 2, 0), (H // 2, Wd - 1)]
    dz = np.zeros((len(spots), H, Wd, co), np.float32)
    for i, (r, c) in enumerate(spots):
        dz[i, r, c, (co - 1 - i) % co] = 1.0                  # the last channels first: column Cout - 1 borders the zero columns
    got = run_input_grad(dz, w, 1, (H, Wd))
    ref = R.conv_grad_input(dz, w, (H, Wd), 1)
    assert np.array_equal(got.astype(np.float64), ref)
    assert np.count_nonzero(ref) > 0
    w = (w / np.sqrt(k * k * ci)).astype(np.float32)
    dz = rng.normal(size=(2, H, Wd, co)).astype(np.float32)
    got = run_input_grad(dz, w, 1, (H, Wd))
    ref = R.conv_grad_input(dz, w, (H, Wd), 1)
    conv_tol.assert_close(got, ref, dz, w, 'direct', 'branch input gradient k%d %d->%d' % (k, ci, co), transposed=True)


# ---- the even-kernel pack --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', TB.EVEN_KERNELS, ids=lambda k: '%dx%d' % k)
def test_input_grad_s1_pack_of_an_even_kernel_is_refused(kernel):
    """SAME padding of an even kernel is asymmetric, so kfn_conv2d_nhwc on a KFN_PACK_INPUT_GRAD_S1 matrix would return the input
    gradient shifted by one pixel (tests/test_train_branches_host.py shows it with the oracle's convolution).  Both pack entry
    points refuse: KFN_ERR_ARG, a message that says why, nothing written.  The forward and the stride-2 packs of the same
    kernel are made as before."""
    import torch
    lib = _lib.load()
    kh, kw = kernel
    ci, co = 32, 16
    w = np.random.default_rng(kh * 10 + kw).normal(size=(kh, kw, ci, co)).astype(np.float32)
    wd = dev(w)
    f32 = torch.full((32 * kh * kw * 16 + G,), -7.0, device='cuda')
    f16 = torch.full((32 * kh * kw * 16 + G,), -7.0, dtype=torch.float16, device='cuda')
    assert lib.kfn_pack_conv_weights(wd.data_ptr(), kh, kw, ci, co, _lib.PACK_INPUT_GRAD_S1, f32.data_ptr(), stream()) == -1
    msg = lib.kfn_last_error()
    assert b'KFN_PACK_INPUT_GRAD_S1' in msg and b'odd' in msg and b'shifted' in msg, msg
    assert lib.kfn_pack_conv_weights_f16(wd.data_ptr(), kh, kw, ci, co, _lib.PACK_INPUT_GRAD_S1, f16.data_ptr(), stream()) == -1
    sync()
    assert bool((f32 == -7.0).all()) and bool((f16 == -7.0).all())
    for kind in (_lib.PACK_FORWARD, _lib.PACK_INPUT_GRAD_S2):
        want, _ = TB.pack_ref(w, kind)
        a, b = _device_packs(w, kind)
        assert np.array_equal(_bits(a.reshape(want.shape)), _bits(want))
        assert np.array_equal(b.reshape(want.shape).view(np.uint16), want.astype(np.float16).view(np.uint16))
