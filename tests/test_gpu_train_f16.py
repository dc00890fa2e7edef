"""Mixed-precision training of SCoordNet on the device: the fp16-operand weight gradient against fp64 on the
rounded operands and exactly on small integers, the half packs, the loss-scale launches against their numpy restatement,
and the trainer with precision='fp16' against the emulation of tests/train_f16_ref.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import conv_tol
import train_f16_ref as HR
import train_ref as R
from gpu_util import dev, stream, sync
from kfnet_amd import _lib
from test_gpu_train import wgrad_bound

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (64, 96)
F16 = _lib.OPERAND_F16


def h16(a):
    """Rounded to IEEE half and widened: what the kernel multiplies."""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


# -- 1. the weight gradient --------------------------------------------------------------------------------------------------
def wgrad_call(x, dz, k, stride, ldx_pad=16, ldz_pad=4, operand_dtype=F16, z_off=0):
    """One kfn_conv2d_grad_weights launch with x and dz in wider buffers; returns (rc, dw, db)."""
    import torch
    lib = _lib.load()
    n, h, w, ci = x.shape
    _, ho, wo, co = dz.shape
    ldx, ldz = ci + ldx_pad, co + ldz_pad
    xb = np.full((n * h * w, ldx), 7.0, np.float32)
    xb[:, :ci] = x.reshape(-1, ci)
    zb = np.full((n * ho * wo * ldz + 4,), -3.0, np.float32)
    zb[z_off:z_off + n * ho * wo * ldz].reshape(-1, ldz)[:, :co] = dz.reshape(-1, co)
    d = _lib.ConvDesc(N=n, H=h, W=w, Cin=ci, ldx=ldx, Cout=co, cout_pad=-(-co // 32) * 32, ldy=ldz, kh=k, kw=k, stride=stride,
                      operand_dtype=operand_dtype)
    nb = C.c_size_t()
    rc = lib.kfn_conv2d_grad_weights_workspace_bytes(C.byref(d), C.byref(nb))
    if rc != _lib.KFN_OK:
        return rc, None, None
    G = 64
    ws = torch.full((nb.value // 4 + G,), -9.0, device='cuda')
    dw = torch.full((k * k * ci * co + G,), -5.0, device='cuda')
    db = torch.full((co + G,), -5.0, device='cuda')
    xd, zd = dev(xb), dev(zb)
    rc = lib.kfn_conv2d_grad_weights(C.byref(d), xd.data_ptr(), zd.data_ptr() + 4 * z_off, dw.data_ptr(), db.data_ptr(),
                                     ws.data_ptr(), stream())
    if rc != _lib.KFN_OK:
        return rc, None, None
    sync()
    dwh, dbh, wsh = dw.cpu().numpy(), db.cpu().numpy(), ws.cpu().numpy()
    assert np.all(dwh[-G:] == -5.0) and np.all(dbh[-G:] == -5.0), 'wrote past dw / db'
    assert np.all(wsh[-G:] == -9.0), 'wrote past the workspace'
    return rc, dwh[:-G].reshape(k, k, ci, co), dbh[:-G]


def run_wgrad(x, dz, k, stride, **kw):
    rc, dw, db = wgrad_call(x, dz, k, stride, **kw)
    _lib.check(rc, 'kfn_conv2d_grad_weights')
    return dw, db


# (Cin, Cout, kernel, stride): one accumulator column per wave (Cout 64) and two, stride 2, several k tiles, 1x1
WGRAD_SHAPES = [(64, 64, 3, 1), (64, 256, 3, 2), (512, 512, 3, 1), (256, 128, 1, 1)]
# 234 pixels: one run with a ragged last stage; 2240: several runs, the last one ragged
WGRAD_SIZES = [(2, 9, 13), (1, 40, 56)]


def _check_against_fp64(x, dz, k, s, label):
    n, h, w, ci = x.shape
    co = dz.shape[3]
    dw, db = run_wgrad(x, dz, k, s)
    x16, z16 = h16(x), h16(dz)
    rw, rb = R.conv_grad_weights(x16, z16, (k, k, ci, co), s)
    P = dz.shape[0] * dz.shape[1] * dz.shape[2]
    # products of halfs are exact in fp32: what is left is the fp32 accumulation over the pixels, DESIGN 6b's model
    bound = wgrad_bound(x16, z16, P)
    err = float(np.abs(dw - rw).max())
    conv_tol.record('wgrad16', label, err, bound)
    assert err <= bound
    bb = wgrad_bound(np.ones(1), z16, P)
    eb = float(np.abs(db - rb).max())
    conv_tol.record('wgrad16', label + ' bias', eb, bb)
    assert eb <= bb
    # ... and it IS reduced precision: the fp64 gradient of the unrounded operands is somewhere else
    fw, _ = R.conv_grad_weights(x, dz, (k, k, ci, co), s)
    assert float(np.abs(dw - fw).max()) > bound


@pytest.mark.parametrize('size', WGRAD_SIZES, ids=['2x9x13', '1x40x56'])
@pytest.mark.parametrize('shape', WGRAD_SHAPES, ids=['%d-%d-k%d-s%d' % s for s in WGRAD_SHAPES])
def test_f16_weight_gradient_against_fp64_on_the_rounded_operands(shape, size):
    ci, co, k, s = shape
    n, h, w = size
    rng = np.random.default_rng([WGRAD_SHAPES.index(shape), WGRAD_SIZES.index(size)])
    x = np.maximum(rng.normal(size=(n, h, w, ci)), 0).astype(np.float32)          # layer inputs are post-ReLU
    dz = rng.normal(size=(n, -(-h // s), -(-w // s), co)).astype(np.float32)
    _check_against_fp64(x, dz, k, s, '%d->%d k%d s%d %dx%dx%d' % (ci, co, k, s, n, h, w))


def test_f16_weight_gradient_of_conv4b_at_its_production_size():
    rng = np.random.default_rng(44)
    x = np.maximum(rng.normal(size=(1, 60, 80, 1024)), 0).astype(np.float32)
    dz = rng.normal(size=(1, 60, 80, 1024)).astype(np.float32)
    _check_against_fp64(x, dz, 3, 1, 'conv4b 1x60x80')


def _integer_operands(rng, n, h, w, ci, co, s):
    x = rng.integers(0, 4, size=(n, h, w, ci)).astype(np.float32)
    dz = rng.integers(-2, 3, size=(n, -(-h // s), -(-w // s), co)).astype(np.float32)
    return x, dz


@pytest.mark.parametrize('size', WGRAD_SIZES, ids=['2x9x13', '1x40x56'])
@pytest.mark.parametrize('shape', WGRAD_SHAPES, ids=['%d-%d-k%d-s%d' % s for s in WGRAD_SHAPES])
def test_f16_weight_gradient_of_small_integers_is_exact(shape, size):
    """x in {0..3}, dz in {-2..2}: every partial sum is an integer below 2^24, so every entry of dw and db must EQUAL the
    integer reference -- a transposed LDS read that takes a wrong chunk, a dropped border tap or a lost bias row shows."""
    ci, co, k, s = shape
    n, h, w = size
    x, dz = _integer_operands(np.random.default_rng([7, ci, co, h]), n, h, w, ci, co, s)
    dw, db = run_wgrad(x, dz, k, s)
    rw, rb = R.conv_grad_weights(x, dz, (k, k, ci, co), s)
    assert np.array_equal(dw.astype(np.float64), rw)
    assert np.array_equal(db.astype(np.float64), rb)
    assert np.count_nonzero(rw) > rw.size // 2


@pytest.mark.parametrize('stride', [1, 2])
def test_f16_weight_gradient_of_corner_impulses_is_exact(stride):
    """x is a single 1 at each of the four corners (one image each): dw holds copies of single dz values, at the taps that
    reach the corner and nowhere else."""
    rng = np.random.default_rng(8)
    ci, co, h, w = 64, 64, 9, 13
    corners = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    for i, (r, c) in enumerate(corners):
        x = np.zeros((2, h, w, ci), np.float32)
        x[i % 2, r, c, 5 + 17 * i] = 1.0
        dz = rng.integers(-2, 3, size=(2, -(-h // stride), -(-w // stride), co)).astype(np.float32)
        dw, db = run_wgrad(x, dz, 3, stride)
        rw, rb = R.conv_grad_weights(x, dz, (3, 3, ci, co), stride)
        assert np.array_equal(dw.astype(np.float64), rw), (r, c)
        assert np.array_equal(db.astype(np.float64), rb), (r, c)
        assert np.count_nonzero(rw) > 0


def test_f16_weight_gradient_launches_are_bit_identical_and_f32_is_untouched():
    rng = np.random.default_rng(3)
    ci, co, k, s = 64, 256, 3, 2
    x = np.maximum(rng.normal(size=(1, 40, 56, ci)), 0).astype(np.float32)
    dz = rng.normal(size=(1, 20, 28, co)).astype(np.float32)
    a = run_wgrad(x, dz, k, s)
    b = run_wgrad(x, dz, k, s)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    # operand_dtype 0 is the fp32 kernel: within its own bound of the fp64 gradient of the UNROUNDED operands, where the
    # fp16 result is not, and bit-identical from launch to launch
    f = run_wgrad(x, dz, k, s, operand_dtype=0)
    f2 = run_wgrad(x, dz, k, s, operand_dtype=0)
    assert np.array_equal(f[0].view(np.uint32), f2[0].view(np.uint32))
    rw, rb = R.conv_grad_weights(x, dz, (k, k, ci, co), s)
    bound = wgrad_bound(x, dz, 20 * 28)
    assert float(np.abs(f[0] - rw).max()) <= bound < float(np.abs(a[0] - rw).max())


def test_f16_weight_gradient_refuses_what_it_cannot_take():
    rng = np.random.default_rng(4)

    def rc_of(ci, co, **kw):
        x = rng.normal(size=(1, 8, 8, ci)).astype(np.float32)
        dz = rng.normal(size=(1, 8, 8, co)).astype(np.float32)
        return wgrad_call(x, dz, 1, 1, **kw)[0]

    ARG = -1                                       # KFN_ERR_ARG
    assert rc_of(128, 4) == ARG                    # 'prediction': Cout below a 32-column tile
    assert rc_of(48, 64) == ARG                    # Cin % 32
    assert rc_of(64, 48) == ARG
    assert rc_of(64, 64, ldz_pad=3) == ARG         # dZ rows that cannot be read as float4
    assert rc_of(64, 64, z_off=1) == ARG           # a dz that is not 16-byte aligned
    assert rc_of(64, 64, operand_dtype=_lib.OPERAND_F16X3) == ARG
    assert rc_of(64, 64) == _lib.KFN_OK
    assert rc_of(128, 4, operand_dtype=0) == _lib.KFN_OK and rc_of(48, 64, operand_dtype=0, ldz_pad=3) == _lib.KFN_OK


# -- 2. the half packs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [_lib.PACK_FORWARD, _lib.PACK_INPUT_GRAD_S1, _lib.PACK_INPUT_GRAD_S2], ids=['forward', 's1', 's2'])
def test_half_packs_equal_the_host_packs_rounded_once(kind):
    import torch
    from kfnet_amd.graph import as_f16
    lib = _lib.load()
    rng = np.random.default_rng(12)
    for k, ci, co in ((3, 64, 256), (1, 256, 128), (3, 32, 48), (1, 128, 4)):
        w = (rng.normal(size=(k, k, ci, co)) * 10.0 ** rng.uniform(-6, 1, size=(k, k, ci, co))).astype(np.float32)
        nf = C.c_size_t()
        _lib.check(lib.kfn_pack_conv_weights_floats(k, k, ci, co, kind, C.byref(nf)), 'pack floats')
        G = 64
        f32 = torch.full((nf.value,), -7.0, device='cuda')
        f16 = torch.full((nf.value + G,), -7.0, dtype=torch.float16, device='cuda')
        wd = dev(w)
        _lib.check(lib.kfn_pack_conv_weights(wd.data_ptr(), k, k, ci, co, kind, f32.data_ptr(), stream()), 'kfn_pack_conv_weights')
        _lib.check(lib.kfn_pack_conv_weights_f16(wd.data_ptr(), k, k, ci, co, kind, f16.data_ptr(), stream()),
                   'kfn_pack_conv_weights_f16')
        sync()
        host32 = f32.cpu().numpy()                                       # the fp32 pack, pinned to the host packers elsewhere
        want = as_f16(lambda m: m)(host32)
        got = f16.cpu().numpy()
        assert np.all(got[-G:] == np.float16(-7.0)), 'wrote past the pack'
        assert np.array_equal(got[:-G].view(np.uint16), want.view(np.uint16)), (k, ci, co)
        if kind == _lib.PACK_FORWARD and ci % 16 == 0:
            from kfnet_amd.graph import pack_conv_kernel
            assert np.array_equal(got[:-G].view(np.uint16), as_f16(pack_conv_kernel)(w).reshape(-1).view(np.uint16)), (k, ci, co)


# -- 3. the loss-scale launches ------------------------------------------------------------------------------------------------
class DeviceScale(object):
    """A kfn_loss_scale_state in device memory."""

    def __init__(self, scale):
        import torch
        st = _lib.LossScaleState(beta1_power=1.0, beta2_power=1.0, scale=scale)
        self.buf = torch.from_numpy(np.frombuffer(bytes(st), dtype=np.uint8).copy()).cuda()
        self.ptr = self.buf.data_ptr()

    def read(self):
        return _lib.LossScaleState.from_buffer_copy(self.buf.cpu().numpy().tobytes())


def _guarded_step(ds, wd_, md, vd, g_scaled, lr, growth_interval, weight_decay=1e-4):
    lib = _lib.load()
    gd = dev(g_scaled)
    _lib.check(lib.kfn_loss_scale_unscale_check(gd.data_ptr(), g_scaled.size, ds.ptr, stream()), 'kfn_loss_scale_unscale_check')
    _lib.check(lib.kfn_adam_step_guarded(wd_.data_ptr(), md.data_ptr(), vd.data_ptr(), gd.data_ptr(), g_scaled.size, lr, R.BETA1,
                                         R.BETA2, R.EPSILON, weight_decay, growth_interval, ds.ptr, stream()),
               'kfn_adam_step_guarded')
    sync()
    return gd.cpu().numpy()


def _same_state(st, ref):
    assert st.scale == float(ref.scale) and st.good_steps == ref.good_steps and st.skipped == ref.skipped
    assert st.adam_t == ref.adam_t and st.overflow == 0
    assert st.beta1_power == float(ref.beta1_power) and st.beta2_power == float(ref.beta2_power)     # bit for bit


@pytest.mark.parametrize('poison', [None, np.inf, np.nan], ids=['finite', 'inf', 'nan'])
def test_loss_scale_launches_against_the_numpy_restatement(poison):
    """Six steps on 1000 elements with growth_interval = 3; with `poison`, step 3's gradient holds one such element."""
    lib = _lib.load()
    rng = np.random.default_rng(21)
    n, scale, interval = 1000, 2.0 ** 10, 3
    w = (rng.normal(size=n) * 0.1).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    wd_, md, vd = dev(w), dev(m), dev(v)
    ds, ref = DeviceScale(scale), HR.LossScale(scale, interval)
    worst = 0.0
    for step in range(1, 7):
        g = (rng.normal(size=n) * 10.0 ** rng.uniform(-6, -2, size=n)).astype(np.float32)
        # scale: the launch that multiplies dL/d(prediction); here it makes the scaled gradient from the plain one
        gd = dev(g)
        _lib.check(lib.kfn_loss_scale_apply(gd.data_ptr(), n, ds.ptr, stream()), 'kfn_loss_scale_apply')
        sync()
        gs = gd.cpu().numpy()
        assert np.array_equal(gs, g * ref.scale)
        if poison is not None and step == 3:
            gs[617] = poison
        lr = 1e-4 * 0.5 ** (step / 7.0)
        before = (w.copy(), m.copy(), v.copy(), ref.adam_t, float(ref.scale), ref.skipped)
        unscaled = _guarded_step(ds, wd_, md, vd, gs, lr, interval)
        w, m, v = ref.step(w, m, v, gs, lr, 1e-4)
        ok = np.isfinite(gs)
        assert np.array_equal(unscaled[ok], (gs * (np.float32(1.0) / np.float32(before[4])))[ok])
        _same_state(ds.read(), ref)
        got = [t.cpu().numpy() for t in (wd_, md, vd)]
        if poison is not None and step == 3:
            for a, b in zip(got, before[:3]):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))           # untouched, bit for bit
            assert ref.adam_t == before[3] and float(ref.scale) == before[4] / 2 and ref.skipped == before[5] + 1
        else:
            assert ref.adam_t == before[3] + 1                                       # t advances by one per applied step only
            for name, a, b in zip('wmv', got, (w, m, v)):
                u = float(R.ulp_distance(a, b).max())
                print('guarded adam step %d %s: %.2f ulp' % (step, name, u))
                worst = max(worst, u)
    assert worst <= 2.0
    print('guarded adam against numpy: worst %.2f ulp' % worst)
    st = ds.read()
    if poison is None:
        assert st.scale == scale * 4 and st.adam_t == 6 and st.skipped == 0 and st.good_steps == 0      # doubled after 3 and 6
    else:
        assert st.scale == scale and st.adam_t == 5 and st.skipped == 1 and st.good_steps == 0  # x2, /2 at step 3, x2 after 4-6


def test_loss_scale_floor_and_cap_on_the_device():
    n = 1000
    z = np.zeros(n, np.float32)
    wd_, md, vd = dev(z), dev(z), dev(z)
    ds = DeviceScale(2.0)
    bad = z.copy()
    bad[0] = np.inf
    for want in (1.0, 1.0):
        _guarded_step(ds, wd_, md, vd, bad, 1e-4, 2000)
        assert ds.read().scale == want
    assert ds.read().skipped == 2
    ds = DeviceScale(2.0 ** 23)
    for want in (2.0 ** 24, 2.0 ** 24):
        _guarded_step(ds, wd_, md, vd, z, 1e-4, 1)
        assert ds.read().scale == want
    assert ds.read().adam_t == 2


# -- 4. the whole step: SCoordNetTrainer(precision='fp16') ---------------------------------------------------------------------
# synthetic_sequence(seed) with initial_weights(seed): of seeds 1..40 the ones whose smallest fp64 |pre-activation| over every
# ReLU unit of the EMULATED network (train_f16_ref.smallest_preactivation, found on the CPU) is largest: 3.1e-8 and 1.5e-8.
STEP_SEEDS = {(64, 96): 37, (72, 104): 5}


def _batch(size, B=2, seed=1):
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    from kfnet_amd.train import synthetic_labels
    frames = synthetic_sequence(B, size[0], size[1], seed=seed)
    labels = synthetic_labels(B, (size[0] // 8, size[1] // 8))
    return frames, labels, synthetic_transform().astype(np.float32)


def _worst(g, ref):
    return max(float(np.abs(g[n] - ref[n]).max() / np.abs(ref[n]).max()) for n in ref)


@pytest.mark.parametrize('size', sorted(STEP_SEEDS), ids=['64x96', '72x104'])
def test_fp16_step_gradients_against_the_emulation(size):
    import torch
    from kfnet_amd.train import SCoordNetTrainer
    from kfnet_amd.weights import initial_weights
    seed = STEP_SEEDS[size]
    frames, labels, M = _batch(size, seed=seed)
    W = initial_weights(seed)
    s64, g64 = HR.loss_and_grads(frames, labels, W, M)                               # the reference: the emulation in fp64
    s32, g32 = HR.loss_and_grads(frames, labels, W, M, dtype=torch.float32)          # the yardstick: the same in torch fp32
    _, plain = R.loss_and_grads(frames, labels, W, M)
    e_32 = _worst(g32, g64)
    print('distance of the emulated gradient to the plain fp64 gradient: %.3e' % _worst(g64, plain))
    grads = {}
    for scale in (2 ** 15, 2 ** 10):
        tr = SCoordNetTrainer(W, image_size=size, batch=2, transform=M, base_lr=1e-4, weight_decay=1e-4, precision='fp16',
                              loss_scale=scale)
        stats = dict(tr.step(frames, labels))
        g = grads[scale] = tr.gradients()                                            # unscaled, whatever the scale
        e_dev = _worst(g, g64)
        print('loss scale 2^%d: loss device %.7g emulation fp32 %.7g fp64 %.7g; worst e: device %.3e, emulation in torch-CPU '
              'fp32 %.3e, bound %.3e' % (int(np.log2(scale)), stats['loss'], s32['loss'], s64['loss'], e_dev, e_32, 4 * e_32))
        assert e_dev <= 4.0 * e_32
        assert stats['loss_scale'] == scale and stats['skipped'] == 0
        st = tr.loss_scale_state()
        assert st['adam_t'] == 1 and st['good_steps'] == 1 and tr.global_step == 1
        # the update: the numpy restatement on the device's own gradients
        after, state = tr.weights(), tr.state()
        ref = HR.LossScale(scale)
        worst = 0.0
        for name in sorted(W):
            z = np.zeros_like(W[name])
            w1, m1, v1 = ref.adam(W[name], z, z, g[name], 1e-4, 1e-4)
            worst = max(worst, float(R.ulp_distance(after[name], w1).max()), float(R.ulp_distance(state['adam_m/' + name], m1).max()),
                        float(R.ulp_distance(state['adam_v/' + name], v1).max()))
        print('weights after the step against the numpy restatement: %.2f ulp' % worst)
        assert worst <= 2.0
    differing = sum(int((grads[2 ** 15][n] != grads[2 ** 10][n]).sum()) for n in g64)
    print('entries that differ between loss scales 2^15 and 2^10 (fp16 underflow of the scaled dZ): %d of %d' %
          (differing, sum(v.size for v in g64.values())))
    assert differing < sum(v.size for v in g64.values()) // 2


def test_fp16_a_loss_scale_that_overflows_comes_down_and_training_goes_on():
    """2^24 and 2^23 overflow fp16 on this batch (the emulation on the CPU says so), 2^22 does not."""
    from kfnet_amd.train import SCoordNetTrainer
    from kfnet_amd.weights import initial_weights
    frames, labels, M = _batch(SIZE)
    W = initial_weights(2)
    tr = SCoordNetTrainer(W, image_size=SIZE, batch=2, transform=M, base_lr=1e-4, weight_decay=1e-4, precision='fp16',
                          loss_scale=2 ** 24)
    stats = [tr.step(frames, labels) for _ in range(11)]
    first = dict(stats[0])
    after = tr.weights()
    assert first['skipped'] == 1 and first['loss_scale'] == 2.0 ** 23
    assert all(np.array_equal(after[k], after[k]) and np.all(np.isfinite(after[k])) for k in after)
    st = tr.loss_scale_state()
    losses = [s['loss'] for s in stats]
    print('skipped %d, scale 2^%d, applied %d of %d; losses %s' % (st['skipped'], int(np.log2(st['scale'])), st['adam_t'],
                                                                   tr.global_step, ' '.join('%.4f' % x for x in losses)))
    assert st['skipped'] >= 1 and st['scale'] < 2.0 ** 24 and st['adam_t'] == 11 - st['skipped'] and tr.global_step == 11
    assert losses[1] == losses[0]                             # the skipped step left the weights alone
    assert losses[-1] < losses[0]


def test_fp16_twenty_steps_on_one_batch_lower_the_loss_like_the_emulated_run():
    """The criterion of test_gpu_train's fp32 test; the emulated run is evaluated in torch fp32, which halves its time."""
    import torch
    from kfnet_amd.train import SCoordNetTrainer, learning_rate
    from kfnet_amd.weights import initial_weights
    frames, labels, M = _batch(SIZE)
    W = initial_weights(2)
    tr = SCoordNetTrainer(W, image_size=SIZE, batch=2, transform=M, base_lr=1e-4, weight_decay=1e-4, precision='fp16')
    dev_losses = [tr.step(frames, labels) for _ in range(21)]          # queued; entry i = the loss after i updates
    dev_losses = [s['loss'] for s in dev_losses]
    ref = {k: v.copy() for k, v in W.items()}
    m = {k: np.zeros_like(v) for k, v in W.items()}
    v_ = {k: np.zeros_like(v) for k, v in W.items()}
    ls = HR.LossScale()
    ref_losses = []
    for t in range(1, 22):
        s, g = HR.loss_and_grads(frames, labels, ref, M, dtype=torch.float32, scale=float(ls.scale))
        ref_losses.append(s['loss'])
        lr = learning_rate(1e-4, 0.5, 80000, t - 1)
        assert all(np.all(np.isfinite(x)) for x in g.values())
        for k in ref:
            ref[k], m[k], v_[k] = ls.adam(ref[k], m[k], v_[k], g[k].astype(np.float32), lr, 1e-4)
        ls.update(False)
    for i in (0, 1, 5, 10, 20):
        print('after %2d updates: device loss %.6f, emulated run %.6f' % (i, dev_losses[i], ref_losses[i]))
    assert tr.loss_scale_state()['skipped'] == 0
    assert ref_losses[20] < ref_losses[0]
    assert abs(dev_losses[0] - ref_losses[0]) <= 1e-4 * abs(ref_losses[0])
    assert dev_losses[20] < 0.5 * (dev_losses[0] + ref_losses[20])


def _run_steps(tr, frames, labels, first, count):
    from kfnet_amd.train import batch_indices
    for s in range(first, first + count):
        idx = batch_indices(s, 2, frames.shape[0])
        tr.step(frames[idx], labels[idx])


def test_fp16_runs_are_bit_identical_and_resume_from_snapshot_files(tmp_path):
    """Four steps from 2^24 with growth_interval = 2, so that the run holds skipped steps and a scale that moves."""
    from kfnet_amd.train import SCoordNetTrainer, restore
    from kfnet_amd.weights import initial_weights
    frames, labels, M = _batch(SIZE, B=4)
    W = initial_weights(2)
    kw = dict(image_size=SIZE, batch=2, transform=M, base_lr=1e-3, stepvalue=3, precision='fp16', loss_scale=2 ** 24, growth_interval=2)
    runs = []
    for _ in range(2):
        tr = SCoordNetTrainer(W, **kw)
        _run_steps(tr, frames, labels, 0, 4)
        runs.append((tr.weights(), tr.state()))
    for k in W:
        assert np.array_equal(runs[0][0][k].view(np.uint32), runs[1][0][k].view(np.uint32)), k
        assert not np.array_equal(runs[0][0][k], W[k]), k
    full = runs[0][1]
    print('after four steps: scale %g, skipped %d, adam_t %d' % (full['loss_scale'], full['loss_scale_skipped'], full['adam_t']))
    assert int(full['loss_scale_skipped']) >= 1 and int(full['adam_t']) == 4 - int(full['loss_scale_skipped'])
    tr = SCoordNetTrainer(W, **kw)
    _run_steps(tr, frames, labels, 0, 2)
    wp, sp = tr.save(str(tmp_path))
    assert os.path.basename(wp) == 'kfnet_weights-2.npz' and os.path.basename(sp) == 'kfnet_train_state-2.npz'
    del tr
    W2, state, step = restore(str(tmp_path), verbose=False)
    assert step == 2 and state is not None and 'loss_scale' in state
    tr = SCoordNetTrainer(W2, **kw)
    tr.load_state(state)
    assert tr.global_step == 2
    _run_steps(tr, frames, labels, 2, 2)
    resumed, rstate = tr.weights(), tr.state()
    for k in W:
        assert np.array_equal(resumed[k].view(np.uint32), runs[0][0][k].view(np.uint32)), k
    assert sorted(rstate) == sorted(full)
    for k in full:
        assert np.asarray(rstate[k]).tobytes() == np.asarray(full[k]).tobytes(), k
    # a state file from before the loss-scale record (or from an fp32 run) loads with the defaults
    old = {k: v for k, v in state.items() if not k.startswith('loss_scale') and not k.startswith('adam_beta')}
    tr = SCoordNetTrainer(W2, **kw)
    tr.load_state(old)
    st = tr.loss_scale_state()
    t = int(state['adam_t'])
    assert st['scale'] == 2.0 ** 24 and st['skipped'] == 0 and st['good_steps'] == 0 and st['adam_t'] == t
    assert abs(st['beta1_power'] - R.BETA1 ** t) <= 1e-15 and abs(st['beta2_power'] - R.BETA2 ** t) <= 1e-15
    # ... and an fp32 trainer reads an fp16 run's files
    tr = SCoordNetTrainer(W2, **dict(kw, precision='fp32'))
    tr.load_state(state)
    assert tr.adam_t == t and 'loss_scale' not in tr.state()


# -- 5. the command line ---------------------------------------------------------------------------------------------------------
def _cli(module, args, timeout=900):
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT'):
        env.pop(k, None)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    r = subprocess.run([sys.executable, '-m', module] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_fp16_train_command_line_then_eval_reads_its_snapshot(tmp_path):
    import re
    model, plain, out = tmp_path / 'm', tmp_path / 'p', tmp_path / 'o'
    out.mkdir()
    small = ['--height', '64', '--width', '96', '--batch', '2', '--scene', 'fire']
    run = ['--synthetic', '8', '--max_steps', '20', '--snapshot', '20', '--display', '5'] + small
    log = _cli('kfnet_amd.SCoordNet.train', ['--model_folder', str(model), '--fp16'] + run)
    assert sorted(os.listdir(str(model))) == ['kfnet_train_state-20.npz', 'kfnet_weights-20.npz']
    lines = [l for l in log.splitlines() if 'step ' in l and 'loss=' in l]
    assert len(lines) == 4 and all(re.search(r'sec/step\), loss_scale=32768, skipped=0$', l) for l in lines), log
    with np.load(str(model / 'kfnet_train_state-20.npz')) as z:
        assert float(z['loss_scale']) == 32768.0 and int(z['adam_t']) == 20 and int(z['global_step']) == 20
    _cli('kfnet_amd.SCoordNet.eval', ['--model_folder', str(model), '--synthetic', '4', '--output_folder', str(out)] + small)
    assert all(np.all(np.isfinite(np.load(str(out / ('coord_%d.npy' % i))))) for i in range(4))
    # without --fp16 the lines are the ones the program always printed, and the state file holds no loss-scale record
    log = _cli('kfnet_amd.SCoordNet.train', ['--model_folder', str(plain)] + run)
    lines = [l for l in log.splitlines() if 'step ' in l and 'loss=' in l]
    assert len(lines) == 4 and all(l.endswith('sec/step)') and 'loss_scale' not in l for l in lines), log
    with np.load(str(plain / 'kfnet_train_state-20.npz')) as z:
        assert 'loss_scale' not in z.files
