"""-m gpu cross-test of kfn_conv2d_nhwc's descriptor fields (csrc/kfn_conv.hip, conv_mfma_kernel): the all-pairs case
table of tests/conv_modes.py -- mode x image set x Cin x Cout x tile config x operands x ReLU x bias x channel windows x
head epilogue x fp16 input -- against the fp64 oracle.  gpu_util.run_conv adds guard rows behind the output and sentinels
around the channel window to every case.

Tolerances (none fitted to the kernel; b = conv_tol.conv_err_bound of the operands the products are exact for):
  no epilogue   |dy| <= b
  L2NORM        |dy_i| <= (1 + sqrt(32)) b / n + 64 * 2^-24 with n = ||v||_2 of the reference: |dv_i| / n plus
                |y_i| ||dv||_2 / n (|y_i| <= 1), plus the epilogue's own < 40 fp32 roundings (32 squares and adds, the
                square root, the quotient; 64 is the next power of two).  n >= 1 is checked on the host
                (test_conv_modes_host.py); an all-zero pixel comes back exactly 0.0 (the 1e-12 floor), not NaN
  EXP_CH3 ch 3, EXP_1E2
                |dy| <= exp(ref) (e^b - 1) s + 2 ulp32(y), s = 1 | 1e-2: the argument's error through exp, plus OCML's 1-ulp
                expf, the product's half ulp and the half ulp of 1e-2f itself
Every case logs `kind label err bound ratio` through conv_tol.record (kinds direct / f16x3 / l2norm / exp_ch3 / exp_1e2;
the label names operands and input type)."""
import ctypes as C

import numpy as np
import pytest

from tests import conv_modes as CM
from tests.conv_tol import conv_err_bound, record

pytestmark = pytest.mark.gpu

CHUNKS = 12
L2_ROUNDINGS = 64 * 2.0 ** -24


def _run(c, x, w, b, config=None):
    from tests.gpu_util import run_conv
    k, s, tr = CM.MODE[c.mode]
    ldx, x_off, ldy, y_off = CM.view_strides(c.cin, c.cout, c.view)
    return run_conv(x, w, b, s, bool(c.relu), transposed=tr, epilogue=c.epi, config=c.config if config is None else config,
                    ldx=ldx, ldy=ldy, x_off=x_off, y_off=y_off, f16=c.operands == 'f16', x3=c.operands == 'f16x3',
                    x16=bool(c.x16))


def _check(i, c, x, w, b, y):
    """None if `y` (device result of case `c`) is within its allowance, else a message.  Logs the worst element."""
    k, s, tr = CM.MODE[c.mode]
    xr, wr = CM.rounded_operands(c, x, w)
    kind = 'f16x3' if c.operands == 'f16x3' else 'direct'
    bnd = conv_err_bound(xr, wr, kind, tr)
    v = CM.reference(c, x, w, b)
    assert y.shape == v.shape, (y.shape, v.shape)
    y = y.astype(np.float64)
    label = 'modes ' + CM.case_id(i, c)
    if not np.all(np.isfinite(y)):
        return '%s: non-finite output' % label
    msg = None
    if c.epi == CM.EPI_NONE:
        diff, allow, name = np.abs(y - v), np.full(v.shape, bnd), kind
    elif c.epi == CM.EPI_L2NORM:
        zm = CM.zero_mask(c, x)
        n = np.sqrt((v * v).sum(axis=-1, keepdims=True))
        assert np.all(n[zm] == 0.0) and np.all(n[~zm] >= 1.0), 'case %d: the reference violates the premise of the bound' % i
        if not np.all(y[zm] == 0.0):
            msg = '%s: all-zero pixel came back as %r' % (label, y[zm].ravel()[:4])
        n = np.where(zm[..., None], 1.0, n)
        diff = np.abs(y - v / n)
        allow = (1.0 + np.sqrt(32.0)) * bnd / n + L2_ROUNDINGS + 0.0 * diff
        diff[zm] = 0.0
        name = 'l2norm'
    else:
        sc = 1.0 if c.epi == CM.EPI_EXP_CH3 else 1e-2
        ref, allow = v.copy(), np.full(v.shape, bnd)
        ch = slice(3, 4) if c.epi == CM.EPI_EXP_CH3 else slice(0, 1)
        ulp = np.spacing(np.abs(y[..., ch]).astype(np.float32)).astype(np.float64)
        ref[..., ch] = np.exp(v[..., ch]) * sc
        allow[..., ch] = np.exp(v[..., ch]) * np.expm1(bnd) * sc + 2.0 * ulp
        diff = np.abs(y - ref)
        name = CM.EPI_NAME[c.epi]
        over = (diff[..., ch] - np.exp(v[..., ch]) * np.expm1(bnd) * sc) / ulp
        j = np.unravel_index(np.argmax(over), over.shape)
        print('%s: worst exp element %.2f ulp beyond the argument term, argument %.6f' % (label, over[j], v[..., ch][j]))
    ratio = diff / allow
    j = np.unravel_index(np.argmax(ratio), ratio.shape)
    record(name, label, float(diff[j]), float(allow[j]))
    if ratio[j] > 1.0:
        msg = '%s: err %.3e, allowed %.3e at %s (device %.9g)' % (label, diff[j], allow[j], j, y[j])
    return msg


@pytest.mark.parametrize('chunk', range(CHUNKS))
def test_conv_modes_vs_oracle(chunk):
    bad = []
    for i, c in enumerate(CM.table()):
        if i % CHUNKS != chunk:
            continue
        x, w, b = CM.make_inputs(i, c)
        try:
            y = _run(c, x, w, b)
        except AssertionError as e:          # run_conv's guard rows / channel-window sentinels
            bad.append('%s: %s' % (CM.case_id(i, c), e))
            continue
        msg = _check(i, c, x, w, b, y)
        if msg:
            bad.append(msg)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('i,c,config', CM.FORCED, ids=[CM.EPI_NAME[c.epi] for _, c, _ in CM.FORCED])
def test_epilogue_forces_other_configs_to_128x32(i, c, config):
    """pick_config(): an explicit config other than 128x32 / 256x32 beside a head epilogue runs the 128x32 tile -- the result
    equals the config-4 one bit for bit (and that one is held to the epilogue's allowance)."""
    assert c.config == 4 and CM.valid(c._asdict()) and not CM.valid(c._replace(config=config)._asdict())
    x, w, b = CM.make_inputs(i, c)
    y4 = _run(c, x, w, b)
    msg = _check(i, c, x, w, b, y4)
    assert not msg, msg
    assert np.array_equal(_run(c, x, w, b, config=config), y4)


def test_conv_mode_refusals():
    """What conv_mfma_kernel would not do is refused (KFN_ERR_ARG = -1, the message names the field), not computed
    differently: a head epilogue on a transposed convolution (HEAD_EPI is forward only), an epilogue value the kernel's
    switch does not know, f16x3 operands on a transposed convolution."""
    import torch
    from kfnet_amd import _lib
    from tests.gpu_util import stream
    lib = _lib.load()
    x = torch.zeros(4096, device='cuda')
    w = torch.zeros(65536, device='cuda')
    bias = torch.zeros(32, device='cuda')
    y = torch.zeros(8192, device='cuda')
    base = dict(N=1, H=4, W=4, Cin=32, ldx=32, Cout=32, cout_pad=32, ldy=32, kh=3, kw=3, stride=1)

    def call(**kw):
        d = _lib.ConvDesc(**dict(base, **kw))
        rc = lib.kfn_conv2d_nhwc(C.byref(d), x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), stream())
        return rc, lib.kfn_last_error() or b''
    accepted = [call(), call(epilogue=_lib.EPI_L2NORM), call(stride=2, transposed=1)]
    on_transposed = [call(stride=2, transposed=1, epilogue=e) for e in (_lib.EPI_L2NORM, _lib.EPI_EXP_CH3, _lib.EPI_EXP_1E2)]
    unknown = [call(epilogue=e) for e in (4, -1, 255)]
    x3_transposed = call(stride=2, transposed=1, operand_dtype=_lib.OPERAND_F16X3)
    torch.cuda.synchronize()
    print('accepted', accepted, 'epilogue on transposed', on_transposed, 'unknown epilogue', unknown, 'f16x3 transposed', x3_transposed)
    assert all(rc == 0 for rc, _ in accepted)
    assert all(rc == -1 and b'epilogue' in err and b'transposed' in err for rc, err in on_transposed), on_transposed
    assert all(rc == -1 and b'epilogue' in err for rc, err in unknown), unknown
    assert x3_transposed[0] == -1 and b'operand_dtype' in x3_transposed[1], x3_transposed
