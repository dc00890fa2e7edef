"""-m gpu cross-test of the Winograd entry points' descriptor fields (csrc/kfn_wino2.hip, kfn_wino3.hip, kfn_wino4.hip,
kfn_wino_s2.hip, kfn_wino_s2c.hip): the all-pairs case table of tests/wino_modes.py -- kernel x image x Cin x Cout x workgroup
order x ReLU x bias x input window x output window x layout x split-K -- against the fp64 oracle.  gpu_util.run_winograd adds guard
rows behind the output and sentinels around the channel window (and behind the split-K planes) to every launch.

Per case:
  bound       conv_tol.assert_close with the kind of the kernel's family (f23 / f43 / f22s2 / f42s2; nothing fitted here).  The two
              fp16-operand kernels get their fp32 siblings' bound: on the gridded inputs of wino_modes.make_inputs every product is
              exact, the reference (wino_modes.reference) rounds V to fp16 once as the kernel must, and what is left is fp32
              accumulation and the output transform
  order       order != AUTO: a second launch with AUTO on the same buffers is bit-identical (the order permutes workgroups)
  store path  yview ld / off with Cout % 4 == 0: the launch with yview pad (16-byte stores) is bit-identical
  layout      channel-blocked tensors: bit-identical to the NHWC launch
  split-K     k_split = 1 is bit-identical to the unsplit eight-wave launch; k_split > 1: two runs are bit-identical
Every comparison made is counted in wino_modes_report.txt beside conv_tol's report (`case kernel path comparisons`)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import wino_modes as WM
from tests import conv_tol
from tests.conv_tol import assert_close

pytestmark = pytest.mark.gpu

CHUNKS = 16
_REPORT = os.path.join(os.path.dirname(conv_tol._REPORT), 'wino_modes_report.txt')


def _note(line):
    print(line)
    try:
        os.makedirs(os.path.dirname(_REPORT), exist_ok=True)
        with open(_REPORT, 'a') as f:
            f.write(line + '\n')
    except OSError:
        pass


def _run(c, x, w, b, relaunch=None, **change):
    from tests.gpu_util import run_winograd
    c = c._replace(**change)
    _, kind, _, _, split, _ = WM.KERNELS[c.kernel]
    return run_winograd(kind, x, w, b, x_fill=1e6, k_split=c.ksplit if split else None, relaunch=relaunch, **WM.launch_args(c))


def _one(i, c):
    """Runs case `c` and everything it is compared with; returns the list of what went wrong."""
    x, w, b = WM.make_inputs(i, c)
    label = 'modes ' + WM.case_id(i, c)
    bad, made = [], []
    relaunch = []
    if c.order != 'auto':
        relaunch.append(('order', dict(wino_order=0)))
    if c.ksplit > 1:
        relaunch.append(('split-K rerun', {}))
    try:
        ys = _run(c, x, w, b, relaunch=[r[1] for r in relaunch])
        for (what, _), other in zip(relaunch, ys[1:]):
            made.append(what)
            if not np.array_equal(ys[0], other):
                bad.append('%s: %s differs in %d elements' % (label, what, int((ys[0] != other).sum())))
        y = ys[0]
        others = []
        if c.yview in ('ld', 'off') and c.cout % 4 == 0:
            others.append(('store path', dict(yview='pad')))
        if c.layout != 'nhwc':
            others.append(('layout', dict(layout='nhwc')))
        if c.ksplit == 1:
            others.append(('split-K 1', dict(kernel=c.kernel[:-1], ksplit=0)))
        for what, change in others:
            made.append(what)
            other = _run(c, x, w, b, **change)
            if not np.array_equal(y, other):
                bad.append('%s: %s differs in %d elements' % (label, what, int((y != other).sum())))
    except AssertionError as e:          # run_winograd's guard rows / channel-window / workspace sentinels
        return ['%s: %s' % (label, e)]
    _note('%s %s %s %s' % (WM.case_id(i, c), c.kernel, WM.store_path(c), ','.join(made) or '-'))
    if not np.all(np.isfinite(y)):
        return bad + ['%s: non-finite output' % label]
    try:
        assert_close(y, WM.reference(c, x, w, b), x, w, WM.TOL_KIND[WM.FAMILY[c.kernel]], label)
    except AssertionError as e:
        bad.append(str(e))
    return bad


@pytest.mark.parametrize('chunk', range(CHUNKS))
def test_wino_modes_vs_oracle(chunk):
    bad = []
    for j, (i, c) in enumerate(WM.cases()):
        if j % CHUNKS == chunk:
            bad += _one(i, c)
    assert not bad, '\n'.join(bad)


def _cu_count():
    import torch
    from kfnet_amd import _lib
    cu = C.c_int(0)
    _lib.check(_lib.load().kfn_device_info(torch.cuda.current_device(), C.byref(cu), None, None, 0), 'kfn_device_info')
    return cu.value


@pytest.mark.parametrize('j', range(6))
def test_wino_s2c_persistent_modes(j):
    """wino_s2c_pkernel (launches of at least two workgroups per CU): its block walk under every order level, on the smallest
    batch of 40x48 images that the launcher's rule sends there and on three more (a ragged last round)."""
    cu = _cu_count()
    i, c = WM.persistent_cases(cu)[j]
    assert WM.s2c_persistent(c.img[0], c.img[1], c.img[2], c.cin, c.cout, cu), (cu, c)
    bad = _one(i, c)
    assert not bad, '\n'.join(bad)


def test_wino_mode_refusals():
    """What the kernels without a dword epilogue cannot store, and the input alignments no kernel gathers from, are refused
    (a negative code and a message), not computed some other way: nothing is launched, the output keeps its sentinel."""
    import torch
    from kfnet_amd import _lib
    from tests.gpu_util import stream
    lib = _lib.load()
    x = torch.zeros(1 << 18, device='cuda')
    u = torch.zeros(1 << 18, device='cuda')
    ws = torch.zeros(1 << 20, device='cuda')
    y = torch.full((1 << 18,), -5.0, device='cuda')
    s1 = dict(N=1, H=32, W=32, Cin=32, ldx=32, Cout=64, cout_pad=64, ldy=64, kh=3, kw=3, stride=1)
    s2 = dict(s1, stride=2)
    entry = {
        'f43a': (lambda d, xp, yp: lib.kfn_conv2d_winograd_f43(C.byref(d), xp, u.data_ptr(), None, yp, stream()), dict(s1, wino_form=2)),
        'f43b': (lambda d, xp, yp: lib.kfn_conv2d_winograd_f43(C.byref(d), xp, u.data_ptr(), None, yp, stream()), dict(s1, wino_form=3)),
        's2c': (lambda d, xp, yp: lib.kfn_conv2d_winograd_s2(C.byref(d), xp, u.data_ptr(), None, yp, stream()), dict(s2, wino_form=5)),
        'f43bk': (lambda d, xp, yp: lib.kfn_conv2d_winograd_f43_splitk(C.byref(d), xp, u.data_ptr(), None, yp, ws.data_ptr(), 2, stream()),
                  dict(s1, wino_form=3)),
        's2bk': (lambda d, xp, yp: lib.kfn_conv2d_winograd_s2_splitk(C.byref(d), xp, u.data_ptr(), None, yp, ws.data_ptr(), 2, stream()),
                 dict(s2, wino_form=4)),
        'fused': (lambda d, xp, yp: lib.kfn_conv2d_winograd_fused(C.byref(d), xp, u.data_ptr(), None, yp, stream()), s1),
        's2a': (lambda d, xp, yp: lib.kfn_conv2d_winograd_s2(C.byref(d), xp, u.data_ptr(), None, yp, stream()), s2),
        's2b': (lambda d, xp, yp: lib.kfn_conv2d_winograd_s2(C.byref(d), xp, u.data_ptr(), None, yp, stream()), dict(s2, wino_form=4)),
    }
    seen = []

    def refused(name, x_off=0, y_off=0, **change):
        fn, base = entry[name]
        rc = fn(_lib.ConvDesc(**dict(base, **change)), x.data_ptr() + x_off, y.data_ptr() + y_off)
        err = lib.kfn_last_error() or b''
        seen.append((name, x_off, y_off, change, rc, err[:60]))
        return rc < 0 and len(err) > 0
    for name in ('f43a', 'f43b', 's2c', 'f43bk', 's2bk'):
        assert entry[name][0](_lib.ConvDesc(**entry[name][1]), x.data_ptr(), y.data_ptr()) == 0, name      # the base is accepted
        y.fill_(-5.0)
        assert refused(name, y_off=4), name                     # y one float past a 16-byte boundary
        if name != 's2c':                                       # (test_winograd_s2_f42_refuses_what_it_cannot_take has these two)
            assert refused(name, Cout=62, ldy=64), name         # Cout % 4 != 0
            assert refused(name, ldy=66), name                  # ldy % 4 != 0
    for name in ('fused', 's2a', 's2b', 's2c', 's2bk'):
        assert refused(name, x_off=8), name                     # x 8-byte aligned only
    for name in ('f43a', 'f43b', 'f43bk'):
        assert entry[name][0](_lib.ConvDesc(**entry[name][1]), x.data_ptr() + 8, y.data_ptr()) == 0, name   # 8 bytes: taken
        y.fill_(-5.0)
        assert refused(name, x_off=4), name                     # 4 bytes: not
    torch.cuda.synchronize()
    print(seen)
    assert bool((y == -5.0).all()), 'a refused call wrote to its output'
