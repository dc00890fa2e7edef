"""Host checks of the training side's launch-branch table (tests/train_branches.py): through kfn_conv2d_grad_weights_plan -- the
function the launcher decides by -- that every case lands on the tiles, runs and last-run length the table states and that the
table reaches every cell of {TN 1, TN 2} x {one run, several runs} x {last stage full, ragged} for fp32 and for fp16 operands;
the workspace size; the export's refusals; KFN_PACK_INPUT_GRAD_S1's refusal of even kernels and why; and the test's own
references against the fp64 ones."""
import ctypes as C

import numpy as np
import pytest

import train_branches as TB
import train_ref as R
from kfnet_amd import _lib
from oracle import kfnet_oracle as O

ARG = -1      # KFN_ERR_ARG


def _desc(c, dtype, **kw):
    f = dict(N=c.N, H=c.H, W=c.W, Cin=c.cin, ldx=c.cin + c.ldx_pad, Cout=c.cout, cout_pad=-(-c.cout // 32) * 32, ldy=c.ldz, kh=c.k,
             kw=c.k, stride=c.stride, operand_dtype=dtype)
    f.update(kw)
    return _lib.ConvDesc(**f)


def _plan(lib, d):
    tn, tm, tnn, splits, chunk = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_long(-1)
    rc = lib.kfn_conv2d_grad_weights_plan(C.byref(d), C.byref(tn), C.byref(tm), C.byref(tnn), C.byref(splits), C.byref(chunk))
    return rc, (tn.value, tm.value, tnn.value, splits.value, chunk.value)


def _cell(c, dtype):
    p = c.plans[dtype]
    return p.tn, p.splits > 1, p.last % TB.STAGE[dtype] != 0


@pytest.mark.parametrize('case', TB.WGRAD_CASES + (TB.REDUCE_CASE,), ids=TB.wgrad_id)
def test_every_case_lands_on_the_plan_the_table_states(case):
    lib = _lib.load()
    P, Ktot = TB.out_pixels(case), case.k * case.k * case.cin
    for dtype, want in sorted(case.plans.items()):
        d = _desc(case, dtype)
        rc, got = _plan(lib, d)
        assert rc == 0, lib.kfn_last_error()
        assert got == tuple(want[:5]), (case.name, dtype, got)
        tn, tiles_m, tiles_n, splits, chunk = got
        assert tn == (1 if case.cout <= 64 else 2)
        assert tiles_m == -(-(Ktot + 1) // TB.WG_BM) and tiles_n == -(-case.cout // (64 * tn))
        assert chunk % TB.STAGE[dtype] == 0 and (splits - 1) * chunk < P <= splits * chunk
        assert P - (splits - 1) * chunk == want.last
        nb = C.c_size_t(7)
        _lib.check(lib.kfn_conv2d_grad_weights_workspace_bytes(C.byref(d), C.byref(nb)), 'workspace bytes')
        assert nb.value == splits * (Ktot + 1) * case.cout * 4
    if TB.F16 in case.plans:
        assert case.cin % 32 == 0 and case.cout % 32 == 0 and case.ldz % 4 == 0
    assert case.ldz >= case.cout and (case.cin + case.ldx_pad) % 4 == 0


def test_wgrad_table_reaches_every_cell_and_keeps_its_cases():
    """Asserted on the whole table, so that a case taken out of it fails here."""
    cases = {c.name: c for c in TB.WGRAD_CASES}
    assert sorted(cases, key=lambda s: int(s[1:])) == ['W%d' % i for i in range(1, 14)]
    shape = lambda c: (c.N, c.H, c.W, c.cin, c.cout, c.k, c.stride, c.ldz, sorted(c.plans))
    assert shape(cases['W1']) == (3, 20, 27, 48, 70, 3, 1, 72, [0]) and shape(cases['W2']) == (2, 23, 29, 16, 130, 3, 2, 131, [0])
    assert shape(cases['W3']) == (5, 11, 21, 80, 6, 1, 2, 8, [0]) and shape(cases['W4'])[:7] + shape(cases['W4'])[8:] == (1, 33, 47, 32, 192, 3, 1, [0, 1])
    assert shape(cases['W5'])[:7] == (3, 19, 30, 16, 100, 1, 1) and shape(cases['W6'])[:7] + shape(cases['W6'])[8:] == (1, 32, 48, 96, 96, 3, 1, [0, 1])
    assert shape(cases['W7'])[:7] + shape(cases['W7'])[8:] == (4, 17, 19, 128, 32, 3, 1, [0, 1])
    assert shape(cases['W8'])[:7] + shape(cases['W8'])[8:] == (2, 24, 40, 32, 160, 3, 2, [0, 1])
    assert shape(cases['W9'])[:7] == (1, 1, 1, 16, 1, 3, 1) and shape(cases['W10'])[:7] == (2, 37, 1, 64, 64, 3, 2)
    for dtype in (TB.F32, TB.F16):
        cells = {_cell(c, dtype) for c in TB.WGRAD_CASES if dtype in c.plans}
        assert cells == {(tn, several, ragged) for tn in (1, 2) for several in (False, True) for ragged in (False, True)}, (dtype, cells)
    # several runs AND a ragged last stage, which no fp32 case of the op-level tests has
    assert {c.name for c in TB.WGRAD_CASES if _cell(c, TB.F32)[1:] == (True, True)} >= {'W1', 'W4', 'W5', 'W7'}
    # channel edges: a ragged tile (Cout % (64 tn) != 0 in the only or the last tile), a second tile at most half full
    ragged = [c for c in TB.WGRAD_CASES if c.cout % (64 * c.plans[TB.F32].tn)]
    half_empty = [c for c in TB.WGRAD_CASES if c.plans[TB.F32].tiles_n == 2 and c.cout - 128 <= 64]
    assert {c.name for c in ragged} >= {'W1', 'W2', 'W3', 'W5', 'W6', 'W7', 'W8'} and {c.name for c in half_empty} >= {'W2', 'W4', 'W8'}
    ktots = [c.k * c.k * c.cin for c in TB.WGRAD_CASES]
    assert any(k % 128 == 0 for k in ktots) and any(k % 128 for k in ktots)
    assert any(128 % c.cin for c in TB.WGRAD_CASES if c.k == 3), 'a float4 column of a k tile whose tap differs from its neighbour tile'
    # the dZ loader's three paths: all float4, float4 with a scalar last quad, all scalar
    paths = {(c.ldz % 4 == 0, c.cout % 4 == 0) for c in TB.WGRAD_CASES}
    assert paths >= {(True, True), (True, False), (False, False)}
    # fp16 operands off the sizes the op-level tests use
    f16 = [c for c in TB.WGRAD_CASES if TB.F16 in c.plans]
    assert {c.cin for c in f16} >= {32, 96} and {c.cout for c in f16} >= {32, 96, 160, 192}
    assert any(c.k == 1 and c.stride == 2 for c in TB.WGRAD_CASES) and any(c.W == 1 for c in TB.WGRAD_CASES)
    assert any(TB.out_pixels(c) == 1 for c in TB.WGRAD_CASES)
    assert set(TB.WGRAD_NO_BIAS) >= {'W1', 'W3', 'W9'} and set(TB.WGRAD_RELAUNCH) == {'W1', 'W4'}
    assert all(n in cases for n in TB.WGRAD_NO_BIAS + TB.WGRAD_RELAUNCH)
    # every partial sum of the exact check is an integer below 2^24
    assert max(TB.out_pixels(c) for c in TB.WGRAD_CASES) == 1710 and 6 * 1710 < 2 ** 24
    # the grid-stride cases are past one pass
    r = TB.REDUCE_CASE
    assert (r.k * r.k * r.cin + 1) * r.cout > TB.GRID_8192 and TB.out_pixels(r) == 40
    assert 32 * 9 * 512 * 16 > TB.GRID_8192 and 512 * 9 * 512 > TB.GRID_8192


def test_first_conv_table_holds_its_seams():
    assert TB.FIRST_IMAGES == ((3, 27, 31), (1, 1, 2049), (2, 9, 13)) and TB.FIRST_WIDTHS == (16, 32, 48, 64)
    n, h, w = TB.FIRST_IMAGES[0]
    P = n * h * w
    assert P == 2511 and -(-P // TB.FC_CHUNK) == 2
    assert h * w == 837 and 2 * h * w == 1674 < TB.FC_CHUNK < P               # image seams inside chunk 0, the chunk seam inside image 2
    assert (P - TB.FC_CHUNK) % TB.FC_SUB == 15                                 # the last block of the second chunk
    assert TB.first_pixels(TB.FIRST_IMAGES[0]) == [0, 30, 806, 836, 837, 1674, 1704, 2047, 2048, 2480, 2510]
    assert TB.first_pixels(TB.FIRST_IMAGES[1]) == [0, 836, 837, 2047, 2048]     # a second chunk of one pixel
    assert TB.first_pixels(TB.FIRST_IMAGES[2]) == [0, 12, 104, 116, 117, 129, 221, 233]
    # threads hold ceil(28 C1 / 256) sums at most: fewer than 7 below C1 = 64, and some threads none
    assert [(-(-28 * c // 256), 28 * c % 256 != 0) for c in TB.FIRST_WIDTHS] == [(2, True), (4, True), (6, True), (7, False)]


def test_plan_export_refuses_what_the_launcher_refuses_and_touches_no_device():
    lib = _lib.load()
    base = TB.WGRAD_CASES[0]
    buf = np.zeros(64, np.float32).ctypes.data
    nb = C.c_size_t()
    assert _plan(lib, _desc(base, TB.F32))[0] == 0
    bad_descs = (dict(Cin=8, ldx=8), dict(Cin=40, ldx=40), dict(kh=5, kw=5), dict(kh=2, kw=2), dict(kh=1, kw=3), dict(stride=3),
                 dict(transposed=1, stride=2), dict(ldy=69), dict(ldx=47), dict(ldx=50), dict(N=0), dict(Cout=0), dict(operand_dtype=1),
                 dict(operand_dtype=2), dict(x_dtype=1), dict(y_dtype=1), dict(struct_size=8))
    for bad in bad_descs:
        d = _desc(base, TB.F32, **bad)
        if 'struct_size' in bad:
            d.struct_size = bad['struct_size']
        rc, got = _plan(lib, d)
        assert rc == ARG and got == (-1, -1, -1, -1, -1), bad
        assert b'kfn_conv2d_grad_weights_plan' in lib.kfn_last_error(), bad
        assert lib.kfn_conv2d_grad_weights_workspace_bytes(C.byref(d), C.byref(nb)) == ARG, bad
        assert lib.kfn_conv2d_grad_weights(C.byref(d), buf, buf, buf, buf, buf, None) == ARG, bad      # refused before any launch
    # fp16 operands: whole 32-channel tiles and float4 rows of dZ only
    w4 = next(c for c in TB.WGRAD_CASES if c.name == 'W4')
    assert _plan(lib, _desc(w4, TB.F16))[0] == 0
    for bad in (dict(Cin=48, ldx=48), dict(Cout=176), dict(ldy=197)):
        assert _plan(lib, _desc(w4, TB.F16, **bad))[0] == ARG, bad
        assert b'fp16' in lib.kfn_last_error()
        assert _plan(lib, _desc(w4, TB.F32, **bad))[0] == 0, bad
    d = _desc(base, TB.F32)
    tn, tm, tnn, sp, ch = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_long()
    assert lib.kfn_conv2d_grad_weights_plan(None, C.byref(tn), C.byref(tm), C.byref(tnn), C.byref(sp), C.byref(ch)) == ARG
    assert lib.kfn_conv2d_grad_weights_plan(C.byref(d), C.byref(tn), C.byref(tm), C.byref(tnn), C.byref(sp), None) == ARG
    assert lib.kfn_conv2d_grad_weights_plan(C.byref(d), None, C.byref(tm), C.byref(tnn), C.byref(sp), C.byref(ch)) == ARG
    # the plan depends on the shapes alone: the runs at the production sizes, as the launcher has always cut them
    conv1b = _lib.ConvDesc(N=1, H=480, W=640, Cin=64, ldx=64, Cout=64, cout_pad=64, ldy=64, kh=3, kw=3, stride=1)
    assert _plan(lib, conv1b) == (0, (1, 5, 1, 203, 1520))
    assert (480 * 640 - 202 * 1520) % 16 == 0                # ... and why the op-level tests never end on a ragged stage


def test_input_grad_s1_pack_refuses_even_kernels_and_says_why():
    lib = _lib.load()
    n = C.c_size_t(5)
    buf = np.zeros(64, np.float32).ctypes.data
    for kh, kw in TB.EVEN_KERNELS:
        assert lib.kfn_pack_conv_weights_floats(kh, kw, 16, 16, _lib.PACK_INPUT_GRAD_S1, C.byref(n)) == ARG, (kh, kw)
        msg = lib.kfn_last_error()
        assert b'KFN_PACK_INPUT_GRAD_S1' in msg and b'odd' in msg and b'shifted' in msg and ('%dx%d' % (kh, kw)).encode() in msg, msg
        assert n.value == 5
        assert lib.kfn_pack_conv_weights(buf, kh, kw, 16, 16, _lib.PACK_INPUT_GRAD_S1, buf, None) == ARG
        assert lib.kfn_pack_conv_weights_f16(buf, kh, kw, 16, 16, _lib.PACK_INPUT_GRAD_S1, buf, None) == ARG
        # the other two kinds stand: the direct convolution runs even kernels forward
        for kind in (_lib.PACK_FORWARD, _lib.PACK_INPUT_GRAD_S2):
            assert lib.kfn_pack_conv_weights_floats(kh, kw, 16, 16, kind, C.byref(n)) == 0 and n.value == 32 * kh * kw * 16
        n.value = 5
    for kh, kw in ((1, 1), (3, 3), (5, 5), (1, 3), (3, 1), (1, 31)):
        assert lib.kfn_pack_conv_weights_floats(kh, kw, 16, 16, _lib.PACK_INPUT_GRAD_S1, C.byref(n)) == 0, (kh, kw)


@pytest.mark.parametrize('k', [2, 3, 4])
def test_same_convolution_with_the_rotated_kernel_is_the_input_gradient_for_odd_kernels_only(k):
    """Why the refusal: the SAME convolution of dz with the KFN_PACK_INPUT_GRAD_S1 matrix (tests/train_branches.pack_ref, the
    header's formula) against the fp64 input gradient.  3x3: equal.  2x2 and 4x4: SAME pads (k - 1) / 2 in front where the
    rotated kernel needs k / 2, so the convolution is the gradient moved by one pixel up and left: got[y][x] = ref[y + 1][x + 1]."""
    rng = np.random.default_rng(k)
    ci, co, H, Wd = 3, 2, 6, 7
    w = rng.integers(-3, 4, size=(k, k, ci, co)).astype(np.float64)
    dz = rng.integers(-3, 4, size=(2, H, Wd, co)).astype(np.float64)
    pack, live = TB.pack_ref(w, 1)
    wr = pack[:ci, :, :, :co].transpose(1, 2, 3, 0)                  # [kh][kw][co][ci]: the HWIO kernel of dz -> dx
    got = O.conv2d_same(dz, wr, None, 1, False)
    ref = R.conv_grad_input(dz, w, (H, Wd), 1)
    if k % 2:
        assert np.array_equal(got, ref)
        return
    assert not np.array_equal(got, ref)
    assert np.array_equal(got[:, :-1, :-1], ref[:, 1:, 1:])


def test_exact_references_equal_the_fp64_ones_on_a_small_case():
    """tests/train_branches.wgrad_ref (numpy, tap by tap), impulse_wgrad_ref and first_impulse_ref (pure indexing) against
    tests/train_ref.conv_grad_weights (torch autograd in fp64): 3x3 at both strides on odd and even sizes, 1x1 at stride 2."""
    rng = np.random.default_rng(3)
    for n, h, w, ci, co, k, s in ((2, 5, 7, 3, 4, 3, 1), (2, 5, 7, 3, 4, 3, 2), (1, 6, 4, 2, 3, 3, 2), (3, 5, 6, 2, 5, 1, 2), (1, 1, 1, 2, 1, 3, 1),
                                  (2, 7, 1, 2, 2, 3, 2)):
        c = TB.WgradCase('t', n, h, w, ci, co, k, s, 0, co, {}, '')
        x, dz = TB.integer_operands(rng, c)
        dw, db = TB.wgrad_ref(x, dz, k, s)
        rw, rb = R.conv_grad_weights(x, dz, (k, k, ci, co), s)
        assert np.array_equal(dw, rw) and np.array_equal(db, rb), (n, h, w, k, s)
        P = TB.out_pixels(c)
        assert dz.shape[0] * dz.shape[1] * dz.shape[2] == P
        pixels = TB.seam_pixels(P, 4, P // n)
        xr = TB.signed_floats(rng, x.shape)
        iz = TB.impulse_dz(c, pixels)
        assert np.array_equal(iz.reshape(-1, co).sum(0), np.ones(co))
        rw, rb = R.conv_grad_weights(xr, iz, (k, k, ci, co), s)
        assert np.array_equal(TB.impulse_wgrad_ref(xr, c, pixels).astype(np.float64), rw) and np.array_equal(rb, np.ones(co))
    assert TB.seam_pixels(1620, 544, 540) == [0, 539, 540, 543, 544, 1087, 1619]
    assert TB.seam_pixels(1, 16, 1) == [0]
    v = TB.signed_floats(rng, (1000,))
    assert np.all(np.abs(v) >= 0.25) and np.all(np.abs(v) < 4) and (v < 0).any() and (v > 0).any()
    # the first convolution: the preprocessed pixel under the tap, as float32
    img = rng.integers(0, 256, size=(2, 4, 5, 3)).astype(np.uint8)
    pixels = TB.first_pixels((2, 4, 5))
    dz = np.zeros((2 * 4 * 5, 16), np.float32)
    for ch in range(16):
        dz[pixels[ch % len(pixels)], ch] = 1.0
    pre = (img.astype(np.float32) - np.float32(128.0)) * np.float32(0.00625)
    rw, _ = R.conv_grad_weights(pre, dz.reshape(2, 4, 5, 16), (3, 3, 3, 16), 1)
    assert np.array_equal(TB.first_impulse_ref(img, 16, pixels).astype(np.float64), rw.reshape(27, 16))


def test_pack_reference_against_the_host_packer():
    """pack_ref's forward form is kfnet_amd.graph.pack_conv_kernel (the matrix every forward test multiplies by); the two
    input-gradient forms differ by the rotation alone; padding rows and columns are zero."""
    from kfnet_amd.graph import pack_conv_kernel
    rng = np.random.default_rng(4)
    for shape in ((3, 3, 16, 40), (1, 1, 32, 4)) + TB.PACK_RAGGED:
        w = rng.normal(size=shape).astype(np.float32)
        fwd, live = TB.pack_ref(w, 0)
        if shape[2] % 16 == 0:
            assert np.array_equal(fwd.reshape(fwd.shape[0], -1), pack_conv_kernel(w))
        s1, live1 = TB.pack_ref(w, 1)
        s2, live2 = TB.pack_ref(w, 2)
        assert np.array_equal(s1, s2[:, ::-1, ::-1]) and np.array_equal(live1, live2)
        assert s1.shape == (-(-shape[2] // 32) * 32, shape[0], shape[1], -(-shape[3] // 16) * 16)
        assert not s1[~live1].any() and not fwd[~live].any() and live1.sum() == w.size == live.sum()
