"""CPU tests (no GPU): host-side graph construction, the Network DSL mechanics mirrored
from cnn_wrapper/network.py, weight container, C-ABI surface, no-fallback guarantees."""
import ctypes
import os
import re

import numpy as np
import pytest

from kfnet_amd import _lib
from kfnet_amd.graph import (Graph, pack_conv_kernel, pack_deconv_kernel, pack_dense_kernel,
                             variable_scope)
from kfnet_amd.KFNet.KFNet import KFNet, KFNetDataSpec
from kfnet_amd.weights import num_params, synthetic_weights, variable_specs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(B=2, H=480, W=640, **graph_options):
    g = Graph()
    for k, v in graph_options.items():
        assert hasattr(g, k)
        setattr(g, k, v)
    img = g.placeholder((B, H, W, 3), 'u8')
    h, w = -(-H // 8), -(-W // 8)
    st = g.placeholder((1, h, w, 4))
    net = KFNet(img, KFNetDataSpec(batch_size=B, image_size=(H, W)))
    net.GetKFCoordRecursive(st.channels(0, 3), st.channels(3, 1))
    return g, net


def test_library_exports_every_declared_symbol():
    lib_path = os.path.join(ROOT, 'kfnet_amd', 'libkfnet_hip.so')
    if not os.path.exists(lib_path):
        from kfnet_amd import build
        build.build(verbose=False)
    hdr = open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()
    declared = set(re.findall(r'\b(kfn_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    h = ctypes.CDLL(lib_path)
    for name in declared:
        assert hasattr(h, name), name
    lib = _lib.load()
    assert lib.kfn_abi_version() == _lib.ABI_VERSION


def test_assign_layouts_blocks_only_what_winograd_launches_own():
    """Graph.assign_layouts (KFN_LAYOUT_C16, round 6): at the bench batch SCoordNet's tensors from conv1b's output to conv5's lie
    between two launches of wino4b_kernel / wino_s2c_kernel and become channel-blocked; conv1a (written by the first-layer kernel) and
    conv6 (read by the 1x1 conv7) stay NHWC, and so does everything at batch 1, where the stride-2 layers take the F(2,2) kernel.  A
    tensor somebody else also reads, a concat member and a view disqualify; blocked tensors refuse channel views and re-binding."""
    def blocked(g):
        g.resolve_routes()
        return sorted(g.assign_layouts())
    chain = ['conv1b', 'conv2a', 'conv2b', 'conv3a', 'conv3b', 'conv4a', 'conv4b', 'conv5']
    g20, net20 = _build(20)
    assert blocked(g20) == chain
    sc = net20.scoordnet
    assert sc.get_output_by_name('conv1a').layout == 'nhwc' and sc.get_output_by_name('conv6').layout == 'nhwc'
    first = {}
    for op in g20.ops:
        first.setdefault(op.name, op)
    d = first['conv2a'].desc()
    assert (d.x_layout, d.y_layout) == (1, 1)
    d = first['conv1b'].desc()
    assert (d.x_layout, d.y_layout) == (0, 1)           # reads the first-layer kernel's NHWC output
    d = first['conv6'].desc()
    assert (d.x_layout, d.y_layout) == (1, 0)           # writes NHWC for the 1x1 conv7
    assert first['conv7'].desc().x_layout == 0
    t = sc.get_output_by_name('conv3b')
    with pytest.raises(ValueError):
        t.channels(0, 16)
    with pytest.raises(ValueError):
        t.rebind(t.storage, 0, t.shape[3] + 16)
    assert t.batch(1, 2).layout == 'c16'                # batch windows: the image stride is the layout's too
    assert blocked(_build(4)[0]) == ['conv1b', 'conv2a', 'conv2b', 'conv3a', 'conv4b', 'conv5']     # conv4a takes the F(2,2) kernel there
    assert blocked(_build(1)[0]) == []
    assert blocked(_build(20, activation_layout_c16=False)[0]) == []
    # a second reader that is not such a launch (here: the same tensor also handed to a copy-like op) keeps the tensor NHWC
    g, net = _build(20)
    class Peek(object):
        name = 'peek'
        def __init__(self, t):
            self.src = t
    g.ops.append(Peek(net.scoordnet.get_output_by_name('conv2b')))
    assert blocked(g) == [n for n in chain if n != 'conv2b']
    # ... and a reader through a batch VIEW
    g, net = _build(20)
    first = {}
    for op in g.ops:
        first.setdefault(op.name, op)
    first['conv3b'].x = first['conv3b'].x.batch(0, 20)
    assert blocked(g) == [n for n in chain if n != 'conv3a']


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    g, _ = _build(1, 64, 96)
    with pytest.raises(_lib.KfnError):
        g.finalize('cuda:0')
    with pytest.raises(_lib.KfnError):
        g.run(stream=0)   # buffers not allocated -> no silent CPU path


def test_graph_matches_reference_architecture():
    g, net = _build(2)
    want = set()
    for n, kind, shape in variable_specs():
        want |= {n + '/kernel', n + '/bias'}
    # every TF variable is consumed (some in a derived device layout, e.g. conv0's class kernels)
    assert {p.source for p in g.params.values()} == want
    by_source = {p.source: p for p in g.params.values()}
    for n, kind, shape in variable_specs():
        assert by_source[n + '/kernel'].shape == shape, n
    # nominal FLOPs/frame == SURVEY.md App. C (496.224 GFLOP)
    fl = sum(op.flops() for op in g.ops if hasattr(op, 'flops')) / 2
    assert abs(fl / 1e9 - 496.224) < 0.01
    W = synthetic_weights(0)
    assert num_params(W) == 24406724 + 180512 + 511186
    # layer LUT / naming mechanics of the DSL (network.py:96-109)
    sc = net.scoordnet
    assert sc.get_output_by_name('conv4b').shape == (2, 60, 80, 1024)
    assert sc.get_output().shape == (2, 60, 80, 4)
    assert sc.get_unique_name('conv') == 'conv_%d' % (sum(k.startswith('conv') for k in sc.layers) + 1)
    with pytest.raises(KeyError):
        sc.feed('nope')
    with pytest.raises(NotImplementedError):
        sc.feed('conv7').max_pool(2, 2, name='p')


def test_default_routes_of_the_3x3_layers():
    """Which kernel every 3x3 layer of the default (fp32) graph is handed to -- the host mirror of the routing rules
    in kfn_conv2d_winograd_fused / kfn_conv2d_winograd_s2 (csrc/kfn_wino2.hip, kfn_wino_s2.hip) that bench.py's
    per-kernel table and roofline rely on."""
    from kfnet_amd.graph import WinogradFusedConvOp, WinogradS2ConvOp
    g, net = _build(4)
    lib = _lib.load()            # kfn_conv2d_plan is host code: no GPU needed
    four_wave = ()
    f43 = ('conv1b', 'conv2b', 'conv3b', 'conv4b', 'conv5', 'conv6', 'feat5')   # Cin, Cout >= 64: F(4x4,3x3), csrc/kfn_wino4.hip (round 4)
    asked = four_wave + f43 + ('feat3', 'conv2a', 'conv3a', 'conv4a', 'feat6')
    names = {}
    for op in g.ops:       # (first op of a name: SCoordNet / the feature tower come before OFlowNet's same-named layers)
        if op.name in asked and op.name not in names:
            names[op.name] = op.kernel_name(lib)
    for n in four_wave:
        assert names[n] == 'wino3_kernel', (n, names[n])
    for n in f43:
        assert names[n] == 'wino4b_kernel', (n, names[n])      # the eight-wave form (Graph.winograd_f43_eight_wave)
    g4, _ = _build(4, winograd_f43_eight_wave=False)
    k4 = [op for op in g4.ops if op.name == 'conv4b'][0]
    assert k4.kernel_name(lib) == 'wino4_kernel' and k4.kernel.pack.__name__ == 'pack_winograd_f43_kernel' and k4.desc().wino_form == 2
    k8 = [op for op in g.ops if op.name == 'conv4b'][0]
    assert k8.kernel.pack.__name__ == 'pack_winograd_f43_kernel_b' and k8.desc().wino_form == 3
    # the pair layout against its index formula (include/kfnet_hip.h)
    from kfnet_amd.graph import pack_winograd_f43_kernel, pack_winograd_f43_kernel_b
    wr = np.random.default_rng(5).normal(size=(3, 3, 16, 40)).astype(np.float32)
    ua, ub = pack_winograd_f43_kernel(wr), pack_winograd_f43_kernel_b(wr)
    assert ua.shape == (2, 36, 64, 8) and ub.shape == (2, 18, 64, 16)
    for (ci, co, pp) in [(0, 0, 0), (13, 39, 35), (6, 17, 22), (9, 5, 7)]:
        assert ub[ci // 8, pp // 2, co, 4 * ((ci % 8) // 2) + 2 * (pp % 2) + ci % 2] == ua[ci // 8, pp, co, ci % 8]
    assert names['feat3'] == 'wino2_kernel'                  # 32 -> 32: one wave per 32 output channels
    # stride 2: polyphase + F(4,2) (wino_s2c_kernel, round 6) where the launch has >= 1024 of its 16x16-pixel workgroups (batch 4:
    # conv2a 2400, conv3a 1200), the F(2,2) eight-wave form below that (conv4a 600, feat6 75)
    for n in ('conv2a', 'conv3a'):
        assert names[n] == 'wino_s2c_pkernel', (n, names[n])   # 2400 / 1200 workgroups: the persistent form (>= 2 per CU)
    for n in ('conv4a', 'feat6'):
        assert names[n] == 'wino_s2b_kernel', (n, names[n])      # the eight-wave form (Graph.winograd_s2_eight_wave)
    kc = [op for op in g.ops if op.name == 'conv3a'][0]
    assert kc.kernel.pack.__name__ == 'pack_winograd_s2_kernel_c' and kc.desc().wino_form == 5 and kc.workgroups() == 1200
    assert kc.mfma_flops() == 2.0 * 81 * (4 * 30 * 40) * 512 * 256           # 81 products per 4x4 tile and channel pair
    def s2_layers(gr):      # SCoordNet's (the first of each name: OFlowNet has layers of the same names on its 8x8 windows)
        first = {}
        for op in gr.ops:
            first.setdefault(op.name, op)
        return [first[nm] for nm in ('conv2a', 'conv3a', 'conv4a')]
    g20, _ = _build(20)
    assert [op.kernel_name(lib) for op in s2_layers(g20)] == ['wino_s2c_pkernel'] * 3
    g1, _ = _build(1)
    assert all(op.kernel_name(lib).startswith('wino_s2b_kernel') for op in s2_layers(g1))
    gn, _ = _build(20, winograd_s2_f42=False)
    assert all(op.kernel_name(lib) == 'wino_s2b_kernel' for op in s2_layers(gn))
    # a concat that re-binds the output to a window the 16-byte stores cannot take: resolve_routes() falls back to the F(2,2) form
    kf = s2_layers(g20)[2]
    kf.y._ld, kf.y._off = kf.y.shape[3] + 2, 2
    g20.resolve_routes()
    assert kf.kernel_name(lib) == 'wino_s2b_kernel' and kf.kernel.pack.__name__ == 'pack_winograd_s2_kernel_b' and kf.desc().wino_form == 4
    gs, _ = _build(4, winograd_s2_eight_wave=False, winograd_s2_f42=False)
    ks = [op for op in gs.ops if op.name == 'conv3a'][0]
    assert ks.kernel_name(lib) == 'wino_s2_kernel' and ks.kernel.pack.__name__ == 'pack_winograd_s2_kernel' and ks.desc().wino_form == 0
    from kfnet_amd.graph import pack_winograd_s2_kernel, pack_winograd_s2_kernel_b
    ws = np.random.default_rng(6).normal(size=(3, 3, 16, 40)).astype(np.float32)
    sa, sb = pack_winograd_s2_kernel(ws), pack_winograd_s2_kernel_b(ws)
    assert sa.shape == (2, 16, 64, 8) and sb.shape == (2, 8, 64, 16)
    for (ci, co, f) in [(0, 0, 0), (13, 39, 15), (6, 17, 9), (9, 5, 4)]:
        assert sb[ci // 8, f // 2, co, 4 * ((ci % 8) // 2) + 2 * (f % 2) + ci % 2] == sa[ci // 8, f, co, ci % 8]
    by_name = {}
    for op in g.ops:
        by_name.setdefault(op.name, op)
    g2, net2 = _build(2, winograd_f43_min_channels=0)      # without F(4x4,3x3): the four-wave F(2x2,3x3) kernel
    by2 = {}
    for op in g2.ops:
        by2.setdefault(op.name, op)
    c2b = by2['conv2b']
    assert not c2b.two_wave() and c2b.four_wave() and c2b.kernel_name(lib) == 'wino3_kernel'
    assert isinstance(by2['conv1b'], WinogradFusedConvOp) and by2['conv1b'].two_wave()      # 64 -> 64: two waves share one transform
    assert by2['conv1b'].kernel_name(lib) == 'wino3_pair_kernel' and by2['feat5'].kernel_name(lib) == 'wino3_pair_kernel'
    assert isinstance(by_name['conv2a'], WinogradS2ConvOp)
    from kfnet_amd.graph import WinogradF43ConvOp
    op4 = by_name['conv4b']
    assert isinstance(op4, WinogradF43ConvOp)
    n4, h4, w4, c4 = op4.y.shape            # 60x80: 15 x 20 tiles of 4x4 pixels, 5 column blocks, rows packed over the batch
    assert op4.mfma_flops() == 2.0 * 36 * 20 * (-(-(n4 * 15) // 8) * 8) * 1024 * 1024
    assert op4.flops() / op4.mfma_flops() == pytest.approx(4.0 * (n4 * 15) / (-(-(n4 * 15) // 8) * 8))   # 36 products per 16 outputs instead of 144
    g0, net0 = _build(2, winograd_f43_min_channels=0)
    assert all(type(op).__name__ != 'WinogradF43ConvOp' for op in g0.ops)
    # a single frame: launches of fewer than 128 F(4x4) workgroups (conv5: 10 tile blocks x 8 channel groups, conv6: 10 x 4,
    # feat5: 40 x 1) would leave most CUs idle and go to the F(2x2,3x3) kernels; conv4b (10 x 16 = 160) stays -- round 4's
    # routing, which is what Graph.winograd_f43_max_k_split = 1 restores (round 5 splits their input channels instead:
    # test_f43_split_k_is_chosen_for_single_frames_only)
    g1, net1 = _build(1, winograd_f43_max_k_split=1)
    by1 = {}
    for op in g1.ops:
        by1.setdefault(op.name, op)
    assert WinogradF43ConvOp.workgroups(by1['conv4b'].x.shape, 1024) == 160
    assert WinogradF43ConvOp.workgroups(by1['conv5'].x.shape, 512) == 80
    assert [type(by1[n]).__name__ for n in ('conv4b', 'conv5', 'conv6', 'feat5')] == \
        ['WinogradF43ConvOp', 'WinogradFusedConvOp', 'WinogradFusedConvOp', 'WinogradFusedConvOp']
    g1b, _ = _build(1, winograd_f43_min_workgroups=0, winograd_f43_max_k_split=1)
    assert sum(type(op).__name__ == 'WinogradF43ConvOp' for op in g1b.ops) == 7
    # executed MFMA FLOPs of the two-wave form: all 64 channels in one column block (no padding to 128)
    op = by2['conv1b']
    n, ho, wo, co = op.y.shape
    assert op.mfma_flops() == 2.0 * 16 * (-(-((wo + 1) // 2) // 8) * 8) * (-(-(n * ((ho + 1) // 2)) // 4) * 4) * 64 * 64


def test_concat_is_zero_copy_rebinding():
    g, net = _build(1, 64, 96)
    of = net.oflownet
    for cat, parts in (('concat2', ('upconv2', 'conv2b')), ('concat1', ('upconv1', 'conv1b')),
                       ('concat0', ('upconv0', 'conv0'))):
        c = of.get_output_by_name(cat)
        off = 0
        for p in parts:
            t = of.get_output_by_name(p)
            assert t.root_storage is c.root_storage and t.ld == c.C and t.ch_off == off
            off += t.C
    assert not any(op.name == 'copy_channels' for op in g.ops)


def test_odd_grid_shapes():
    g, net = _build(1, 540, 960)
    assert net.scoordnet.get_output().shape == (1, 68, 120, 4)   # ceil, not eval.py's 540//8 = 67
    assert net.temp_feat_maps.shape == (2, 68, 120, 32)


def test_weight_packing_layouts():
    rng = np.random.default_rng(0)
    w = rng.normal(size=(3, 3, 16, 5)).astype(np.float32)
    p = pack_conv_kernel(w)
    assert p.shape == (32, 144) and np.all(p[5:] == 0)
    assert p[3, (1 * 3 + 2) * 16 + 7] == w[1, 2, 7, 3]
    wd = rng.normal(size=(3, 3, 6, 16)).astype(np.float32)   # [kh,kw,Cout,Cin]
    pd = pack_deconv_kernel(wd)
    assert pd.shape == (32, 144) and pd[4, (2 * 3 + 0) * 16 + 9] == wd[2, 0, 4, 9]
    wf = rng.normal(size=(128, 64)).astype(np.float32)
    assert np.array_equal(pack_dense_kernel(wf)[:64], wf.T)


def test_round3_weight_layouts_follow_their_documented_index_formulas():
    """The device layouts the window-resident OFlowNet kernels and the fp16-activation convolution read, element by
    element against the index expressions in their docstrings / include/kfnet_hip.h (seeded random kernels)."""
    from kfnet_amd.graph import (pack_conv_kernel_chunked, pack_oflow_head_kernel, pack_oflow_tail_kernel,
                                 pack_oflow_upconv_kernel, pack_winograd_fused_kernel)
    rng = np.random.default_rng(11)
    # chunk-major conv weights: [K/32][cout_pad][32], K = (kh, kw, ci)
    w = rng.normal(size=(3, 3, 64, 40)).astype(np.float32)
    m = pack_conv_kernel_chunked(w)
    assert m.shape == (9 * 64 // 32, 64, 32)
    for (ky, kx, ci, co) in [(0, 0, 0, 0), (1, 2, 37, 39), (2, 2, 63, 5), (2, 0, 31, 17)]:
        k = (ky * 3 + kx) * 64 + ci
        assert m[k // 32, co, k % 32] == w[ky, kx, ci, co]
    assert np.all(m[:, 40:, :] == 0)                       # channels 40..63 of the padded column tile
    # oflow_head: fragment t = (tap*8 + j)*2 + nb of lane (kq, n) = w[tap][kq*8 + j][nb*16 + n]
    w1 = rng.normal(size=(3, 3, 32, 32)).astype(np.float32)
    h = pack_oflow_head_kernel(w1)
    assert h.shape == (144, 64)
    for (tap, j, nb, kq, n) in [(0, 0, 0, 0, 0), (4, 7, 1, 3, 15), (8, 3, 0, 2, 9)]:
        assert h[(tap * 8 + j) * 2 + nb, kq * 16 + n] == w1[tap // 3, tap % 3, kq * 8 + j, nb * 16 + n]
    # oflow_tail2's upconv0: fragment t = tap*8 + j of lane (kq, n) = w[tap][n][kq*8 + j]  (conv2d_transpose: [3,3,Cout,Cin])
    wu = rng.normal(size=(3, 3, 16, 32)).astype(np.float32)
    u = pack_oflow_upconv_kernel(wu)
    assert u.shape == (72, 64)
    for (tap, j, kq, n) in [(0, 0, 0, 0), (5, 6, 3, 11), (8, 7, 1, 15)]:
        assert u[tap * 8 + j, kq * 16 + n] == wu[tap // 3, tap % 3, n, kq * 8 + j]
    # conv6: fragment t = tap*12 + j of lane (kq, n) = w[tap][kq*12 + j][n]
    w6 = rng.normal(size=(3, 3, 48, 16)).astype(np.float32)
    t6 = pack_oflow_tail_kernel(w6)
    assert t6.shape == (108, 64)
    for (tap, j, kq, n) in [(0, 0, 0, 0), (7, 11, 3, 15), (3, 5, 2, 8)]:
        assert t6[tap * 12 + j, kq * 16 + n] == w6[tap // 3, tap % 3, kq * 12 + j, n]
    # single-kernel Winograd: u2[((ci/8)*16 + 4*xi + nu)*cout_pad + co][ci%8] = (G g G^T)[xi][nu]  (include/kfnet_hip.h)
    ww = rng.normal(size=(3, 3, 16, 24)).astype(np.float32)
    u2 = pack_winograd_fused_kernel(ww).reshape(2, 16, 32, 8)
    G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
    for (ci, co) in [(0, 0), (9, 23), (15, 7)]:
        U = G @ ww[:, :, ci, co].astype(np.float64) @ G.T
        assert np.allclose(u2[ci // 8, :, co, ci % 8].reshape(4, 4), U, rtol=1e-6, atol=1e-7)
    assert np.all(u2[:, :, 24:, :] == 0)


def test_round4_fp16_weight_layouts_follow_their_documented_index_formulas():
    """The half-precision operand layouts of config 5's own kernels (round 4), element by element against the index
    expressions of their docstrings: kfn_conv3x3_c64_f16's A fragments and the 16x16x16 B fragments of the window-resident
    OFlowNet kernels; a CPU emulation of the conv64 kernel's MFMA bookkeeping (weights as A, pixels as B, three kernel rows
    on three accumulator sets) reproduces the oracle's convolution."""
    from kfnet_amd.graph import (pack_conv64_rows_kernel, pack_oflow_head_kernel_f16, pack_oflow_tail_kernel_f16,
                                 pack_oflow_upconv_kernel_f16)
    rng = np.random.default_rng(12)
    w = rng.normal(size=(3, 3, 64, 64)).astype(np.float32)
    a = pack_conv64_rows_kernel(w)
    assert a.shape == (2, 36, 64, 8) and a.dtype == np.float16
    for (half, dy, dx, c, lane, t) in [(0, 0, 0, 0, 0, 0), (1, 2, 1, 3, 63, 7), (0, 1, 2, 2, 37, 5), (1, 0, 2, 1, 31, 0)]:
        i, hk = lane % 32, lane // 32
        assert a[half, (dy * 3 + dx) * 4 + c, lane, t] == np.float16(w[dy, dx, 16 * c + 8 * hk + t, 32 * half + i])
    # emulate the kernel's arithmetic on one 3-row, 32-pixel patch: D[ch][px] += A[ch][k] B[k][px] per (dy, dx, c)
    x = rng.normal(size=(3, 34, 64)).astype(np.float16).astype(np.float64)      # input rows r-1, r, r+1; pixels -1 .. 32
    af = a.astype(np.float64)
    out = np.zeros((64, 32))
    for half in range(2):
        for dy in range(3):
            for dx in range(3):
                for c in range(4):
                    frag = af[half, (dy * 3 + dx) * 4 + c]                       # [lane][t] -> A[i][k = 8 hk + t]
                    A = np.zeros((32, 16))
                    for lane in range(64):
                        A[lane % 32, 8 * (lane // 32):8 * (lane // 32) + 8] = frag[lane]
                    B = x[dy, dx:dx + 32, 16 * c:16 * c + 16].T                  # [k][px]: pixel j + dx of the LDS row
                    out[32 * half:32 * half + 32] += A @ B
    ref = np.einsum('yxc,yxco->o', x[:, 0:3], w.astype(np.float16).astype(np.float64))   # pixel 0 of the output row
    assert np.allclose(out[:, 0], ref, rtol=1e-12, atol=1e-12)
    ref31 = np.einsum('yxc,yxco->o', x[:, 31:34], w.astype(np.float16).astype(np.float64))
    assert np.allclose(out[:, 31], ref31, rtol=1e-12, atol=1e-12)
    # oflow_head_f16: fragment t = (tap*2 + s)*2 + nb of lane (kq, n), half j = w[tap][kq*8 + 4s + j][nb*16 + n]
    w1 = rng.normal(size=(3, 3, 32, 32)).astype(np.float32)
    h = pack_oflow_head_kernel_f16(w1)
    assert h.shape == (36, 64, 4) and h.dtype == np.float16
    for (tap, s_, nb, kq, n, j) in [(0, 0, 0, 0, 0, 0), (8, 1, 1, 3, 15, 3), (4, 0, 1, 2, 7, 2)]:
        assert h[(tap * 2 + s_) * 2 + nb, kq * 16 + n, j] == np.float16(w1[tap // 3, tap % 3, kq * 8 + 4 * s_ + j, nb * 16 + n])
    # oflow_tail2_f16 upconv0: fragment t = tap*2 + s, half j = w[tap][n][kq*8 + 4s + j]
    wu = rng.normal(size=(3, 3, 16, 32)).astype(np.float32)
    u = pack_oflow_upconv_kernel_f16(wu)
    assert u.shape == (18, 64, 4)
    for (tap, s_, kq, n, j) in [(0, 0, 0, 0, 0), (8, 1, 3, 15, 3), (5, 1, 1, 9, 2)]:
        assert u[tap * 2 + s_, kq * 16 + n, j] == np.float16(wu[tap // 3, tap % 3, n, kq * 8 + 4 * s_ + j])
    # oflow_tail2_f16 conv6: fragment t = tap*3 + s, half j = w[tap][kq*12 + 4s + j][n]
    w6 = rng.normal(size=(3, 3, 48, 16)).astype(np.float32)
    t6 = pack_oflow_tail_kernel_f16(w6)
    assert t6.shape == (27, 64, 4)
    for (tap, s_, kq, n, j) in [(0, 0, 0, 0, 0), (8, 2, 3, 15, 3), (3, 1, 2, 8, 1)]:
        assert t6[tap * 3 + s_, kq * 16 + n, j] == np.float16(w6[tap // 3, tap % 3, kq * 12 + 4 * s_ + j, n])


def test_config5_graph_routes_conv1b_and_the_window_kernels_to_their_fp16_forms():
    """conv_operands = 'f16' (BASELINE config 5): SCoordNet's conv1b goes to kfn_conv3x3_c64_f16, the two window-resident
    OFlowNet launches to their _f16 entry points with half-precision packers; the fp32 graph keeps the fp32 forms; every
    switch turns its route off."""
    g, net = _build(B=2, H=540, W=960, conv_operands='f16')
    by = {}
    for op in g.ops:
        by.setdefault(op.name, op)
    assert type(by['conv1b']).__name__ == 'Conv64RowsF16Op' and by['conv1b'].kernel.pack.__name__ == 'pack_conv64_rows_kernel'
    assert by['conv1b'].kernel_name(_lib.load()) == 'conv64_rows_kernel<3, true>'          # 960 = 5 x 192
    head = [op for op in g.ops if op.name.startswith('oflow_head')][0]
    tail = [op for op in g.ops if op.name.startswith('oflow_tail2')][0]
    assert head.operands_f16 and head.k1.pack.__name__ == 'pack_oflow_head_kernel_f16'
    assert tail.operands_f16 and tail.ku.pack.__name__ == 'pack_oflow_upconv_kernel_f16' and tail.k6.pack.__name__ == 'pack_oflow_tail_kernel_f16'
    g32, _ = _build(B=2, H=540, W=960)
    assert all(type(op).__name__ != 'Conv64RowsF16Op' and not getattr(op, 'operands_f16', False) for op in g32.ops)
    goff, _ = _build(B=2, H=540, W=960, conv_operands='f16', conv64_rows_f16=False, oflow_tail_f16=False)
    assert all(type(op).__name__ != 'Conv64RowsF16Op' and not getattr(op, 'operands_f16', False) for op in goff.ops)
    d = by['conv1b'].desc()
    assert _lib.load().kfn_conv3x3_c64_f16_supported(ctypes.byref(d)) == 1                # host code: no GPU needed


def test_variable_scope_names():
    g = Graph()
    with variable_scope('A'):
        with variable_scope('B'):
            p = g.variable('x/kernel', (1,), lambda a: a)
    assert p.name == 'A/B/x/kernel'
    with variable_scope('A'):
        with variable_scope('B'):
            assert g.variable('x/kernel', (1,), lambda a: a) is p   # AUTO_REUSE


def test_dataspec_matches_reference_table():
    s = KFNetDataSpec()
    assert s.scene == 'stairs' and s.sequence_length == 500 and s.image_num == 2000
    assert KFNetDataSpec(scene='heads').sequence_length == 1000


def test_header_is_plain_c_and_a_c_host_links(tmp_path):
    """The boundary is a C ABI: the header must compile as C99 and as C++, and a C program
    must link against libkfnet_hip.so and reach the entry points that need no GPU."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = os.path.join(root, 'include', 'kfnet_hip.h')
    lib = os.path.join(root, 'kfnet_amd', 'libkfnet_hip.so')
    if shutil.which('gcc') is None or not os.path.exists(lib):
        pytest.skip('needs gcc and the built library')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-fsyntax-only', '-x', 'c', hdr])
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-fsyntax-only', '-x', 'c++', hdr])
    src = tmp_path / 'host.c'
    src.write_text('#include "kfnet_hip.h"\n#include <stdio.h>\n'
                   'int main(void) {\n'
                   '  kfn_conv_desc d = KFN_CONV_DESC_INIT;\n'
                   '  int ho = 0, wo = 0;\n'
                   '  d.N = 1; d.H = 480; d.W = 640; d.Cin = 64; d.ldx = 64; d.Cout = 256; d.cout_pad = 256; d.ldy = 256;\n'
                   '  d.kh = 3; d.kw = 3; d.stride = 2;\n'
                   '  if (kfn_conv2d_out_shape(&d, &ho, &wo) != KFN_OK) return 1;\n'
                   '  /* a host compiled against an OLDER, shorter struct: fields beyond its size read as 0 */\n'
                   '  d.struct_size = (int)offsetof(kfn_conv_desc, x_dtype);\n'
                   '  d.weights_path = 77; d.k_step = 5;   /* beyond the declared size: must be ignored */\n'
                   '  if (kfn_conv2d_out_shape(&d, &ho, &wo) != KFN_OK) return 2;\n'
                   '  /* no struct_size (an ABI <= 4 host): a clean argument error, never an out-of-bounds read */\n'
                   '  d.struct_size = 0;\n'
                   '  if (kfn_conv2d_out_shape(&d, &ho, &wo) != KFN_ERR_ARG) return 3;\n'
                   '  d.struct_size = (int)sizeof(kfn_conv_desc) + 4;\n'
                   '  if (kfn_conv2d_out_shape(&d, &ho, &wo) != KFN_ERR_ARG) return 4;\n'
                   '  printf("%d %d %d\\n", kfn_abi_version(), ho, wo);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / 'host'
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(root, 'include'), str(src), '-o', str(exe),
                           '-L', os.path.dirname(lib), '-lkfnet_hip', '-Wl,-rpath,' + os.path.dirname(lib)])
    out = subprocess.check_output([str(exe)]).decode().split()
    from kfnet_amd._lib import ABI_VERSION
    assert out == [str(ABI_VERSION), '240', '320']          # ABI version, TF-SAME output size of conv2a


def _header_struct_fields(text, name):
    """Member names of `typedef struct <name> { ... } <name>;` in declaration order (comments stripped;
    `int32_t a, b;` and `float t[12];` forms)."""
    import re
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), text, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    out = []
    for stmt in body.split(';'):
        stmt = stmt.strip()
        if not stmt:
            continue
        typ, names = stmt.split(None, 1)
        for n in names.split(','):
            m = re.match(r'\s*(\w+)\s*(\[(\d+)\])?\s*$', n)
            out.append((m.group(1), typ, int(m.group(3)) if m.group(3) else 1))
    return out


def test_conv_desc_matches_header_and_integration_doc():
    """VERDICT r3 Weak #6: kfn_conv_desc grew (weights_path) while _lib.py, the header and INTEGRATION.md drifted apart.
    The three field lists -- include/kfnet_hip.h, kfnet_amd._lib.ConvDesc, the reference-side stub in INTEGRATION.md --
    must name the same members in the same order, the struct must start with struct_size, and the ABI numbers agree."""
    import ctypes as C
    import re
    from kfnet_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'kfnet_hip.h')).read()
    fields = _header_struct_fields(hdr, 'kfn_conv_desc')
    assert all(t == 'int32_t' and n == 1 for _, t, n in fields)
    names = [f[0] for f in fields]
    assert names[0] == 'struct_size'
    assert names == [f[0] for f in _lib.ConvDesc._fields_]
    assert C.sizeof(_lib.ConvDesc) == 4 * len(names)
    assert _lib.ConvDesc(N=1).struct_size == C.sizeof(_lib.ConvDesc)
    doc = open(os.path.join(root, 'INTEGRATION.md')).read()
    snippet = re.search(r'class ConvDesc\(C\.Structure\):.*?_fields_ = \[\(n, C\.c_int32\) for n in \((.*?)\)\]', doc, re.S).group(1)
    assert re.findall(r"'(\w+)'", snippet) == names
    abi = int(re.search(r'#define KFN_ABI_VERSION (\d+)', hdr).group(1))
    assert abi == _lib.ABI_VERSION
    assert 'kfn_abi_version() == %d' % abi in doc
    # the scan descriptor too
    kf = _header_struct_fields(hdr, 'kfn_kalman_desc')
    assert [f[0] for f in kf] == [f[0] for f in _lib.KalmanDesc._fields_]
    width = {'int32_t': 4, 'float': 4, 'double': 8}       # min_uncertainty is a double (ABI 13), 8-byte aligned at offset 24
    assert sum(width[f[1]] * f[2] for f in kf) == C.sizeof(_lib.KalmanDesc)           # no padding: 88 bytes
    assert _lib.KalmanDesc.min_uncertainty.offset == 24 and _lib.KalmanDesc.min_uncertainty.size == 8


def test_every_header_function_is_bound_and_exported():
    """Every `int kfn_*(` / `const char* kfn_*(` prototype of the header has a ctypes signature in _lib.SYMBOLS with the
    same number of parameters, and nothing is bound that the header does not declare."""
    import re
    from kfnet_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'kfnet_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    protos = dict()
    for m in re.finditer(r'(?:int|const char\*)\s+(kfn_\w+)\s*\(([^;{]*?)\)\s*;', hdr, re.S):
        args = m.group(2).strip()
        protos[m.group(1)] = 0 if args in ('', 'void') else len(args.split(','))
    assert set(protos) == set(_lib.SYMBOLS)
    for name, n in protos.items():
        assert len(_lib.SYMBOLS[name][1]) == n, name


def test_kernel_sources_have_no_build_switches():
    """The library is built one way (kfnet_amd/build.py): no source selects code by a KFN_ macro
    that a -D could flip, so the sources read as what ships."""
    csrc = os.path.join(ROOT, 'kfnet_amd', 'csrc')
    cond = re.compile(r'^\s*#\s*(if|ifdef|ifndef|elif|elifdef|elifndef)\b.*\bKFN_.*$', re.M)
    found = []
    for name in sorted(os.listdir(csrc)):
        path = os.path.join(csrc, name)
        if os.path.isfile(path):
            text = open(path, errors='replace').read()
            found += ['%s:%d: %s' % (name, text.count('\n', 0, m.start()) + 1, m.group(0).strip())
                      for m in cond.finditer(text)]
    assert not found, '\n'.join(found)


def test_loader_generated_cost_volume_route_packs_conv0_for_the_direct_kernel():
    """with Graph.factor_cost_volume = False conv0's kernel variable goes to kfn_cost_volume_conv,
    which reads the [cout_pad][9 Cin] direct-convolution layout -- whatever route Network.conv had picked for the layer
    (3x3 stride 1 on an 8x8 grid with 32 channels qualifies for the Winograd kernels since round 3)."""
    from kfnet_amd.graph import Graph, pack_bias, pack_conv_kernel
    from kfnet_amd.KFNet.KFNet import KFNet, KFNetDataSpec
    g = Graph()
    g.factor_cost_volume = False
    images = g.placeholder((2, 64, 96, 3), 'u8', name='images')
    state = g.placeholder((1, 8, 12, 4), name='last_state')
    net = KFNet(images, KFNetDataSpec(batch_size=2, image_size=(64, 96)))
    net.GetKFCoordRecursive(state.channels(0, 3), state.channels(3, 1), transform=None, reset_period=500, nis_gate=0.0,
                            emit_temp=False, emit_nis=False)
    fused = [op for op in net.pair_ops if type(op).__name__ == 'CostVolumeConvOp']
    assert len(fused) == 1
    assert fused[0].kernel.pack is pack_conv_kernel and fused[0].bias.pack is pack_bias
    assert not any(type(op).__name__ in ('CostVolumeOp', 'OFlowHeadOp') for op in net.pair_ops)


def test_comm_entry_points_validate_arguments_without_a_gpu():
    """kfn_comm_* / kfn_send_state / kfn_recv_state (the RCCL hand-off of include/kfnet_hip.h) are
    exported and reject bad arguments before touching RCCL or the device."""
    import ctypes as C
    from kfnet_amd import _lib
    lib = _lib.load()
    for name in ('kfn_comm_unique_id', 'kfn_comm_init', 'kfn_comm_destroy', 'kfn_comm_rank', 'kfn_send_state',
                 'kfn_recv_state'):
        assert hasattr(lib, name)
    buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
    comm = C.c_void_p()
    assert lib.kfn_comm_unique_id(None, _lib.COMM_ID_BYTES) == -1
    assert lib.kfn_comm_unique_id(buf, 64) == -1 and b'128-byte' in lib.kfn_last_error()
    assert lib.kfn_comm_init(None, 0, 1, buf, 0) == -1
    assert lib.kfn_comm_init(C.byref(comm), 0, 1, None, 0) == -1
    assert lib.kfn_comm_init(C.byref(comm), 2, 2, buf, 0) == -1 and b'bad rank' in lib.kfn_last_error()
    assert lib.kfn_comm_init(C.byref(comm), 0, 1, buf, -1) == -1
    assert not comm.value
    x = (C.c_float * 16)()
    assert lib.kfn_send_state(None, 1, x, 2, 2, None) == -1 and b'null communicator' in lib.kfn_last_error()
    assert lib.kfn_recv_state(None, 0, x, 2, 2, None) == -1
    assert lib.kfn_comm_destroy(None) == 0      # destroying nothing is fine
    assert lib.kfn_comm_rank(None, None, None) == -1


def test_handoff_links_share_one_interface():
    from kfnet_amd import dist as D
    for cls in (D.TorchLink, D.RcclLink, D.LoopbackLink):
        for m in ('recv', 'send', 'close'):
            assert callable(getattr(cls, m))
    box = {}
    import torch
    a, b = D.LoopbackLink(box, 0), D.LoopbackLink(box, 1)
    s = torch.arange(8.0)
    a.send(s, 1)
    r = torch.zeros(8)
    b.recv(r, 0)
    assert torch.equal(r, s) and not box


def test_epilogue_on_a_winograd_routed_layer_reroutes_to_the_direct_kernel():
    """with winograd_min_channels <= 32, feat7 (3x3, 128 -> 32) would take the Winograd
    path, which has no fused epilogue -- tf.nn.l2_normalize must not be dropped silently."""
    from kfnet_amd import _lib
    from kfnet_amd.graph import ConvOp, Graph, WinogradConvOp, WinogradFusedConvOp, pack_conv_kernel
    from kfnet_amd.KFNet.KFNet import KFNet, KFNetDataSpec
    g = Graph()
    g.winograd_min_channels = 32
    assert g.winograd_fused_min_channels <= 32       # feat7 (128 -> 32) is Winograd-routed before its epilogue is set
    images = g.placeholder((2, 64, 96, 3), 'u8', name='images')
    net = KFNet(images, KFNetDataSpec(batch_size=2, image_size=(64, 96)))
    feat7 = [op for op in net.feat_tower.ops if op.name == 'feat7']
    assert len(feat7) == 1 and type(feat7[0]) is ConvOp and feat7[0].epilogue == _lib.EPI_L2NORM
    assert feat7[0].kernel.pack is pack_conv_kernel and feat7[0] in net.frame_ops and feat7[0] in g.ops
    # the other wide stride-1 layers of the tower did go to Winograd with this setting
    assert any(isinstance(op, (WinogradConvOp, WinogradFusedConvOp)) for op in net.feat_tower.ops)
    with pytest.raises(KeyError):
        net.feat_tower.set_epilogue('no_such_layer', _lib.EPI_L2NORM)


def test_epilogue_on_f43_and_conv64_routed_layers_reroutes_to_the_direct_kernel():
    """a 3x3 layer with >= 64 channels is routed to WinogradF43ConvOp (fp32) / Conv64RowsF16Op (fp16
    activations); neither kernel carries head epilogues, so set_epilogue must put the layer back on the direct kernel
    with the direct kernel's weight packing (and, for fp16, keep the operand type)."""
    from kfnet_amd import _lib
    from kfnet_amd.cnn_wrapper.network import Network
    from kfnet_amd.graph import (Conv64RowsF16Op, ConvOp, Graph, WinogradF43ConvOp, pack_conv_kernel, variable_scope)

    class Two(Network):
        def setup(self):
            (self.feed('input').conv(3, 64, 1, name='a').conv(3, 64, 1, name='b'))

    g = Graph()
    x = g.placeholder((32, 64, 96, 64), name='input')
    net = Two({'input': x}, is_training=False)
    b = [op for op in net.ops if op.name == 'b'][0]
    assert isinstance(b, WinogradF43ConvOp) and b.eight_wave
    net.set_epilogue('b', _lib.EPI_EXP_CH3)
    assert type(b) is ConvOp and b.epilogue == _lib.EPI_EXP_CH3 and b.kernel.pack is pack_conv_kernel
    assert not hasattr(b, 'eight_wave') and b.desc().wino_form == 0
    # packed weights have the direct kernel's [cout_pad][9 Cin] shape
    w = np.arange(3 * 3 * 64 * 64, dtype=np.float32).reshape(3, 3, 64, 64)
    assert b.kernel.pack(w).shape == (64, 576)
    a = [op for op in net.ops if op.name == 'a'][0]
    assert isinstance(a, WinogradF43ConvOp)          # untouched neighbour

    g16 = Graph()
    g16.conv_operands = 'f16'
    g16.f16_activation_scopes = ('S',)
    x16 = g16.placeholder((2, 64, 96, 64), dtype='f16', name='input')
    with variable_scope('S'):
        net16 = Two({'input': x16}, is_training=False)
    b16 = [op for op in net16.ops if op.name == 'b'][0]
    assert isinstance(b16, Conv64RowsF16Op)
    net16.set_epilogue('b', _lib.EPI_EXP_CH3)
    assert type(b16) is ConvOp and b16.operand_dtype == _lib.OPERAND_F16 and b16.epilogue == _lib.EPI_EXP_CH3
    p = b16.kernel.pack(w)
    assert p.dtype == np.float16 and p.size == 64 * 576          # chunk-major fp16 weights of the direct kernel


def test_bench_telemetry_picks_the_busy_card_and_parses_sysfs(tmp_path):
    """bench.py's clock / power sampler on a fake sysfs tree: partition nodes (no pp_dpm_sclk) are ignored;
    when the PCI address cannot be matched (no GPU here) every card is watched and the busiest reported."""
    import time
    bench, _ = _load_bench()
    for i, (busy, mhz, uw) in enumerate([(0, 132, 90000000), (97, 2104, 912000000)]):
        d = tmp_path / ('card%d' % i) / 'device'
        (d / 'hwmon' / 'hwmon3').mkdir(parents=True)
        (d / 'pp_dpm_sclk').write_text('0: 132Mhz %s\n1: %dMhz %s\n' % ('*' if mhz == 132 else '', mhz, '' if mhz == 132 else '*'))
        (d / 'gpu_busy_percent').write_text('%d\n' % busy)
        (d / 'hwmon' / 'hwmon3' / 'power1_average').write_text('%d\n' % uw)
    (tmp_path / 'card9' / 'device').mkdir(parents=True)      # a partition node
    t = bench.Telemetry(0, period=0.02, sysfs=str(tmp_path))
    with t:
        time.sleep(0.2)
    s = t.summary()
    assert s['samples_during_timed_region'] >= 3 and 'card1' in s['source'] and 'busiest of 2' in s['source']
    assert s['sclk_mhz']['mean'] == 2104.0 and s['power_w']['max'] == 912.0 and s['busy_pct']['min'] == 97
    assert s['after']['sclk_mhz'] == 2104.0


def _load_bench():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('kfn_bench', os.path.join(root, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench, root


def test_bench_compact_line_fits_the_drivers_reader(tmp_path, capsys):
    """BENCH_r05.json had `parsed: null`: the one stdout line had grown to 21 KB.  The driver's line is now
    `compact_line(full result)`: strict JSON, < 4 KB, carrying the contract fields + roofline + cpu_baseline, whatever the
    full result holds -- checked on the round-5 result itself (the 21 KB object) and on a multi-rank one with error
    strings and NaNs; `emit` writes the full object to the sidecar and prints the compact line LAST."""
    import argparse
    import json
    bench, root = _load_bench()
    full = json.load(open(os.path.join(root, 'profiles', 'r05_bench_driver_command.json')))
    assert len(json.dumps(full)) > 20000
    s = bench.compact_line(full)
    assert len(s) < 4096 and '\n' not in s
    d = json.loads(s, parse_constant=lambda c: (_ for _ in ()).throw(ValueError(c)))     # NaN / Infinity are not JSON
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in d, k
    assert d['value'] == full['value'] and d['steps'] == 20 and d['warmup'] == 5 and d['n_gpus'] == 1
    assert d['config']['workload'].startswith('full KFNet')
    r = d['roofline']
    assert r['kernel'] == 'wino4b_kernel' and r['bound'] == 'mfma' and r['unit'] == 'TFLOP/s'
    assert abs(r['frac'] - r['achieved'] / r['peak']) < 1e-3
    assert set(r['traffic']) >= {'fetch', 'write', 'algorithmic'} and r['traffic']['fetch'] > 1e9
    c = d['cpu_baseline']
    assert c['kind'] == 'port' and c['cores'] >= 1 and c['value'] > 0 and c['deduplicated_value'] > 0 and len(c['sample']) <= 140
    assert d['value_streamed'] == full['host_streamed']['value']
    assert d['parity']['coord_max_abs'] < 1e-4 and d['parity']['conf_max_rel'] < 1e-4
    assert set(d['roofline_kalman']) >= {'T64', 'T256', 'fuse'}
    assert d['config5']['value'] > 0 and 0 < d['config5']['frac'] < 1 and d['config2_ms'] > 0
    assert not any(isinstance(v, str) and len(v) > 200 for v in d.values())          # no prose
    # a hostile multi-rank result: long error strings, NaN, numpy scalars
    import numpy as np
    bad = dict(full, n_gpus=8, state_link='rccl', dist_backend='nccl', rccl_ranks=[[i, 8] for i in range(8)],
               handoff={'error': 'RuntimeError: ' + 'x' * 5000}, sharding_cyclic={'value': np.float32(1.5), 'block': 32, 'tail_ms': float('nan')},
               config4_2048_frames={'value': 5000.0, 'ms_per_step': 0.2, 'note': 'y' * 9000},
               multi_rank_extras='TIMED OUT ' + 'z' * 3000, data='d' * 4000, dtype='t' * 4000)
    args = argparse.Namespace(detail=str(tmp_path / 'sub' / 'detail.json'))
    print('an earlier line')
    bench.emit(bad, args)
    lines = capsys.readouterr().out.strip().split('\n')
    assert len(lines[-1]) < 4096
    d2 = json.loads(lines[-1], parse_constant=lambda c: (_ for _ in ()).throw(ValueError(c)))
    assert d2['n_gpus'] == 8 and d2['sharding_cyclic'].get('tail_ms') is None and len(d2['handoff']['error']) <= 160
    side = json.load(open(args.detail))
    assert side['handoff']['error'].endswith('x' * 100) and side['sharding_cyclic']['tail_ms'] is None
    assert d2['detail_file'].endswith('detail.json')
    # one entry point, called once (a duplicated `if __name__ == '__main__'` block ran the whole bench twice and printed two lines)
    src = open(os.path.join(root, 'bench.py')).read()
    assert src.count("__name__ == '__main__'") == 1 and src.rstrip().endswith('main()')


def test_bench_dump_outputs_and_plain_run_defaults(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float32 records, all of them under the size cap; past it a seeded frame sample that holds the
    last frame, the same on every run, with its indices.  A plain run times exactly --steps steps and writes no sidecar;
    --full writes one and keeps the 2 s side measurements; the seeded frames are those of synthetic_sequence."""
    import sys
    import torch
    from kfnet_amd.synth import synthetic_sequence
    bench, _ = _load_bench()
    rec = torch.arange(40 * 6 * 8 * 4, dtype=torch.float32).reshape(40, 6, 8, 4)
    bench.dump_outputs(str(tmp_path / 'all'), rec, 0, 1)
    assert os.listdir(tmp_path / 'all') == ['records.npy']
    got = np.load(tmp_path / 'all' / 'records.npy')
    assert got.dtype == np.float32 and np.array_equal(got, rec.numpy())
    bench.DUMP_LIMIT = 2 * 5 * (6 * 8 * 4 * 4 + 8)        # five frames per rank of two
    for d in ('s1', 's2'):
        bench.dump_outputs(str(tmp_path / d), rec, 1, 2)
    assert sorted(os.listdir(tmp_path / 's1')) == ['records_rank1.npy', 'records_rank1_frames.npy']
    idx = np.load(tmp_path / 's1' / 'records_rank1_frames.npy')
    assert idx.dtype == np.float64 and len(idx) == 5 and idx[-1] == 39 and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.load(tmp_path / 's2' / 'records_rank1_frames.npy'))
    assert np.array_equal(np.load(tmp_path / 's1' / 'records_rank1.npy'), rec.numpy()[idx.astype(int)])
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    a = bench.parse()
    assert a.headline_min_seconds == 0 and a.detail is None and not a.full and a.min_seconds == 2.0
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full'])
    a = bench.parse()
    assert a.full and a.headline_min_seconds == 0 and a.detail == bench.DEFAULT_DETAIL and a.min_seconds == 2.0
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--min-seconds', '0.5'])
    assert bench.parse().headline_min_seconds == 0.5
    for T, start in ((1, 0), (35, 4), (50, 300)):
        assert np.array_equal(bench.synthetic_frames(T, 16, 24, start), synthetic_sequence(T, 16, 24, seed=1, start=start))


def test_f43_split_k_is_chosen_for_single_frames_only():
    """BASELINE configs[1] (one 480x640 frame): SCoordNet's conv4b / conv5 / conv6 launch 160 / 80 / 40 F(4x4,3x3) workgroups on
    256 CUs -- Network.conv splits their input channels (WinogradF43ConvOp.best_k_split) so that the launch fills the chip; every
    split layer owns a private workspace (the two towers run on two streams).  At the bench batch nothing is split."""
    from kfnet_amd.cnn_wrapper.SCoordNet import SCoordNet
    from kfnet_amd.graph import Graph, WinogradF43ConvOp, WinogradS2ConvOp, variable_scope

    def build(batch):
        g = Graph()
        img = g.placeholder((batch, 480, 640, 3), 'u8', name='images')
        with variable_scope('ScoreNet'):
            net = SCoordNet({'input': img}, is_training=False, focal_x=525., focal_y=525., u=320., v=240.)
        return g, {op.name: op for op in net.ops if isinstance(op, WinogradF43ConvOp)}

    g1, f1 = build(1)
    assert {k: v.k_split for k, v in f1.items()} == {'conv1b': 1, 'conv2b': 1, 'conv3b': 1, 'conv4b': 3, 'conv5': 3, 'conv6': 6}
    for name in ('conv4b', 'conv5', 'conv6'):
        op = f1[name]
        assert op.eight_wave and op.workspace in g1.storages and op.workspace.numel * 4 >= op.workspace_bytes() > 0
        assert op.launch_workgroups() >= 240 and 'split-K' in op.kernel_name(None)
    assert len({id(f1[n].workspace) for n in ('conv4b', 'conv5', 'conv6')}) == 3
    assert f1['conv2b'].workspace is None
    g32, f32 = build(32)
    assert set(f32) == set(f1) and all(v.k_split == 1 and v.workspace is None for v in f32.values())
    # the stride-2 layers: conv4a at batch 1 is 320 workgroups = two rounds, the second a quarter full -> 4 runs (1280 = 5 rounds)
    s1 = {op.name: op for op in g1.ops if isinstance(op, WinogradS2ConvOp)}
    assert {k: v.k_split for k, v in s1.items()} == {'conv2a': 1, 'conv3a': 1, 'conv4a': 4}
    assert s1['conv4a'].workspace in g1.storages and s1['conv4a'].launch_workgroups() == 1280 if hasattr(s1['conv4a'], 'launch_workgroups') \
        else s1['conv4a'].workgroups() == 1280
    assert all(op.k_split == 1 for op in g32.ops if isinstance(op, WinogradS2ConvOp))
    # the switch: Graph.winograd_f43_max_k_split = 1 restores round 4's routing (conv5 / conv6 on the F(2x2,3x3) kernel at batch 1)
    g = Graph()
    g.winograd_f43_max_k_split = 1
    img = g.placeholder((1, 480, 640, 3), 'u8', name='images')
    with variable_scope('ScoreNet'):
        net = SCoordNet({'input': img}, is_training=False, focal_x=525., focal_y=525., u=320., v=240.)
    kinds = {op.name: type(op).__name__ for op in net.ops}
    assert kinds['conv4b'] == 'WinogradF43ConvOp' and kinds['conv5'] == 'WinogradFusedConvOp' and kinds['conv6'] == 'WinogradFusedConvOp'
    # the cost model itself: never an empty last run, never a split when the launch already fills the chip
    assert WinogradF43ConvOp.best_k_split(320, 512, 1 << 20) == 1 and WinogradF43ConvOp.best_k_split(40, 16, 1 << 20) == 1
    for wg in (10, 40, 80, 160, 250):
        for cin in (32, 64, 512, 1024):
            ks = WinogradF43ConvOp.best_k_split(wg, cin, 10 << 20)
            n_super = cin // 16
            assert 1 <= ks <= max(1, n_super) and (ks == 1 or (ks - 1) * (-(-n_super // ks)) < n_super)
