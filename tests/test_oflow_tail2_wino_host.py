"""conv6 inside kfn_oflow_tail2 (csrc/kfn_oflow_fused.hip, fp32) runs as Winograd F(2x2,3x3) on the window's 16 tiles of 2x2
cells.  The kernel's scheme restated in numpy, in fp32 and in the kernel's order of operations, against the oracle's
convolution -- the CPU counterpart of the GPU cases in test_oflow_tail2_wino_gpu.py (and of
test_oracle_kat.py::test_polyphase_f42_stride2_identity for the stride-2 kernel)."""
from types import SimpleNamespace

import numpy as np

from oracle import kfnet_oracle as O
from tests.conv_tol import assert_close

F32 = np.float32


def bt4(d0, d1, d2, d3):
    """One axis of B^T d, B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]."""
    return d0 - d2, d1 + d2, d2 - d1, d1 - d3


def g4(g0, g1, g2):
    """One axis of G w, G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1], as the kernel rounds it: a sum, then the halving."""
    return g0, F32(0.5) * ((g0 + g2) + g1), F32(0.5) * ((g0 + g2) - g1), g2


def u_from_fragments(frag):
    """The packed conv6 fragments [108][64] (fragment tap*12 + j of lane (kq, n) = w[tap][kq*12 + j][n]) -> U[pos][j][lane],
    pos = i*4 + l: G along ky, then along kx."""
    f = frag.reshape(3, 3, 12, 64)                                  # [ky][kx][j][lane]
    t = np.stack(g4(f[0], f[1], f[2]))                              # [i][kx][j][lane]
    u = np.stack(g4(t[:, 0], t[:, 1], t[:, 2]), 1)                  # [i][l][j][lane]
    return u.reshape(16, 12, 64).astype(F32)


def conv6_f23_window(cat, frag, b6):
    """One window: cat [8,8,48] fp32 -> relu(conv6) [8,8,16], the way the kernel's lanes do it."""
    img = np.zeros((10, 10, 48), F32)                               # the LDS image with its zero border
    img[1:9, 1:9] = cat
    U = u_from_fragments(frag)
    # A operand: lane (tile m = ty*4 + tx, kq) reads the 4x4 patch at padded cell (2ty, 2tx), channels kq*12 .. kq*12 + 11
    V = np.zeros((16, 16, 48), F32)                                 # [pos][tile][channel]
    for m in range(16):
        ty, tx = m >> 2, m & 3
        d = img[2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4]               # [i][j][c]
        r = np.stack(bt4(d[0], d[1], d[2], d[3]))                   # along the patch rows
        v = np.stack(bt4(r[:, 0], r[:, 1], r[:, 2], r[:, 3]), 1)    # along its columns
        V[:, m] = v.reshape(16, 48)
    # 16 position products, 12 k-steps of 16x16x4: k index kq <-> channel kq*12 + j
    M = np.zeros((16, 16, 16), F32)                                 # [pos][tile][n]
    for pos in range(16):
        for j in range(12):
            a = V[pos][:, j::12]                                    # [tile][kq]
            bm = U[pos, j].reshape(4, 16)                           # [kq][n]
            M[pos] = (M[pos] + (a @ bm).astype(F32)).astype(F32)
    # Y = A^T M A, A^T = [1 1 1 0; 0 1 -1 -1]; tile m -> cells (2ty + a, 2tx + b)
    Mp = M.reshape(4, 4, 16, 16)                                    # [i][l][tile][n]
    tr = np.stack([(Mp[0] + Mp[1]) + Mp[2], (Mp[1] - Mp[2]) - Mp[3]])              # [a][l][tile][n]
    y = np.stack([(tr[:, 0] + tr[:, 1]) + tr[:, 2], (tr[:, 1] - tr[:, 2]) - tr[:, 3]], 1)   # [a][b][tile][n]
    out = np.zeros((8, 8, 16), F32)
    for m in range(16):
        ty, tx = m >> 2, m & 3
        out[2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = y[:, :, m]
    return np.maximum(out + b6.astype(F32), 0)


def test_f23_transforms_are_an_identity():
    """The three matrices, before any packing: A^T [(G g G^T) . (B^T d B)] A is the 2x2 correlation of a 4x4 patch."""
    rng = np.random.default_rng(3)
    d = rng.integers(-3, 4, size=(4, 4)).astype(np.float64)
    g = rng.integers(-3, 4, size=(3, 3)).astype(np.float64)
    BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
    G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
    AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)
    y = AT @ ((G @ g @ G.T) * (BT @ d @ BT.T)) @ AT.T
    ref = np.array([[np.sum(d[a:a + 3, b:b + 3] * g) for b in range(2)] for a in range(2)])
    assert np.array_equal(y, ref)


def test_oflow_tail2_conv6_f23_restatement():
    from kfnet_amd.graph import pack_oflow_tail_kernel
    rng = np.random.default_rng(57)
    P = 3
    # drawn like test_gpu_ops.py::test_oflow_tail2_vs_oracle's concat0: ReLU outputs of O(1), He-scaled weights
    cat = np.maximum(rng.normal(size=(P, 8, 8, 48)), 0).astype(F32)
    w6 = (rng.normal(size=(3, 3, 48, 16)) * np.sqrt(2.0 / (9 * 48))).astype(F32)
    b6 = (rng.normal(size=16) * 0.1).astype(F32)
    frag = pack_oflow_tail_kernel(w6)
    assert frag.shape == (108, 64) and frag.dtype == F32
    got = np.stack([conv6_f23_window(cat[p], frag, b6) for p in range(P)])
    ref = O.conv2d_same(cat.astype(np.float64), w6, b6, 1, True)
    assert_close(got, ref, cat, w6, kind='f23', label='oflow_tail2 conv6 F(2x2,3x3) restatement')
    # exactly representable data: every product and sum is exact, so is the result -- borders and tile map included
    cat_i = rng.integers(0, 4, size=(1, 8, 8, 48)).astype(F32)
    w6_i = np.zeros((3, 3, 48, 16), F32)
    ci, co = np.meshgrid(np.arange(48), np.arange(16), indexing='ij')
    tap = (5 * ci + 3 * co) % 9
    w6_i[tap // 3, tap % 3, ci, co] = 1
    b6_i = np.arange(16).astype(F32) - 8
    got_i = conv6_f23_window(cat_i[0], pack_oflow_tail_kernel(w6_i), b6_i)
    assert np.array_equal(got_i, O.conv2d_same(cat_i.astype(np.float64), w6_i, b6_i, 1, True)[0])


def test_oflow_tail2_mfma_flops():
    """The executed count: upconv0's nine 16x16x32 products as before, conv6's 16 positions of 16 tiles x 16 channels over
    K = 48 (the nominal count keeps the nine taps).  The fp16 launch keeps its nine-tap kernel."""
    from kfnet_amd.graph import OFlowTail2Op
    t = SimpleNamespace(shape=(2, 3, 5, 288))
    args = [None] * 8                                               # x5, ku, bu, k6, b6, kp, bpred, flow
    op = OFlowTail2Op(t, None, True, *args)
    P = 2 * 3 * 5
    assert op.mfma_flops() == 2.0 * P * (9 * 16 * 32 * 16 + 16 * 16 * 48 * 16)
    assert op.flops() == 2.0 * P * (16 * 9 * 32 * 16 + 64 * 9 * (48 * 16 + 16))
    assert op.flops() > op.mfma_flops()
    op16 = OFlowTail2Op(t, None, True, *args, operands_f16=True)
    assert op16.mfma_flops() == 2.0 * P * (9 * 16 * 32 * 16 + 64 * 9 * 48 * 16)
