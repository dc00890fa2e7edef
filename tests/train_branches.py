"""Case table of the training side's launch-branch tests (tests/test_gpu_train_branches.py; checked on the host by
tests/test_train_branches_host.py), after tests/branches.py for the forward launchers.

kfn_conv2d_grad_weights promises "Cin % 16 == 0, any Cout >= 1", 3x3 or 1x1, stride 1 or 2, `db` optional, and the first
convolution's gradient C1 = 16, 32, 48 or 64; the op-level tests launch what SCoordNet's and OFlowNet's layers need.  This table
names one case per branch of wgrad_plan (kfnet_amd/csrc/kfn_train.hip, reported by kfn_conv2d_grad_weights_plan) and of the
kernels' guards that those tests never take:

  * several runs of pixels whose last stage is ragged (fp32: every tested case with splits > 1 ends on a full stage);
  * the two-tile instantiation (Cout > 64) with a ragged channel edge, and with a second n tile that is partly empty;
  * the mixed dZ quad: float4 loads (ldz % 4 == 0) with Cout % 4 != 0, where the last quad falls back to scalar loads;
  * fp16 operands at Cin 32 and 96 and Cout 32, 96, 160 and 192 (tested so far: Cin in {64, 256, 512, 1024}, Cout in {64 .. 1024});
  * 1x1 at stride 2, db == NULL, images one pixel wide, the smallest admitted call;
  * the first convolution's gradient at C1 < 64 and with a ragged 64-pixel block in a chunk other than the first;
  * the second pass of every grid-stride loop of the training launches (grids cap at 8192 / 16384 blocks).

The references are restated here in numpy: an accumulation that is exact on small integers, and pure indexing for impulses.
Nothing below touches the GPU."""
import collections

import numpy as np

F32, F16 = 0, 1                     # kfn_conv_desc.operand_dtype
STAGE = {F32: 16, F16: 32}          # pixels per stage (kfn_train_shared.h WG_BP, WG_BP_F16)
WG_BM = 128                         # k rows per workgroup tile

Plan = collections.namedtuple('Plan', 'tn tiles_m tiles_n splits chunk last')     # last = pixels of the last run
WgradCase = collections.namedtuple('WgradCase', 'name N H W cin cout k stride ldx_pad ldz plans role')
# plans: {operand type: Plan}, the operand types a case runs with being its keys
WGRAD_CASES = (
    WgradCase('W1', 3, 20, 27, 48, 70, 3, 1, 16, 72, {F32: Plan(2, 4, 1, 3, 544, 532)},
              'ragged TN=2 tile, mixed quad at column 68, taps straddling k tiles (128 % 48 != 0), stages straddling images, '
              'several runs with a ragged last stage'),
    WgradCase('W2', 2, 23, 29, 16, 130, 3, 2, 0, 131, {F32: Plan(2, 2, 2, 1, 368, 360)},
              'second n tile with 2 live columns, all-scalar dZ (ldz % 4 != 0), odd sizes at stride 2'),
    WgradCase('W3', 5, 11, 21, 80, 6, 1, 2, 4, 8, {F32: Plan(1, 1, 1, 1, 336, 330)},
              '1x1 at stride 2, bias row at 80, mixed quad in TN=1'),
    WgradCase('W4', 1, 33, 47, 32, 192, 3, 1, 0, 196, {F32: Plan(2, 3, 2, 3, 528, 495), F16: Plan(2, 3, 2, 3, 544, 463)},
              'half-empty second n tile, several runs with a ragged last stage; fp16 at Cin 32, Cout 192'),
    WgradCase('W5', 3, 19, 30, 16, 100, 1, 1, 16, 104, {F32: Plan(2, 1, 1, 3, 576, 558)},
              'a single k tile holding the taps and the bias row, several runs'),
    WgradCase('W6', 1, 32, 48, 96, 96, 3, 1, 0, 96, {F32: Plan(2, 7, 1, 3, 512, 512), F16: Plan(2, 7, 1, 3, 512, 512)},
              'Cin = Cout = 96 (ragged TN=2 tile), several flush runs'),
    WgradCase('W7', 4, 17, 19, 128, 32, 3, 1, 4, 36, {F32: Plan(1, 10, 1, 2, 656, 636), F16: Plan(1, 10, 1, 2, 672, 620)},
              'bias row alone in its k tile (Ktot % 128 == 0), Cout 32: a half-empty 64-column tile'),
    WgradCase('W8', 2, 24, 40, 32, 160, 3, 2, 16, 164, {F32: Plan(2, 3, 2, 1, 480, 480), F16: Plan(2, 3, 2, 1, 480, 480)},
              'even sizes at stride 2 (pads 0), second n tile a quarter full'),
    WgradCase('W9', 1, 1, 1, 16, 1, 3, 1, 0, 1, {F32: Plan(1, 2, 1, 1, 16, 1)},
              'the smallest admitted call: one pixel, every tap but the centre in the padding'),
    WgradCase('W10', 2, 37, 1, 64, 64, 3, 2, 0, 68, {F32: Plan(1, 5, 1, 1, 48, 38), F16: Plan(1, 5, 1, 1, 64, 38)},
              'an image one pixel wide; fp16: one ragged run in TN=1'),
    # the cells of {TN} x {runs} x {last stage} that the ten cases above leave empty (the host test asserts all eight, per type)
    WgradCase('W11', 1, 16, 16, 32, 64, 3, 1, 0, 64, {F32: Plan(1, 3, 1, 1, 256, 256), F16: Plan(1, 3, 1, 1, 256, 256)},
              'TN=1, one run, last stage full'),
    WgradCase('W12', 2, 16, 32, 32, 64, 1, 1, 0, 64, {F32: Plan(1, 1, 1, 2, 512, 512), F16: Plan(1, 1, 1, 2, 512, 512)},
              'TN=1, several runs, last stage full; the run seam is the image seam'),
    WgradCase('W13', 1, 13, 17, 32, 96, 3, 1, 4, 96, {F32: Plan(2, 3, 1, 1, 224, 221), F16: Plan(2, 3, 1, 1, 224, 221)},
              'fp16: TN=2, one ragged run'),
)
WGRAD_NO_BIAS = ('W1', 'W3', 'W9')            # run once more with db == NULL
WGRAD_RELAUNCH = ('W1', 'W4')                 # two fp32 launches, bit-identical
# 1x1, Cin 2048, Cout 1025 on 40 pixels: 2049 * 1025 = 2.1 M results, past wgrad_reduce_kernel's 8192 x 256 grid
REDUCE_CASE = WgradCase('reduce', 1, 5, 8, 2048, 1025, 1, 1, 0, 1028, {F32: Plan(2, 17, 9, 1, 48, 40)},
                        'the reduce kernel takes a second pass; mixed quad at column 1024')
GRID_8192 = 8192 * 256                        # relu_grad / pack_weights / wgrad_reduce: elements of one pass
GRID_16384 = 16384 * 256                      # adam_step / adam_guarded / scale / unscale_check

FIRST_IMAGES = ((3, 27, 31), (1, 1, 2049), (2, 9, 13))
FIRST_WIDTHS = (16, 32, 48, 64)
FC_CHUNK, FC_SUB = 2048, 64                   # first_wgrad_kernel: pixels per workgroup, per LDS block

PACK_BIG = (3, 3, 512, 512)                   # 2.36 M elements: pack_weights_kernel's second pass
PACK_RAGGED = ((3, 3, 48, 70), (1, 1, 16, 1))
INPUT_GRAD_RAGGED = ((3, 48, 70), (1, 16, 6))         # (k, Cin, Cout) on 9x13 images, stride 1
EVEN_KERNELS = ((2, 2), (4, 4), (2, 3), (3, 4))       # KFN_PACK_INPUT_GRAD_S1 refuses them


def wgrad_id(c):
    return '%s-%dx%dx%d-%dto%d-k%ds%d' % (c.name, c.N, c.H, c.W, c.cin, c.cout, c.k, c.stride)


def same_pad(size, k, stride):
    out = -(-size // stride)
    total = max((out - 1) * stride + k - size, 0)
    return out, total // 2


def out_pixels(c):
    return c.N * same_pad(c.H, c.k, c.stride)[0] * same_pad(c.W, c.k, c.stride)[0]


def wgrad_ref(x, dz, k, stride):
    """dw [k,k,ci,co] and db [co] of the SAME convolution, accumulated in fp64 tap by tap.  On small integers every sum is an
    integer far below 2^53: exact."""
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    n, h, w, ci = x.shape
    (ho, pt), (wo, pl) = same_pad(h, k, stride), same_pad(w, k, stride)
    assert dz.shape[:3] == (n, ho, wo)
    xp = np.zeros((n, pt + h + k, pl + w + k, ci))          # SAME pads at most k - 1 pixels behind
    xp[:, pt:pt + h, pl:pl + w] = x
    z2 = dz.reshape(-1, dz.shape[3])
    dw = np.zeros((k, k, ci, dz.shape[3]))
    for a in range(k):
        for b in range(k):
            xs = xp[:, a:a + (ho - 1) * stride + 1:stride, b:b + (wo - 1) * stride + 1:stride]
            dw[a, b] = xs.reshape(-1, ci).T.dot(z2)
    return dw, z2.sum(0)


def integer_operands(rng, c):
    """x in {0..3}, dz in {-2..2}: exact halfs, every partial sum an integer below 6 * pixels < 2^24."""
    ho, wo = same_pad(c.H, c.k, c.stride)[0], same_pad(c.W, c.k, c.stride)[0]
    x = rng.integers(0, 4, size=(c.N, c.H, c.W, c.cin)).astype(np.float32)
    dz = rng.integers(-2, 3, size=(c.N, ho, wo, c.cout)).astype(np.float32)
    return x, dz


def seam_pixels(P, chunk, per_image, stage=None):
    """The output pixels an impulse is put on: both ends of the first two runs, the last pixel, both sides of the first image
    seam and (given `stage`) of the first stage seam -- those that exist, each once."""
    want = (0, chunk - 1, chunk, 2 * chunk - 1, P - 1, per_image - 1, per_image) + ((stage - 1, stage) if stage else ())
    return sorted({p for p in want if 0 <= p < P})


def impulse_dz(c, pixels):
    """dz [N,Ho,Wo,Cout] with a single 1.0 per output channel, channel co on pixels[co % len(pixels)]."""
    ho, wo = same_pad(c.H, c.k, c.stride)[0], same_pad(c.W, c.k, c.stride)[0]
    dz = np.zeros((c.N * ho * wo, c.cout), np.float32)
    for co in range(c.cout):
        dz[pixels[co % len(pixels)], co] = 1.0
    return dz.reshape(c.N, ho, wo, c.cout)


def impulse_wgrad_ref(x, c, pixels):
    """What impulse_dz makes of dw: dw[a][b][ci][co] = x[n, oy*s + a - pad_t, ox*s + b - pad_l, ci] at channel co's pixel, 0 in
    the padding.  Pure indexing, in x's own dtype."""
    (ho, pt), (wo, pl) = same_pad(c.H, c.k, c.stride), same_pad(c.W, c.k, c.stride)
    dw = np.zeros((c.k, c.k, c.cin, c.cout), x.dtype)
    for co in range(c.cout):
        p = pixels[co % len(pixels)]
        n, rem = divmod(p, ho * wo)
        oy, ox = divmod(rem, wo)
        for a in range(c.k):
            for b in range(c.k):
                iy, ix = oy * c.stride + a - pt, ox * c.stride + b - pl
                if 0 <= iy < c.H and 0 <= ix < c.W:
                    dw[a, b, :, co] = x[n, iy, ix]
    return dw


def signed_floats(rng, shape):
    """Random float32 with 0.25 <= |v| < 4: no value that a half holds as a subnormal."""
    return (rng.uniform(0.25, 4.0, size=shape) * rng.choice((-1.0, 1.0), size=shape)).astype(np.float32)


# ---- first convolution ---------------------------------------------------------------------------------------------------------
def first_pixels(shape):
    """Impulse pixels of the first convolution's gradient: the corners of the first and of the last image, both sides of the chunk
    seam (2047, 2048) and of an image seam inside chunk 0 (836, 837 at 3x27x31), and the last pixel -- those that exist."""
    n, h, w = shape
    P = n * h * w
    corners = [b + o for b in (0, (n - 1) * h * w) for o in (0, w - 1, (h - 1) * w, h * w - 1)]
    return sorted({p for p in corners + [FC_CHUNK - 1, FC_CHUNK, 836, 837, P - 1] if 0 <= p < P})


def first_impulse_ref(img, C1, pixels):
    """dw [27][C1] for dz = 1.0 at pixels[c % len] of channel c: one product float32((float32(v) - 128) * 0.00625f) * 1, then
    additions of zeros."""
    n, h, w, _ = img.shape
    pre = (img.astype(np.float32) - np.float32(128.0)) * np.float32(0.00625)
    dw = np.zeros((3, 3, 3, C1), np.float32)
    for ch in range(C1):
        b, rem = divmod(pixels[ch % len(pixels)], h * w)
        y, x = divmod(rem, w)
        for a in range(3):
            for bb in range(3):
                iy, ix = y + a - 1, x + bb - 1
                if 0 <= iy < h and 0 <= ix < w:
                    dw[a, bb, :, ch] = pre[b, iy, ix]
    return dw.reshape(27, C1)


# ---- packs ---------------------------------------------------------------------------------------------------------------------
def pack_ref(w, kind):
    """include/kfnet_hip.h's layout formulas: KFN_PACK_FORWARD (0) [cout_pad][kh][kw][cin16] = w[a][b][c][r];
    KFN_PACK_INPUT_GRAD_S1 (1) [cin_pad][kh][kw][cout16] = w[kh-1-a][kw-1-b][r][c]; KFN_PACK_INPUT_GRAD_S2 (2) = w[a][b][r][c].
    Rows padded to a multiple of 32, columns to a multiple of 16, with zeros.  Returns (matrix [rows_pad,kh,kw,cols_pad], live
    mask of the same shape)."""
    kh, kw, ci, co = w.shape
    if kind == 0:
        m = w.transpose(3, 0, 1, 2)
    elif kind == 1:
        m = w[::-1, ::-1].transpose(2, 0, 1, 3)
    else:
        m = w.transpose(2, 0, 1, 3)
    rows, cols = m.shape[0], m.shape[3]
    out = np.zeros((-(-rows // 32) * 32, kh, kw, -(-cols // 16) * 16), w.dtype)
    out[:rows, :, :, :cols] = m
    live = np.zeros(out.shape, bool)
    live[:rows, :, :, :cols] = True
    return out, live
