"""Case table of the launch-branch tests (tests/test_gpu_branches.py; checked on the host by tests/test_branches_host.py).

The host launchers pick a kernel instantiation from the shape, and the descriptors admit more shapes than KFNet runs.  This
table names one case per branch that the op-level suite (tests/test_gpu_ops.py) never launches:

  * the Kalman scan's five forms (kfn_kalman_scan_plan; csrc/kfn_kalman.hip scan_plan), each at both ends of its H*W range,
    each with and without the optional outputs (two different instantiations);
  * the direct convolution at kernel sizes other than 1x1 and 3x3 (kfn_conv_desc promises kh*kw <= 32): even kernels (SAME
    padding is asymmetric), rectangular ones, and the two that fill the 32-bit tap mask, 1x32 and 32x1;
  * the first convolution's head widths other than 64(+16);
  * window and pad parameters other than 8 and 2.

Nothing below touches the GPU."""
import collections

import numpy as np

# ---- Kalman scan ---------------------------------------------------------------------------------------------------------
# H*W limits of forms 1..4 (include/kfnet_hip.h, kfn_kalman_scan_plan); form 5 is everything above the last
SCAN_LIMITS = (5120, 6144, 8192, 10240)
SCAN_S, SCAN_T, SCAN_T0, SCAN_RESET = 2, 3, 1, 2      # frames 1, 2, 3: a recursion, a reset, a recursion; odd T: form 5 copies back
NIS_GATE = 7.815                                      # KFNet/eval.py --NIS
GATE_BAND = 1e-5                                      # relative distance of a pixel's NIS sum from the gate inside which its record is not compared
GATE_BAND_MAX_FRACTION = 1e-3                         # ... and the share of pixels the reference may put there

ScanCase = collections.namedtuple('ScanCase', 'form H W role use_transform nis_gate seed')
# role: 'low' = first grid of the form (one pixel above the previous form's limit, or the smallest admitted grid), 'high' = the
# form's limit itself, 'interior' = neither.  The transform is on in half the cases; the gate on the two interior grids.
SCAN_CASES = (
    ScanCase(1, 2, 2, 'low', False, 0.0, 101),
    ScanCase(1, 64, 80, 'high', True, 0.0, 102),
    ScanCase(2, 3, 1707, 'low', True, 0.0, 103),
    ScanCase(2, 72, 80, 'interior', False, NIS_GATE, 104),
    ScanCase(2, 64, 96, 'high', False, 0.0, 105),
    ScanCase(3, 5, 1229, 'low', True, 0.0, 106),
    ScanCase(3, 64, 128, 'high', False, 0.0, 107),
    ScanCase(4, 3, 2731, 'low', False, 0.0, 108),
    ScanCase(4, 80, 120, 'interior', True, NIS_GATE, 109),
    ScanCase(4, 80, 128, 'high', True, 0.0, 110),
    ScanCase(5, 7, 1463, 'low', False, 0.0, 111),
)
# (threads, pixels per thread) of the production instantiation and of the one with the optional outputs, per form
SCAN_MAPPING = {1: ((1024, 5), (768, 7)), 2: ((1024, 6), (512, 12)), 3: ((1024, 8), (512, 16)), 4: ((1024, 10), (512, 20)),
                5: ((256, 1), (256, 1))}


def scan_id(c):
    return 'form%d-%dx%d' % (c.form, c.H, c.W)


def scan_inputs(c):
    """Inputs of one scan case, drawn as tests/test_gpu_ops.py::test_kalman_scan_vs_oracle draws them (a row of the flow pushed
    out of range included): flow [S,T,H,W,2], sigma_trans [S,T,H,W,1], meas [S,T,H,W,4], state0 [S,H,W,4]."""
    S, T, H, W = SCAN_S, SCAN_T, c.H, c.W
    rng = np.random.default_rng(c.seed)
    flow = (rng.normal(size=(S, T, H, W, 2)) * 2.0).astype(np.float32)
    flow[:, :, 0, :, :] = -3.0  # push a row out of range
    sig = np.abs(rng.normal(size=(S, T, H, W, 1)) * 0.05).astype(np.float32)
    meas = rng.normal(size=(S, T, H, W, 4)).astype(np.float32)
    meas[..., 3] = np.abs(meas[..., 3]) * 0.3 + 0.05
    state0 = rng.normal(size=(S, H, W, 4)).astype(np.float32)
    state0[..., 3] = np.abs(state0[..., 3]) * 0.3 + 0.05
    return flow, sig, meas, state0


def gate_band(ref_nis, gate):
    """[S,T,H,W] bool from the REFERENCE's NIS maps alone: pixels whose NIS sum (added in the scan's order) lies within a relative
    GATE_BAND of the gate, where a last-bit difference may flip which of (measurement, filtered) the record carries."""
    s = (ref_nis[..., 0] + ref_nis[..., 1]) + ref_nis[..., 2]
    return np.abs(s.astype(np.float64) - gate) <= GATE_BAND * gate


# ---- direct convolution --------------------------------------------------------------------------------------------------
CONV_KERNELS = ((2, 2), (4, 4), (5, 5), (1, 3), (3, 1), (2, 7), (4, 8), (1, 32), (32, 1))
CONV_IMAGES = ((2, 7, 41), (1, 12, 40))          # W >= 40: a 1x32 kernel has pixels with all 32 taps live and pixels at both borders
CONV_CHANNELS = ((16, 20), (48, 64))             # (Cin, Cout)
ConvCase = collections.namedtuple('ConvCase', 'kh kw stride img cin cout mode')
# mode: 'f32' fp32 operands, 'f16' KFN_OPERAND_F16, 'x3' KFN_OPERAND_F16X3, 'act16' fp16 activations in and out
CONV_F32_CASES = tuple(ConvCase(kh, kw, s, img, ci, co, 'f32') for (kh, kw) in CONV_KERNELS for s in (1, 2) for img in CONV_IMAGES
                       for (ci, co) in CONV_CHANNELS)
MODE_KERNELS = ((5, 5), (2, 2), (1, 32))
CONV_MODE_CASES = tuple(ConvCase(kh, kw, 1, CONV_IMAGES[0], ci, co, mode) for (kh, kw) in MODE_KERNELS
                        for mode, ci, co in (('f16', 32, 48), ('x3', 32, 48), ('act16', 64, 64)))
SELECTOR_KERNELS = ((1, 32), (4, 8))             # one tap 1, all others 0, every tap in turn
DECONV_REFUSED = ((2, 2), (4, 4), (5, 5))        # transposed convolutions are 3x3 only: these sizes are refused (KFN_ERR_ARG)


def conv_id(c):
    return '%dx%d-s%d-%s-%dto%d-%s' % (c.kh, c.kw, c.stride, 'x'.join(map(str, c.img)), c.cin, c.cout, c.mode)


def conv_seed(c):
    return (c.kh * 33 + c.kw) * 1000 + c.stride * 100 + c.img[1] * 7 + c.cin      # no hash(): the same draw in every process


def shifted_input(x, kh, kw, ky, kx, stride=1):
    """What a SAME convolution whose kernel is 1 at tap (ky, kx) (input channel c -> output channel c) and 0 elsewhere returns:
    y[n, oy, ox] = x[n, oy*stride + ky - pad_top, ox*stride + kx - pad_left], 0 outside.  Pure indexing: exact."""
    from oracle.kfnet_oracle import same_pad
    n, h, w, c = x.shape
    ho, pt, _ = same_pad(h, kh, stride)
    wo, pl, _ = same_pad(w, kw, stride)
    y = np.zeros((n, ho, wo, c), x.dtype)
    for oy in range(ho):
        iy = oy * stride + ky - pt
        if not 0 <= iy < h:
            continue
        for ox in range(wo):
            ix = ox * stride + kx - pl
            if 0 <= ix < w:
                y[:, oy, ox] = x[:, iy, ix]
    return y


# ---- first convolution, windows, pads ------------------------------------------------------------------------------------
FIRST_WIDTHS = ((16, 0), (32, 0), (16, 64), (32, 16))      # (C1, C2) instantiated beside 64(+16)
FIRST_IMAGES = ((9, 70), (5, 4))
WINDOWS = (2, 4, 6, 12, 16)
PADS = (0, 1, 3)
