"""Which kernel a convolution runs on: chosen when the layer is built (`choose`), and chosen again when something the
first choice rested on changes -- a head epilogue only the direct kernel carries (`direct`), an output a later concat
re-bound to a window a kernel's 16-byte stores cannot take (`after_binding`).

A `Route` only names things; ConvOp.reroute (graph.py) is what puts an op on one.  The re-choosing rules have fixed
targets: they do not run `choose` again, whose thresholds they are meant to skip.
"""
import collections

from . import _lib
from .graph import (Conv64RowsF16Op, ConvOp, WindowFcConvOp, WinogradConvOp, WinogradF43ConvOp, WinogradFusedConvOp,
                    WinogradS2ConvOp, as_f16, as_f16x3, pack_bias, pack_bias_x4, pack_conv64_rows_kernel, pack_conv_kernel,
                    pack_conv_kernel_chunked, pack_window_fc_kernel, pack_winograd_f43_kernel, pack_winograd_f43_kernel_b,
                    pack_winograd_fused_kernel, pack_winograd_kernel, pack_winograd_s2_kernel, pack_winograd_s2_kernel_b,
                    pack_winograd_s2_kernel_c, winograd_plan)

# eight_wave / k_split / f42: None = the class has no such option.  workspace: None, 'shared' (the graph's two-kernel Winograd
# workspace: those layers run one after the other) or 'private' (split-K: the two towers run on two streams, a shared one
# would race -- single frames only, 29-59 MB per split layer at batch 1)
Route = collections.namedtuple('Route', 'op_class kernel_pack bias_pack operand_dtype eight_wave k_split f42 workspace')
Route.__new__.__defaults__ = (pack_bias, _lib.OPERAND_F32, None, None, None, None)


def _direct(operand_dtype, x, y):
    if operand_dtype == _lib.OPERAND_F16:
        # fp16 activations on either side: the tap-innermost kernels with chunk-major weights
        chunked = x.dtype == 'f16' or y.dtype == 'f16'
        return Route(ConvOp, as_f16(pack_conv_kernel_chunked if chunked else pack_conv_kernel), operand_dtype=operand_dtype)
    if operand_dtype == _lib.OPERAND_F16X3:
        return Route(ConvOp, as_f16x3(pack_conv_kernel), operand_dtype=operand_dtype)
    return Route(ConvOp, pack_conv_kernel)


def direct(op):
    """The direct MFMA kernel for an existing op: same tensors, variables and operand type, the direct kernel's weight layout."""
    return _direct(op.operand_dtype, op.x, op.y)


def choose(g, x, y, k, stride, biased):
    """The route of a new k x k convolution x -> y.  Reads the graph's switches, the two tensors' geometry (shape, ld, ch_off,
    dtype) and, for the Winograd routes, the library's launch plan of the layer (graph.winograd_plan: is it taken, does its
    kernel fit this device's LDS, how many workgroups); constructs nothing."""
    n, h, w, cin = x.shape
    filters = y.shape[3]
    F16 = _lib.OPERAND_F16
    f16 = g.conv_operands == 'f16' and cin % 32 == 0
    f32_io = x.dtype == 'f32' and y.dtype == 'f32'
    # (measured, 16 frames: conv3b 2.07 vs 2.31 ms direct fp16, conv4b 1.81 vs 2.59, conv5 1.00 vs 1.25; at
    #  Cin = 256 the direct kernel is as fast -- conv2b 2.56 vs 2.48 -- and stays)
    if (f16 and f32_io and k == 3 and stride == 1 and g.winograd_fused and cin >= 512
            and winograd_plan(x, y, 1, operand_dtype=F16) is not None):
        # BASELINE config 5: the four-wave Winograd kernel on fp16 MFMAs (transform in fp32, V and U rounded to fp16)
        return Route(WinogradFusedConvOp, as_f16(pack_winograd_fused_kernel), operand_dtype=F16)
    # (the fp16 instantiation of the polyphase stride-2 kernel exists and is tested, but at fp16 MFMA rates it is
    #  latency-bound and the direct fp16 kernel is faster: conv3a 1.20 vs 1.68 ms -- Graph.winograd_s2_f16 = False)
    if (f16 and f32_io and k == 3 and stride == 2 and g.winograd_s2_f16 and cin >= 64
            and filters >= 128 and winograd_plan(x, y, 2, operand_dtype=F16) is not None):
        return Route(WinogradS2ConvOp, as_f16(pack_winograd_s2_kernel), operand_dtype=F16, eight_wave=False, k_split=1, f42=False)
    if (f16 and k == 3 and stride == 1 and h == 2 and w == 2 and g.window_fc and biased and (4 * cin) % 32 == 0
            and filters % 8 == 0 and f32_io):
        # OFlowNet's 2x2 level in the fp16-operand mode: the same dense window matrix, operands rounded to fp16
        return Route(WindowFcConvOp, as_f16(pack_window_fc_kernel), pack_bias_x4, F16)
    if (f16 and g.conv64_rows_f16 and k == 3 and stride == 1 and biased
            and Conv64RowsF16Op.supported(x, y, cin, filters)):
        # (measured, 16 frames of 540x960: 1.05 ms on the 256x64 implicit-GEMM tile, LDS-bound at 0.23 of the fp16 peak)
        return Route(Conv64RowsF16Op, pack_conv64_rows_kernel, operand_dtype=F16)
    if f16:
        return _direct(F16, x, y)
    if g.conv_operands == 'f16x3' and cin % 32 == 0 and cin >= g.f16x3_min_channels:
        return _direct(_lib.OPERAND_F16X3, x, y)
    if (k == 3 and stride == 1 and h == 2 and w == 2 and g.window_fc and biased and cin % 8 == 0 and filters % 8 == 0
            and g.conv_operands == 'f32'):
        # OFlowNet's 2x2 level: dense window matrix (16 Cin Cout products per window instead of 36)
        return Route(WindowFcConvOp, pack_window_fc_kernel, pack_bias_x4)
    f43 = g.winograd_f43_min_channels
    # (measured at batch 32, F(2x2,3x3) -> F(4x4,3x3), profiles/r04_wino4_microbench.log: conv2b 10.02 -> 6.99 ms,
    #  conv3b 9.30 -> 6.41, conv4b 9.18 -> 6.26, conv5 4.61 -> 3.28, conv6 1.24 -> 0.85, conv1b 3.66 -> 2.77, feat5 0.23 -> 0.18;
    #  with 32 output channels -- feat3 -- half of the workgroup idles: 0.31 -> 0.47, stays on wino2_kernel)
    fmin = g.winograd_fused_min_channels
    fused_ok = (k == 3 and stride == 1 and g.winograd_fused and fmin and cin >= fmin and filters >= fmin
                and cin <= g.winograd_fused_max_channels
                and min(h, w) >= 8 and winograd_plan(x, y, 1) is not None)
    # A launch of fewer than winograd_f43_min_workgroups workgroups (of 32 tiles x 64 channels, one per CU) leaves
    # most of the 256 CUs idle and the smaller F(2x2,3x3) workgroups win -- single frames only (batch 1, F(4x4) ->
    # F(2x2): conv5 80 workgroups 0.287 -> 0.238 ms, conv6 40: 0.151 -> 0.123, feat5 40: 0.031 -> 0.022; from 160
    # workgroups up F(4x4) is ahead: conv4b at batch 1 0.288 against 0.479; profiles/r04_wino4_microbench.log, r4z)
    e8 = bool(g.winograd_f43_eight_wave)
    plan = None
    if k == 3 and stride == 1 and g.winograd_fused and f43:
        plan = winograd_plan(x, y, 1, _lib.WINO_FORM_F43_EIGHT_WAVE if e8 else _lib.WINO_FORM_F43_FOUR_WAVE)
    wgs = plan.tiles_m * plan.tiles_n if plan is not None else 0
    ksplit = 1
    if plan is not None and e8 and g.winograd_f43_max_k_split > 1:
        ksplit = WinogradF43ConvOp.best_k_split(wgs, cin, n * h * w * filters * 4, g.winograd_f43_max_k_split)
    f43_fills = (not fused_ok or wgs * ksplit >= g.winograd_f43_min_workgroups)
    if plan is not None and cin >= f43 and filters >= f43 and f43_fills:
        return Route(WinogradF43ConvOp, pack_winograd_f43_kernel_b if e8 else pack_winograd_f43_kernel,
                     eight_wave=e8, k_split=ksplit, workspace='private' if ksplit > 1 else None)
    # (measured, 16-frame batch, single-kernel vs two-kernel form: conv1b 2.3 ms vs 3.3 direct, conv2b 5.60 vs
    #  7.10, conv3b 5.05 vs 5.99, conv4b 4.93 vs 5.42, conv5 2.49 vs 2.73, conv6 0.63 vs 0.77)
    if fused_ok:
        return Route(WinogradFusedConvOp, pack_winograd_fused_kernel)
    smin = g.winograd_s2_min_channels
    # 3x3 stride-2 layers (SCoordNet conv2a / conv3a / conv4a): polyphase + F(2,2), 25/36 of the direct MFMAs
    e8 = bool(g.winograd_s2_eight_wave)
    plan = None
    if k == 3 and stride == 2 and smin and cin >= smin and filters >= 128:
        plan = winograd_plan(x, y, 2, _lib.WINO_FORM_S2_EIGHT_WAVE if e8 else 0)
    if plan is not None:
        f42 = winograd_plan(x, y, 2, _lib.WINO_FORM_S2_F42) if g.winograd_s2_f42 else None
        if f42 is not None and f42.tiles_m * f42.tiles_n >= g.winograd_s2_f42_min_workgroups:
            return Route(WinogradS2ConvOp, pack_winograd_s2_kernel_c, eight_wave=False, k_split=1, f42=True)
        ksplit = 1
        if e8 and g.winograd_s2_max_k_split > 1 and filters % 4 == 0:
            ksplit = WinogradS2ConvOp.best_k_split(plan.tiles_m * plan.tiles_n, cin,
                                                   y.shape[0] * y.shape[1] * y.shape[2] * filters * 4, g.winograd_s2_max_k_split)
        return Route(WinogradS2ConvOp, pack_winograd_s2_kernel_b if e8 else pack_winograd_s2_kernel,
                     eight_wave=e8, k_split=ksplit, f42=False, workspace='private' if ksplit > 1 else None)
    wmin = g.winograd_min_channels
    if (k == 3 and stride == 1 and wmin and cin >= wmin and filters >= wmin and filters % 4 == 0
            and min(h, w) >= 8):
        return Route(WinogradConvOp, pack_winograd_kernel, workspace='shared')
    return Route(ConvOp, pack_conv_kernel)


def after_binding(op):
    """The route an op has to move to now that every concat has re-bound its producers, or None if it can stay."""
    x, y = op.x, op.y
    n, h, w, cin = x.shape
    cout = y.shape[3]
    if isinstance(op, WindowFcConvOp):
        # the window matrix needs both tensors pixel-contiguous; else the plain convolution
        return None if x.ld == cin and y.ld == cout else direct(op)
    if isinstance(op, WinogradF43ConvOp):
        # an output the F(4x4,3x3) launcher would now reject: the fused F(2x2,3x3) kernel (dword stores for unaligned
        # outputs) or the direct one
        if op.plan(required=False) is not None:
            return None
        if winograd_plan(x, y, 1) is not None and min(h, w) >= 8:
            return Route(WinogradFusedConvOp, pack_winograd_fused_kernel)
        return direct(op)
    if isinstance(op, WinogradS2ConvOp):
        # the F(4,2) form and the split-K form store 16 bytes at a time; the F(2,2) eight-wave form has a dword-store path
        if op.f42 and op.plan(required=False) is None:
            return Route(WinogradS2ConvOp, pack_winograd_s2_kernel_b, eight_wave=True, k_split=1, f42=False)
        if op.k_split > 1 and op.plan(required=False) is None:
            #  kfn_conv2d_winograd_s2_splitk needs a 16-byte aligned output with ldy % 4 == 0: same kernel, same
            # weights, unsplit
            return Route(WinogradS2ConvOp, op.kernel.pack, op.bias.pack if op.bias is not None else pack_bias,
                         op.operand_dtype, eight_wave=op.eight_wave, k_split=1, f42=False)
    return None
