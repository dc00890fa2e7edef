"""Helpers for the -m gpu tests: device buffers via torch, calls via the ctypes C ABI."""
import ctypes as C

import numpy as np

from kfnet_amd import _lib
from kfnet_amd.graph import pack_conv_kernel, pack_conv_kernel_chunked, pack_deconv_kernel


def dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def sync():
    import torch
    torch.cuda.synchronize()


def run_conv(x, w, b, stride=1, relu=False, transposed=False, epilogue=0, config=0, ldx=None, ldy=None,
             x_off=0, y_off=0, f16=False, x3=False, x16=False, y16=False, k_step=0, weights_path=0):
    """x [N,H,W,Cin] np fp32; w TF layout; returns y np [N,Ho,Wo,Cout] computed by the HIP library.
    ldx/ldy > C exercise the strided-view paths (input/output living in wider buffers)."""
    import torch
    lib = _lib.load()
    n, h, wd, cin = x.shape
    if transposed:
        kh, kw, cout, _ = w.shape
        ho, wo = h * stride, wd * stride
        wp = pack_deconv_kernel(w)
    else:
        kh, kw, _, cout = w.shape
        ho, wo = -(-h // stride), -(-wd // stride)
        wp = pack_conv_kernel(w)
    ldx = ldx or cin
    ldy = ldy or cout
    # x16 / y16: the activation tensors hold IEEE halfs in memory (kfn_conv_desc.x_dtype / y_dtype)
    xb = np.full((n * h * wd, ldx), 7.0, dtype=np.float16 if x16 else np.float32)
    xb[:, x_off:x_off + cin] = x.reshape(-1, cin)
    xd = dev(xb)
    GUARD = 96   # rows behind the tensor: the last (partial) tile must not write past row M
    yd = torch.full((n * ho * wo + GUARD, ldy), -123.0, dtype=torch.float16 if y16 else torch.float32, device='cuda')
    xsz, ysz = (2 if x16 else 4), (2 if y16 else 4)
    if x3:
        m = wp * np.float32(1024.0)
        hi = m.astype(np.float16)
        wp_dev = np.stack([hi, (m - hi.astype(np.float32)).astype(np.float16)])
    else:
        wp_dev = wp.astype(np.float16) if f16 else wp
        if x16 or y16:      # fp16 activations: chunk-major weights
            wp_dev = pack_conv_kernel_chunked(w).astype(np.float16)
    wd_ = dev(wp_dev)
    bd = dev(b.astype(np.float32)) if b is not None else None
    d = _lib.ConvDesc(N=n, H=h, W=wd, Cin=cin, ldx=ldx, Cout=cout, cout_pad=wp.shape[0], ldy=ldy, kh=kh, kw=kw,
                      stride=stride, transposed=int(transposed), relu=int(relu), epilogue=epilogue, config=config,
                      operand_dtype=2 if x3 else int(f16), x_dtype=int(x16), y_dtype=int(y16), k_step=k_step, weights_path=weights_path)
    rc = lib.kfn_conv2d_nhwc(C.byref(d), xd.data_ptr() + xsz * x_off, wd_.data_ptr(),
                             bd.data_ptr() if bd is not None else None, yd.data_ptr() + ysz * y_off, stream())
    _lib.check(rc, 'kfn_conv2d_nhwc')
    sync()
    yh = yd.cpu().numpy().astype(np.float32)
    assert np.all(yh[n * ho * wo:] == -123.0), 'conv wrote past the last output row'
    yh = yh[:n * ho * wo]
    out = yh[:, y_off:y_off + cout].reshape(n, ho, wo, cout)
    # untouched columns must keep the sentinel
    mask = np.ones(ldy, dtype=bool)
    mask[y_off:y_off + cout] = False
    assert np.all(yh[:, mask] == -123.0), 'conv wrote outside its channel window'
    return out


def winograd_fields(kind, x_shape, co, relu=False, form=0, ldx_pad=0, ldy_pad=8, config=0, x_layout='nhwc', y_layout='nhwc',
                    order=0, x_off=0, y_off=0, f16=False):
    """The descriptor fields of a run_winograd launch (same arguments) and where the two windows start, in floats: (fields,
    x_off, y_off).  No device access: tests/test_wino_modes_host.py asks the library for the launch plan of the same fields."""
    n, h, w, ci = x_shape
    stride = 2 if kind == 's2' else 1
    if x_layout == 'c16':
        ldx_pad = x_off = 0
    if y_layout == 'c16':
        ldy_pad = y_off = 0
    assert 0 <= x_off <= ldx_pad and 0 <= y_off <= ldy_pad
    fields = dict(N=n, H=h, W=w, Cin=ci, ldx=ci + ldx_pad, Cout=co, cout_pad=-(-co // 32) * 32, ldy=co + ldy_pad, kh=3, kw=3,
                  stride=stride, relu=int(relu), wino_form=form, config=config, wino_order=order, operand_dtype=int(f16),
                  x_layout=_lib.LAYOUT_C16 if x_layout == 'c16' else 0, y_layout=_lib.LAYOUT_C16 if y_layout == 'c16' else 0)
    return fields, x_off, y_off


def run_winograd(kind, x, wt, b, relu=False, form=0, ldx_pad=0, ldy_pad=8, config=0, x_layout='nhwc', y_layout='nhwc',
                 order=0, x_off=0, y_off=0, x_fill=9.0, f16=False, k_split=None, relaunch=None):
    """One launch of a minimal-filtering entry point on x [N,H,W,Cin] fp32 with the TF-layout 3x3 kernel wt:
      kind 'wino'  kfn_conv2d_winograd        (two kernels + workspace; F(2x2,3x3))
           'fused' kfn_conv2d_winograd_fused  (form 0 = the library's routing, 1 = KFN_WINO_FORM_ONE_WAVE)
           'f43'   kfn_conv2d_winograd_f43    (form 2 = four waves, 3 = eight waves)
           's2'    kfn_conv2d_winograd_s2     (stride 2; form 0 = four waves, 4 = eight waves, 5 = the F(4,2) form)
    Input and output live in wider buffers (ldx = Cin + ldx_pad filled with x_fill outside the window, which starts x_off floats
    in; ldy = Cout + ldy_pad, the window y_off floats in); guard rows behind the output and the columns before and behind the
    window must come back untouched.  x_layout / y_layout 'c16': that tensor is handed
    over / comes back channel-blocked (KFN_LAYOUT_C16, per image [C/16][H][W][16]; dense, so its pad is dropped); the conversion
    from / to NHWC happens here on the host.  order: kfn_conv_desc.wino_order.  f16: operand_dtype = KFN_OPERAND_F16 with the
    packed kernel stored as halfs ('fused', and 's2' form 0).  k_split: through the split-K entry point of 'f43' (form 3) / 's2'
    (form 4) with a workspace of its own, whose guard behind the planes must come back untouched.  relaunch: a sequence of
    dicts of descriptor fields; each is one more launch on the same device buffers (y refilled with its sentinel) with those
    fields changed, and the return value becomes the list of all results.  Returns y [N,Ho,Wo,Cout] np fp32."""
    import torch
    from kfnet_amd.graph import (as_f16, pack_winograd_f43_kernel, pack_winograd_f43_kernel_b, pack_winograd_fused_kernel,
                                 pack_winograd_kernel, pack_winograd_s2_kernel, pack_winograd_s2_kernel_b, pack_winograd_s2_kernel_c)
    lib = _lib.load()
    n, h, w, ci = x.shape
    co = wt.shape[3]
    fields, x_off, y_off = winograd_fields(kind, x.shape, co, relu, form, ldx_pad, ldy_pad, config, x_layout, y_layout, order,
                                           x_off, y_off, f16)
    ldx, ldy, stride = fields['ldx'], fields['ldy'], fields['stride']
    ho, wo = -(-h // stride), -(-w // stride)
    if x_layout == 'c16':
        xb = np.ascontiguousarray(x.reshape(n, h, w, ci // 16, 16).transpose(0, 3, 1, 2, 4)).reshape(n * h * w, ci)
    else:
        xb = np.full((n * h * w, ldx), x_fill, dtype=np.float32)
        xb[:, x_off:x_off + ci] = x.reshape(-1, ci)
    GUARD = 64
    dx = dev(xb)
    db = dev(np.concatenate([b, np.zeros((-co) % 4, np.float32)]).astype(np.float32)) if b is not None else None
    bp = db.data_ptr() if db is not None else None
    xp = dx.data_ptr() + 4 * x_off
    ws = None
    if kind == 'wino':
        assert not f16 and k_split is None
        nb = C.c_size_t()
        _lib.check(lib.kfn_winograd_workspace_bytes(C.byref(_lib.ConvDesc(**fields)), C.byref(nb)), 'ws')
        ws = torch.empty((nb.value // 4 + 64,), device='cuda')
        du = dev(pack_winograd_kernel(wt))
        call = lambda d, yp: lib.kfn_conv2d_winograd(C.byref(d), xp, du.data_ptr(), bp, yp, ws.data_ptr(), 3, stream())
    elif kind == 'fused':
        assert k_split is None
        du = dev((as_f16(pack_winograd_fused_kernel) if f16 else pack_winograd_fused_kernel)(wt))
        call = lambda d, yp: lib.kfn_conv2d_winograd_fused(C.byref(d), xp, du.data_ptr(), bp, yp, stream())
    elif kind == 'f43':
        assert not f16
        du = dev((pack_winograd_f43_kernel_b if form == 3 else pack_winograd_f43_kernel)(wt))
        call = lambda d, yp: lib.kfn_conv2d_winograd_f43(C.byref(d), xp, du.data_ptr(), bp, yp, stream())
        split_fns = (lib.kfn_winograd_f43_splitk_workspace_bytes, lib.kfn_conv2d_winograd_f43_splitk)
    elif kind == 's2':
        assert not f16 or form == 0
        pack = {4: pack_winograd_s2_kernel_b, 5: pack_winograd_s2_kernel_c}.get(form, pack_winograd_s2_kernel)
        du = dev((as_f16(pack) if f16 else pack)(wt))
        call = lambda d, yp: lib.kfn_conv2d_winograd_s2(C.byref(d), xp, du.data_ptr(), bp, yp, stream())
        split_fns = (lib.kfn_winograd_s2_splitk_workspace_bytes, lib.kfn_conv2d_winograd_s2_splitk)
    else:
        raise ValueError(kind)
    ws_used = 0
    if k_split is not None:
        nb = C.c_size_t()
        _lib.check(split_fns[0](C.byref(_lib.ConvDesc(**fields)), k_split, C.byref(nb)), 'split-K workspace bytes')
        assert nb.value == (k_split * n * ho * wo * co * 4 if k_split > 1 else 0)
        ws_used = nb.value // 4
        ws = torch.full((ws_used + GUARD,), -7.0, device='cuda')
        call = lambda d, yp: split_fns[1](C.byref(d), xp, du.data_ptr(), bp, yp, ws.data_ptr(), k_split, stream())
    window = np.zeros(ldy, dtype=bool)
    window[y_off:y_off + co] = True
    outs = []
    for change in [{}] + list(relaunch or []):
        y = torch.full((n * ho * wo + GUARD, ldy), -5.0, device='cuda')
        _lib.check(call(_lib.ConvDesc(**dict(fields, **change)), y.data_ptr() + 4 * y_off), 'kfn_conv2d_winograd (%s)' % kind)
        sync()
        got = y.cpu().numpy()
        assert np.all(got[n * ho * wo:] == -5.0), '%s wrote past the last output pixel' % kind
        assert np.all(got[:, ~window] == -5.0), '%s wrote outside its channel window' % kind
        if k_split is not None:
            assert bool((ws[ws_used:] == -7.0).all()), '%s: the partial sums went past the workspace' % kind
        if y_layout == 'c16':
            outs.append(np.ascontiguousarray(got[:n * ho * wo].reshape(n, co // 16, ho, wo, 16).transpose(0, 2, 3, 1, 4)).reshape(n, ho, wo, co))
        else:
            outs.append(got[:n * ho * wo, y_off:y_off + co].reshape(n, ho, wo, co).copy())
    return outs if relaunch is not None else outs[0]
