"""Training OFlowNet on the device: stage 2 of the reference's procedure ("Train OFlowNet").

A step sees P pairs (a, b) of frames -- frames 2p and 2p + 1 of the batch -- and is a fixed list of launches of libkfnet_hip.so:

    forward   the feature tower on the 2P frames (kfn_first_conv_u8, kfn_conv2d_nhwc; feat7 once plain, for the backward pass,
              and once with the L2-norm epilogue), kfn_cost_volume, the window U-Net (kfn_conv2d_nhwc, the three transposed
              layers with transposed = 1; concatenations are channel windows of one buffer), kfn_flow_softargmax with the
              probabilities kept, the dense head as 1x1 convolutions with the exp 1e-2 epilogue
    loss      kfn_flow_loss_grad: label a warped by the flow against label b, d_flow and d_sigma
    backward  kfn_flow_head_backward, then per layer, last to first: kfn_conv2d_grad_weights, the input gradient on the
              forward kernel with the pack kfn_pack_conv_weights made for it, kfn_relu_grad; the outputs that feed two
              consumers get the second gradient added before their ReLU mask; kfn_cost_volume_backward,
              kfn_l2norm_backward, the tower, kfn_first_conv_u8_grad_weights
    update    kfn_adam_step on the flat buffer of every Temporal/* variable, then the packs of the new weights

A transposed layer y = deconv(x, w[k,k,Cout,Cin]) is the input gradient of the stride-2 convolution V: [2h,2w,Cout] ->
[h,w,Cin] whose HWIO kernel is w as it lies in memory.  So its forward runs on V's KFN_PACK_INPUT_GRAD_S2 pack, its input
gradient is V itself (KFN_PACK_FORWARD), and its weight gradient is V's, with the layer's output gradient as input and the
layer's input as dZ.  Its bias gradient, the pixel sum of the output gradient, is the bias row of a 1x1 weight-gradient launch.

With `frames` and `pair_index` the pairs share frames (joint stage 3, DESIGN.md 6g: a group of T frames holds T - 1 overlapping
pairs): the tower runs once per frame, f_a and f_b are gathers of its normalised output, and the backward pass writes d_fb to
the rows of the b frames and adds d_fa at the rows of the a frames.

There is no fallback: a missing entry point or an unsupported shape raises.
"""
import ctypes as C

import numpy as np

from . import _lib, staging
from .cnn_wrapper.OFlowNet import DECODER, ENCODER, FC, LOGITS
from .train_common import LazyStats, ParamStore, size_query
from .weights import variable_specs

SCOPE = 'Temporal'
TOWER = (('feat1', 1, True), ('feat2', 2, True), ('feat3', 1, True), ('feat4', 2, True), ('feat5', 1, True), ('feat6', 2, True),
         ('feat7', 1, False))                      # (name, stride, relu): KFNet/KFNet.py:318-338
WINDOW = 8


def _pad16(c):
    return -(-c // 16) * 16


def check_pair_index(pair_index, pairs, frames):
    """(a_idx, b_idx) as int64 arrays of length `pairs`: frame numbers below `frames`, no number twice within a list -- so the
    scatter of the backward pass meets every row of d_feat at most once per list and repeats bit for bit."""
    a, b = (np.asarray(x, dtype=np.int64).reshape(-1) for x in pair_index)
    for name, idx in (('a', a), ('b', b)):
        if len(idx) != pairs:
            raise ValueError('pair_index: %d %s frames for %d pairs' % (len(idx), name, pairs))
        if idx.min() < 0 or idx.max() >= frames:
            raise ValueError('pair_index: an %s frame outside 0..%d' % (name, frames - 1))
        if len(np.unique(idx)) != len(idx):
            raise ValueError('pair_index: an %s frame is listed twice' % name)
    return a, b


class View(object):
    """`C` channels of the pixels of a [rows, ld] float32 device buffer, from channel `off`: n images of h x w pixels."""

    def __init__(self, buf, off, Cc, n, h, w):
        self.buf, self.off, self.C, self.n, self.h, self.w = buf, off, Cc, n, h, w
        self.ld = buf.shape[1]

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.off

    @property
    def rows(self):
        return self.n * self.h * self.w

    def tensor(self):
        return self.buf[:, self.off:self.off + self.C]


class Layer(object):
    """One convolution of the Temporal scope: kind 'conv' | 'deconv' | 'dense', x -> y (Views), the gradient views dx, dy."""

    def __init__(self, name, kind, k, ci, co, stride, relu, epilogue=_lib.EPI_NONE):
        self.name, self.kind, self.k, self.ci, self.co, self.stride, self.relu, self.epilogue = name, kind, k, ci, co, stride, relu, epilogue


class StepStats(LazyStats):
    """loss, accuracy, pixels (sum M), lost (cells whose warp left the grid or met a masked corner), lr."""
    KEYS = ('loss', 'accuracy', 'pixels', 'lost', 'lr')

    def _decode(self, s):
        return dict(loss=float(s[0]), accuracy=float(s[1]), pixels=float(s[2]) - 1.0, lost=float(s[3]), lr=self._lr)


class OFlowNetTrainer(ParamStore):
    def __init__(self, weights, image_size=(480, 640), pairs=4, base_lr=1e-4, gamma=0.5, stepvalue=100000, weight_decay=1e-4,
                 loss_clip=None, device='cuda:0', frames=None, pair_index=None):
        """weights: {TF name: array} holding at least Temporal/*.  pairs = P: a batch is 2P frames, pair p = frames (2p, 2p + 1).
        loss_clip: None (no clip) or a float.  frames = B with pair_index = (a_idx, b_idx): a batch is B frames instead and
        pair p = frames (a_idx[p], b_idx[p]), each list without repeats; the gradients then come from the caller
        (backward(d_flow, d_sigma)), the loss of stage 2 knows the default layout only."""
        import torch
        H, Wd = image_size
        staging.check_size(H, Wd, 'the height and width of a training batch')
        if pairs < 1:
            raise ValueError('pairs must be >= 1')
        self.lib = _lib.load()
        self.image_size, self.pairs, self.grid = (H, Wd), int(pairs), (H // 8, Wd // 8)
        self.loss_clip = None if loss_clip is None else float(loss_clip)
        P, (h, w) = self.pairs, self.grid
        if (frames is None) != (pair_index is None):
            raise ValueError('frames and pair_index go together')
        self.nframes = F = 2 * P if frames is None else int(frames)
        self.pair_index = None if pair_index is None else check_pair_index(pair_index, P, F)
        self.windows = N = P * h * w

        specs = {n.split('/', 1)[1]: (kind, shape) for n, kind, shape in variable_specs() if n.startswith(SCOPE + '/')}
        # the flat parameter store: kernel then bias per variable of the scope; a transposed layer's bias has its Cout = shape[2]
        ParamStore.__init__(self, [('%s/%s/%s' % (SCOPE, name, var), shp) for name, (kind, shape) in specs.items()
                                   for var, shp in (('kernel', shape), ('bias', (shape[2] if kind == 'deconv' else shape[-1],)))],
                            device, base_lr, gamma, stepvalue, weight_decay)

        with torch.cuda.device(self.device):
            f32 = dict(dtype=torch.float32, device=self.device)
            self.set_weights(weights)
            self.frames = torch.zeros((F, H, Wd, 3), dtype=torch.uint8, device=self.device)
            if self.pair_index is not None:
                self.a_idx, self.b_idx = (torch.from_numpy(x).to(self.device) for x in self.pair_index)
            self.labels = None
            self.label_stride = 1

            def buf(rows, ld):
                return torch.zeros((rows, ld), **f32)

            # ---- the tower on the F frames (2P unless the pairs share them): every output kept, feat7 both plain and normalised
            self.layers = []
            hh, ww, ci = H, Wd, 3
            prev = None
            for name, s, relu in TOWER:
                co = specs[name][1][3]
                hh, ww = -(-hh // s), -(-ww // s)
                L = Layer(name, 'conv', 3, ci, co, s, relu)
                L.x = prev
                L.y = View(buf(F * hh * ww, co), 0, co, F, hh, ww)
                L.dy = View(buf(F * hh * ww, _pad16(co)), 0, co, F, hh, ww)
                L.dx = None if prev is None else self.layers[-1].dy
                self.layers.append(L)
                prev, ci = L.y, co
            self.tower = list(self.layers)
            assert (hh, ww) == (h, w) and ci == 32
            self.feat = buf(F * h * w, 32)                           # l2_normalize(feat7), all frames
            self.f_a, self.f_b = buf(N, 32), buf(N, 32)
            self.d_feat = buf(F * h * w, 32)
            self.d_fa, self.d_fb = buf(N, 32), buf(N, 32)
            self.vol = View(buf(N * 64, 32), 0, 32, N, WINDOW, WINDOW)
            self.d_vol = View(buf(N * 64, 32), 0, 32, N, WINDOW, WINDOW)

            # ---- the window U-Net: a concatenation is one buffer, its two producers write channel windows of it
            joins = {j[1]: (j[2], j[3]) for j in DECODER if j[0] == 'join'}
            widths = {s[1]: s[2] for s in ENCODER + DECODER if s[0] != 'join'}
            home = {}                                             # producer -> (join, channel offset)
            for j, (first, second) in joins.items():
                home[first] = (j, 0)
                home[second] = (j, widths[first])
            cur, hw = 'input', WINDOW
            views = {'input': (self.vol, self.d_vol)}
            join_bufs = {}
            for step in ENCODER + DECODER:
                kind, name = step[0], step[1]
                if kind == 'join':
                    cur = name
                    continue
                co, s = step[2], step[3]
                hw_out = hw * s if kind == 'deconv' else -(-hw // s)
                if name in home:
                    j, o = home[name]
                    if j not in join_bufs:
                        tot = widths[joins[j][0]] + widths[joins[j][1]]
                        join_bufs[j] = (buf(N * hw_out * hw_out, tot), buf(N * hw_out * hw_out, tot))
                        views[j] = (View(join_bufs[j][0], 0, tot, N, hw_out, hw_out), View(join_bufs[j][1], 0, tot, N, hw_out, hw_out))
                    views[name] = (View(join_bufs[j][0], o, co, N, hw_out, hw_out), View(join_bufs[j][1], o, co, N, hw_out, hw_out))
                else:
                    views[name] = (View(buf(N * hw_out * hw_out, co), 0, co, N, hw_out, hw_out),
                                   View(buf(N * hw_out * hw_out, _pad16(co)), 0, co, N, hw_out, hw_out))
                x, dx = views[cur]
                L = Layer(name, kind, 3, x.C, co, s, True)
                L.x, L.dx, (L.y, L.dy) = x, dx, views[name]
                self.layers.append(L)
                cur, hw = name, hw_out
            x, dx = views[cur]
            L = Layer(LOGITS, 'conv', 3, x.C, 1, 1, False)
            L.x, L.dx = x, dx
            L.y = View(buf(N * 64, 1), 0, 1, N, WINDOW, WINDOW)
            L.dy = View(buf(N * 64, 16), 0, 1, N, WINDOW, WINDOW)
            self.layers.append(L)
            self.logits_layer = L
            x, dx = views['conv3b']
            self.fc = []
            for name, units, relu in FC:
                last = name == FC[-1][0]
                L = Layer(name, 'dense', 1, x.C, units, 1, relu, _lib.EPI_EXP_1E2 if last else _lib.EPI_NONE)
                L.x, L.dx = x, dx
                L.y = View(buf(N, units), 0, units, N, 1, 1)
                L.dy = View(buf(N, _pad16(units)), 0, units, N, 1, 1)
                self.layers.append(L)
                self.fc.append(L)
                x, dx = L.y, L.dy
            self.unet = [l for l in self.layers if l not in self.tower and l not in self.fc]
            self.views = views
            # outputs that feed two consumers: the later consumer's input gradient goes to a spare buffer and is added
            self.spare = {n: buf(views[n][0].rows, views[n][0].C) for n in ('conv0', 'conv1b', 'conv2b', 'conv3b')}
            self.second = {'conv1a': 'conv0', 'conv2a': 'conv1b', 'conv3a': 'conv2b', FC[0][0]: 'conv3b'}

            self.prob, self.flow, self.sigma = buf(N, 64), buf(N, 2), self.fc[-1].y.buf
            self.d_flow, self.d_sigma = buf(N, 2), buf(N, 1)
            self.stats = torch.zeros(16, **f32)

            ws_bytes = size_query(self.lib.kfn_first_conv_u8_grad_weights_workspace_bytes, F, H, Wd, self.tower[0].co)
            for L in self.layers[1:]:
                k, ci, co = L.k, L.ci, L.co
                if L.kind == 'deconv':                              # the stride-2 convolution V: Cout -> Cin
                    ci, co = L.co, L.ci
                L.vci, L.vco = ci, co
                L.fwd = torch.zeros(size_query(self.lib.kfn_pack_conv_weights_floats, k, k, ci, co, _lib.PACK_FORWARD), **f32)
                L.back_kind = _lib.PACK_INPUT_GRAD_S2 if L.stride == 2 else _lib.PACK_INPUT_GRAD_S1
                L.back = torch.zeros(size_query(self.lib.kfn_pack_conv_weights_floats, k, k, ci, co, L.back_kind), **f32)
                for d in self._wgrad_descs(L):
                    ws_bytes = max(ws_bytes, size_query(self.lib.kfn_conv2d_grad_weights_workspace_bytes, C.byref(d)))
            self.workspace = torch.zeros(-(-ws_bytes // 4), **f32)
            self.scratch_dw = torch.zeros(128 * 128 + 128, **f32)      # the unused halves of the bias-only launches

    # ---- descriptors -----------------------------------------------------------------------------------------------------------
    def _ptr(self, flat, L, var):
        return flat.data_ptr() + 4 * self.slots['%s/%s/%s' % (SCOPE, L.name, var)][0]

    def _wgrad_descs(self, L):
        """The kfn_conv2d_grad_weights launches of layer L: [kernel (and, for a convolution, bias)] and for a transposed layer
        the 1x1 launch whose bias row sums its output gradient."""
        cp = lambda c: -(-c // 32) * 32
        if L.kind == 'deconv':
            v = _lib.ConvDesc(N=L.y.n, H=L.y.h, W=L.y.w, Cin=L.co, ldx=L.dy.ld, Cout=L.ci, cout_pad=cp(L.ci), ldy=L.x.ld, kh=3,
                              kw=3, stride=2)
            b = _lib.ConvDesc(N=L.y.n, H=L.y.h, W=L.y.w, Cin=L.co, ldx=L.dy.ld, Cout=L.co, cout_pad=cp(L.co), ldy=L.dy.ld, kh=1,
                              kw=1, stride=1)
            return [v, b]
        return [_lib.ConvDesc(N=L.x.n, H=L.x.h, W=L.x.w, Cin=L.ci, ldx=L.x.ld, Cout=L.co, cout_pad=cp(L.co), ldy=L.dy.ld, kh=L.k,
                              kw=L.k, stride=L.stride)]

    # ---- one step ----------------------------------------------------------------------------------------------------------------
    def _repack(self, stream):
        for L in self.layers[1:]:
            w = self._ptr(self.params, L, 'kernel')
            for kind, out in ((_lib.PACK_FORWARD, L.fwd), (L.back_kind, L.back)):
                _lib.check(self.lib.kfn_pack_conv_weights(w, L.k, L.k, L.vci, L.vco, kind, out.data_ptr(), stream),
                           'kfn_pack_conv_weights[%s]' % L.name)
        self._packs_stale = False

    def stage(self, frames_u8, labels=None):
        """Brings the batch's frames (uint8 [2P,H,W,3]; [B,H,W,3] with `frames` = B) and their labels (float32 [2P,H,W,4] or
        grid-sized) to the device.  With `pair_index` the labels may be None (the caller owns the loss), and a uint8 tensor
        of the batch's shape that lies on the device already is read where it is: stage 3 stages its frames once."""
        torch = self.torch
        B, (H, Wd), (h, w) = self.nframes, self.image_size, self.grid
        if self.pair_index is not None and torch.is_tensor(frames_u8) and frames_u8.device == self.device:
            if tuple(frames_u8.shape) != (B, H, Wd, 3) or frames_u8.dtype != torch.uint8 or not frames_u8.is_contiguous():
                raise ValueError('frames on the device must be contiguous uint8 %s' % [B, H, Wd, 3])
            self.frames = frames_u8
        else:
            staging.stage(self.frames, frames_u8, torch.uint8, (B, H, Wd, 3), 'frames')
        if labels is None and self.pair_index is not None:
            return None
        self.labels, self.label_stride = staging.stage_labels(self.labels, labels, B, (H, Wd), (h, w), self.device)
        return self.label_stride

    def _conv(self, L, x, y, pack, stream, transposed=0, relu=0, bias=None, epilogue=_lib.EPI_NONE, cin=None, cout=None, stride=1):
        d = _lib.ConvDesc(N=x.n, H=x.h, W=x.w, Cin=cin, ldx=x.ld, Cout=cout, cout_pad=-(-cout // 32) * 32, ldy=y.ld, kh=L.k,
                          kw=L.k, stride=stride, transposed=transposed, relu=relu, epilogue=epilogue)
        _lib.check(self.lib.kfn_conv2d_nhwc(C.byref(d), x.ptr, pack.data_ptr(), bias, y.ptr, stream), 'kfn_conv2d_nhwc[%s]' % L.name)

    def _forward_layer(self, L, stream, y=None, epilogue=None):
        bias = self._ptr(self.params, L, 'bias')
        y = L.y if y is None else y
        epilogue = L.epilogue if epilogue is None else epilogue
        if L.kind == 'deconv':
            self._conv(L, L.x, y, L.back, stream, transposed=1, relu=int(L.relu), bias=bias, cin=L.ci, cout=L.co, stride=2)
        else:
            self._conv(L, L.x, y, L.fwd, stream, relu=int(L.relu), bias=bias, epilogue=epilogue, cin=L.ci, cout=L.co, stride=L.stride)

    def forward(self, stream=None):
        """The forward pass on the staged frames: self.flow [N,2], self.sigma [N,1], self.prob [N,64]; every output is kept."""
        stream = staging.current_stream(self.device) if stream is None else stream
        if self._packs_stale:
            self._repack(stream)
        P, F, (H, Wd), (h, w), N = self.pairs, self.nframes, self.image_size, self.grid, self.windows
        first = self.tower[0]
        _lib.check(self.lib.kfn_first_conv_u8(self.frames.data_ptr(), F, H, Wd, self._ptr(self.params, first, 'kernel'),
                                              self._ptr(self.params, first, 'bias'), first.y.ptr, first.co, None, None, None, 0,
                                              stream), 'kfn_first_conv_u8')
        for L in self.tower[1:]:
            self._forward_layer(L, stream)
        last = self.tower[-1]
        self._forward_layer(last, stream, y=View(self.feat, 0, 32, F, h, w), epilogue=_lib.EPI_L2NORM)
        if self.pair_index is None:
            f = self.feat.view(P, 2, h * w, 32)
            self.f_a.view(P, h * w, 32).copy_(f[:, 0])
            self.f_b.view(P, h * w, 32).copy_(f[:, 1])
        else:
            f = self.feat.view(F, h * w, 32)
            self.torch.index_select(f, 0, self.a_idx, out=self.f_a.view(P, h * w, 32))
            self.torch.index_select(f, 0, self.b_idx, out=self.f_b.view(P, h * w, 32))
        _lib.check(self.lib.kfn_cost_volume(self.f_a.data_ptr(), self.f_b.data_ptr(), self.vol.ptr, P, h, w, 32, WINDOW, stream),
                   'kfn_cost_volume')
        for L in self.unet + self.fc:
            self._forward_layer(L, stream)
        _lib.check(self.lib.kfn_flow_softargmax(self.logits_layer.y.ptr, self.flow.data_ptr(), self.prob.data_ptr(), N, WINDOW,
                                                stream), 'kfn_flow_softargmax')

    def loss(self, stream=None):
        """The loss launch: self.stats, self.d_flow and self.d_sigma."""
        stream = staging.current_stream(self.device) if stream is None else stream
        P, (h, w) = self.pairs, self.grid
        if self.pair_index is not None:
            raise ValueError('the loss of stage 2 reads pairs of frames (2p, 2p + 1): with pair_index the gradients are the caller\'s')
        d = _lib.FlowLossDesc(P=P, h=h, w=w, label_stride=self.label_stride, has_loss_clip=int(self.loss_clip is not None),
                              loss_clip=self.loss_clip or 0.0, dist_threshold=0.05, min_uncertainty=1e-5)
        _lib.check(self.lib.kfn_flow_loss_grad(C.byref(d), self.flow.data_ptr(), self.sigma.data_ptr(), self.labels.data_ptr(),
                                               self.d_flow.data_ptr(), self.d_sigma.data_ptr(), self.stats.data_ptr(), stream),
                   'kfn_flow_loss_grad')

    def _weight_gradient(self, L, stream):
        dw, db = self._ptr(self.grads, L, 'kernel'), self._ptr(self.grads, L, 'bias')
        descs = self._wgrad_descs(L)
        ws = self.workspace.data_ptr()
        if L.kind == 'deconv':
            _lib.check(self.lib.kfn_conv2d_grad_weights(C.byref(descs[0]), L.dy.ptr, L.x.ptr, dw, self.scratch_dw.data_ptr(), ws,
                                                        stream), 'kfn_conv2d_grad_weights[%s]' % L.name)
            _lib.check(self.lib.kfn_conv2d_grad_weights(C.byref(descs[1]), L.dy.ptr, L.dy.ptr, self.scratch_dw.data_ptr(), db, ws,
                                                        stream), 'kfn_conv2d_grad_weights[%s, bias]' % L.name)
        else:
            _lib.check(self.lib.kfn_conv2d_grad_weights(C.byref(descs[0]), L.x.ptr, L.dy.ptr, dw, db, ws, stream),
                       'kfn_conv2d_grad_weights[%s]' % L.name)

    def _input_gradient(self, L, stream):
        """d(L.x) from d(L.y).  Where L.x feeds an earlier-listed consumer too, the result goes to the spare buffer and is added."""
        target = L.dx
        spare = self.second.get(L.name)
        if spare is not None:
            s = self.spare[spare]
            target = View(s, 0, L.x.C, L.x.n, L.x.h, L.x.w)
        if L.kind == 'deconv':
            self._conv(L, L.dy, target, L.fwd, stream, cin=L.co, cout=L.ci, stride=2)
        else:
            # dZ's channels up to the next multiple of 16 (zero behind Cout): the input-gradient pack's columns
            self._conv(L, L.dy, target, L.back, stream, transposed=int(L.stride == 2), cin=_pad16(L.co), cout=L.ci, stride=L.stride)
        if spare is not None:
            L.dx.tensor().add_(target.tensor())

    def _relu_mask(self, y, dy, stream):
        _lib.check(self.lib.kfn_relu_grad(y.ptr, y.ld, dy.ptr, dy.ld, y.rows, y.C, stream), 'kfn_relu_grad')

    def backward(self, d_flow=None, d_sigma=None, stream=None):
        """The backward pass into self.grads from the gradients with respect to flow [N,2] and sigma_trans [N] -- the loss's
        by default; explicit device tensors are the seam of joint stage 3."""
        stream = staging.current_stream(self.device) if stream is None else stream
        P, F, (H, Wd), (h, w), N = self.pairs, self.nframes, self.image_size, self.grid, self.windows
        d_flow = self.d_flow if d_flow is None else d_flow
        d_sigma = self.d_sigma if d_sigma is None else d_sigma
        lg, un = self.logits_layer, self.fc[-1]
        _lib.check(self.lib.kfn_flow_head_backward(d_flow.data_ptr(), self.prob.data_ptr(), d_sigma.data_ptr(), self.sigma.data_ptr(),
                                                   lg.dy.ptr, lg.dy.ld, un.dy.ptr, un.dy.ld, N, stream), 'kfn_flow_head_backward')
        by_output = {L.name: L for L in self.layers}
        # the decoder and the logits first, then the dense head (its gradient joins conv3b's), then the encoder
        order = [L for L in reversed(self.unet) if L.name not in ('conv0', 'conv1a', 'conv1b', 'conv2a', 'conv2b', 'conv3a', 'conv3b')]
        order += list(reversed(self.fc)) + [by_output[n] for n in ('conv3b', 'conv3a', 'conv2b', 'conv2a', 'conv1b', 'conv1a', 'conv0')]
        masked = set()
        for L in order:
            if L.relu and L.name not in masked:
                self._relu_mask(L.y, L.dy, stream)
                masked.add(L.name)
            self._weight_gradient(L, stream)
            self._input_gradient(L, stream)
        _lib.check(self.lib.kfn_cost_volume_backward(self.d_vol.ptr, self.d_fb.data_ptr(), self.d_fa.data_ptr(), P, h, w, 32, stream),
                   'kfn_cost_volume_backward')
        if self.pair_index is None:
            g = self.d_feat.view(P, 2, h * w, 32)
            g[:, 0].copy_(self.d_fa.view(P, h * w, 32))
            g[:, 1].copy_(self.d_fb.view(P, h * w, 32))
        else:
            # a frame is at most once a b and once an a: its row is zero, then d_fb, then d_fb + d_fa -- one add per address
            g = self.d_feat.view(F, h * w, 32)
            g.zero_()
            g.index_copy_(0, self.b_idx, self.d_fb.view(P, h * w, 32))
            g.index_add_(0, self.a_idx, self.d_fa.view(P, h * w, 32))
        last = self.tower[-1]
        _lib.check(self.lib.kfn_l2norm_backward(last.y.ptr, last.y.ld, self.d_feat.data_ptr(), 32, last.dy.ptr, last.dy.ld,
                                                F * h * w, 32, stream), 'kfn_l2norm_backward')
        for L in reversed(self.tower[1:]):
            if L.relu:
                self._relu_mask(L.y, L.dy, stream)
            self._weight_gradient(L, stream)
            self._input_gradient(L, stream)
        first = self.tower[0]
        self._relu_mask(first.y, first.dy, stream)
        _lib.check(self.lib.kfn_first_conv_u8_grad_weights(self.frames.data_ptr(), F, H, Wd, first.dy.ptr, first.co,
                                                           self._ptr(self.grads, first, 'kernel'), self._ptr(self.grads, first, 'bias'),
                                                           self.workspace.data_ptr(), stream), 'kfn_first_conv_u8_grad_weights')

    def step(self, frames_u8, labels):
        """One update on 2P frames and their labels.  Returns StepStats of THIS step's loss, before the update."""
        with self.torch.cuda.device(self.device):
            stream = staging.current_stream(self.device)
            self.stage(frames_u8, labels)
            self.forward(stream)
            self.loss(stream)
            self.backward(stream=stream)
            stats = self.stats.clone()
            lr = self.apply_gradients(stream)
            self._repack(stream)
        return StepStats(stats, lr)
