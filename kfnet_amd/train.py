"""Training SCoordNet on the device: stage 1 of the reference's procedure ("Train SCoordNet").

The reference builds the TF-1 graph of KFNet/train.py:268-315 and lets tf.gradients / AdamOptimizer derive the rest.  Here
one step is a fixed list of launches of libkfnet_hip.so (DESIGN.md "Training"):

    augment      (step(..., augment=params) only) kfn_augment_batch: the raw batch -> self.frames and grid-sized labels
    forward      kfn_first_conv_u8, then kfn_conv2d_nhwc per layer (the direct route, fp32, every output kept)
    loss         kfn_coord_loss_grad: NLL + smoothness on the prepared labels, and d(loss)/d(prediction)
                 (reproj_weight > 0 only) kfn_reproj_loss_grad behind it: w_r * R of KFNet.ReprojectionLoss and its gradient
                 added to d(loss)/d(prediction); with augment= the rays come from kfn_augment_pixel_map
    backward     per layer, last to first: kfn_conv2d_grad_weights; the input gradient on the FORWARD kernel
                 (stride 1: kfn_conv2d_nhwc with the rotated, channel-swapped pack; stride 2: its transposed form);
                 kfn_relu_grad.  conv1a: kfn_first_conv_u8_grad_weights.
    update       kfn_adam_step on the flat parameter buffer (TensorFlow's Adam, L2 regulariser folded in)
    packs        kfn_pack_conv_weights: the forward and input-gradient matrices of the new weights

Nothing travels through the host inside a step, and nothing is read back unless the caller asks (StepStats).  There is no
fallback: a missing entry point or an unsupported shape raises.

Definitions that are this module's own (the reference's SCoordNet training branch is not in the snapshot):
`global_step` counts applied updates, the learning rate of update number global_step + 1 is base_lr * gamma ** (global_step /
stepvalue), and Adam's t is the number of updates applied since the slots were zero, + 1.

precision='fp16'  runs the layers of f16_layer() on fp16 MFMA operands -- forward, weight gradient and input
gradient; tensors, master weights and Adam's slots stay fp32 -- under dynamic loss scaling whose state lives on the device:
the loss gradient is multiplied by the scale, the weight gradients are divided by it and checked, and kfn_adam_step_guarded
applies the update only if every gradient is finite.  `global_step` then counts ATTEMPTED steps (it drives the learning
rate and the batch stream; the host cannot know whether a step was applied), Adam's t counts applied ones on the device.
"""
import ctypes as C

import numpy as np

from . import _lib, staging
from .cnn_wrapper.SCoordNet import layers
from .train_common import BETA1, BETA2, EPSILON, LazyStats, ParamStore, learning_rate, read_snapshot, size_query
from .train_common import adam_lr_t, snapshot_paths  # noqa: F401  (callers of this module read them here)

LAYERS = layers()                                 # (name, kernel, Cin, Cout, stride, relu), the architecture's own table
SCOPE = 'ScoreNet'
PRECISIONS = ('fp32', 'fp16')
MAX_LOSS_SCALE = 2 ** 24


def f16_layer(kernel, cin, cout):
    """The one statement of which layers precision='fp16' runs on fp16 operands: those whose three launches all take them.
    kfn_conv2d_nhwc needs Cin % 32 == 0 of what it reads -- the layer's input going forward, its dZ (Cout channels) going
    back -- and kfn_conv2d_grad_weights needs both.  That leaves out conv1a (3 input channels, its own entry points) and
    'prediction' (4 output channels), the head that carries the log-uncertainty.  Every eligible layer's fp16 weight
    gradient is faster than its fp32 launch, so none is routed back."""
    return cin % 32 == 0 and cout % 32 == 0


def power_of_two(x):
    m, _ = np.frexp(float(x))
    return float(x) > 0 and m == 0.5


def batch_indices(step, batch, count, shuffle=False, seed=0):
    """The frames of update number `step` (from 0): consecutive indices that wrap round; with `shuffle` position q of the
    stream is entry q % count of a permutation drawn per epoch q // count from (seed, epoch).  A function of its arguments
    alone, so a resumed run continues the same stream."""
    out = []
    perms = {}
    for j in range(batch):
        q = step * batch + j
        if not shuffle:
            out.append(q % count)
            continue
        e = q // count
        if e not in perms:
            perms[e] = np.random.default_rng([int(seed), int(e)]).permutation(count)
        out.append(int(perms[e][q % count]))
    return out


def synthetic_labels(count, grid_hw, seed=3, start=0):
    """Grid-sized label maps [count,h,w,4] of a seeded synthetic scene, for runs without data: a gently curved surface seen
    from a camera that drifts with the frame index; the mask leaves out a border column and a moving block."""
    h, w = grid_hw
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.5, 1.5, size=6)
    r, c = np.meshgrid(np.arange(h, dtype=np.float64) / h, np.arange(w, dtype=np.float64) / w, indexing='ij')
    out = np.zeros((count, h, w, 4), dtype=np.float32)
    for i in range(count):
        t = 0.05 * (start + i)
        out[i, ..., 0] = a[0] * c + t
        out[i, ..., 1] = a[1] * r - 0.5 * t
        out[i, ..., 2] = 1.5 + a[2] * np.sin(a[3] * c + t) * np.cos(a[4] * r)
        m = np.ones((h, w), dtype=np.float32)
        m[:, 0] = 0.0
        b = (start + i) % max(w - 2, 1)
        m[h // 2:h // 2 + 2, b:b + 2] = 0.0
        out[i, ..., 3] = m
    return out


def beta_powers(t):
    """(beta1^t, beta2^t) as the device accumulates them: one fp64 multiplication per applied step."""
    p1 = p2 = 1.0
    for _ in range(int(t)):
        p1, p2 = p1 * BETA1, p2 * BETA2
    return p1, p2


class StepStats(LazyStats):
    """loss, l_measure, l_smooth, a_measure, pixels, lr."""
    KEYS = ('loss', 'l_measure', 'l_smooth', 'a_measure', 'pixels', 'lr')
    SCALE_KEYS = ('loss_scale', 'skipped')      # precision='fp16' only: the scale after this step, the steps skipped so far
    REPROJ_KEYS = ('l_reproj',)                 # reproj_weight > 0 only: R itself; `loss` then includes reproj_weight * R

    def __init__(self, stats_dev, lr, scale_dev=None, reproj_dev=None):
        LazyStats.__init__(self, stats_dev, lr)
        self._scale_dev, self._reproj_dev = scale_dev, reproj_dev

    def keys(self):
        return (list(self.KEYS) + (list(self.SCALE_KEYS) if self._scale_dev is not None else []) +
                (list(self.REPROJ_KEYS) if self._reproj_dev is not None else []))

    def _decode(self, s):
        # kfn_coord_loss_grad's stats; valid = sum(mask) + 1, the reference logs np.sum(masks)
        host = dict(loss=float(s[4]), l_measure=float(s[0]), l_smooth=float(s[1]), a_measure=float(s[2]),
                    pixels=float(s[3]) - 1.0, lr=self._lr)
        if self._scale_dev is not None:
            st = _lib.LossScaleState.from_buffer_copy(self._scale_dev.cpu().numpy().tobytes())
            host.update(loss_scale=float(st.scale), skipped=int(st.skipped))
        if self._reproj_dev is not None:
            r = self._reproj_dev.cpu().numpy()       # kfn_reproj_loss_grad's stats: R, ., ., weight * R
            host.update(l_reproj=float(r[0]), loss=float(s[4]) + float(r[3]))
        return host


class SCoordNetTrainer(ParamStore):
    def __init__(self, weights, image_size=(480, 640), batch=4, transform=None, base_lr=1e-4, gamma=0.5, stepvalue=80000,
                 weight_decay=1e-4, loss_clip=None, smooth_weight=50.0, device='cuda:0', precision='fp32', loss_scale=2 ** 15,
                 growth_interval=2000, reproj_weight=0.0, camera=None):
        """weights: {TF name: array} holding at least ScoreNet/*.  transform: the 4x4 of transform.txt ITSELF (labels are
        mapped by it, KFNet/train.py:279-280), None = identity.  loss_clip: None (no clip) or the reference's -2.0.
        precision: 'fp32', or 'fp16' = fp16 MFMA operands in the layers of f16_layer() under dynamic loss scaling that starts
        at loss_scale (a power of two in 1 .. 2^24) and doubles after growth_interval applied steps without an overflow.
        reproj_weight: w_r of the reprojection term w_r * R (KFNet/KFNet.py:246-248 uses 50; 0 = off: nothing of it is
        launched or allocated); camera: the kfnet_amd.labels.DepthCamera whose intrinsics give the cells' rays (None: the
        7-Scenes defaults).  Every step() then needs a set_poses() in front of it."""
        import torch
        H, Wd = image_size
        staging.check_size(H, Wd, 'the height and width of a training batch')
        if batch < 1:
            raise ValueError('batch must be >= 1')
        if precision not in PRECISIONS:
            raise ValueError('precision must be one of %s' % (PRECISIONS,))
        if not (power_of_two(loss_scale) and 1 <= loss_scale <= MAX_LOSS_SCALE):
            raise ValueError('loss_scale must be a power of two in 1 .. 2^24')
        if growth_interval < 1:
            raise ValueError('growth_interval must be >= 1')
        self.precision, self.loss_scale, self.growth_interval = precision, float(loss_scale), int(growth_interval)
        self.f16 = [precision == 'fp16' and f16_layer(k, ci, co) for _, k, ci, co, _, _ in LAYERS]
        self.lib = _lib.load()
        self.image_size, self.batch = (H, Wd), batch
        self.grid = (H // 8, Wd // 8)
        self.loss_clip = None if loss_clip is None else float(loss_clip)
        self.smooth_weight = float(smooth_weight)
        self.transform = None if transform is None else np.asarray(transform, dtype=np.float32).reshape(4, 4)
        from .reproj import check_weights
        self.reproj_weight = check_weights(reproj_weight, 1)[0]
        self.reproj = None                # kfnet_amd.reproj.ReprojTerm when the weight is positive
        self.pixel_map = None             # [h,w,2]: the augmented pixel map, made by the first augmented step with the term on
        self._poses_set = False           # set_poses() has run since the last step
        self._pixel_map_live = False      # the staged batch is augmented: the rays come from self.pixel_map

        # the flat parameter store: kernel then bias per layer, TF HWIO order
        specs = [(self.variable(li, kind), shape) for li, (name, k, ci, co, _, _) in enumerate(LAYERS)
                 for kind, shape in (('kernel', (k, k, ci, co)), ('bias', (co,)))]
        ParamStore.__init__(self, specs, device, base_lr, gamma, stepvalue, weight_decay)
        with torch.cuda.device(self.device):
            f32 = dict(dtype=torch.float32, device=self.device)
            self.set_weights(weights)

            # activations (each layer's output after its ReLU) and the gradients with respect to them
            self.frames = torch.zeros((batch, H, Wd, 3), dtype=torch.uint8, device=self.device)
            self.labels = None
            self._augmenter = None        # kfnet_amd.augment.Augmenter, made by the first step(..., augment=params)
            self.shapes, self.act, self.dact, self.packs = [], [], [], []
            h, w = H, Wd
            ws_bytes = size_query(self.lib.kfn_first_conv_u8_grad_weights_workspace_bytes, batch, H, Wd, LAYERS[0][3])
            for li, (name, k, ci, co, s, relu) in enumerate(LAYERS):
                hin, win = h, w
                h, w = -(-h // s), -(-w // s)
                self.shapes.append((hin, win, h, w))
                self.act.append(torch.zeros((batch, h, w, co), **f32))
                self.dact.append(torch.zeros((batch, h, w, -(-co // 16) * 16), **f32))   # 'prediction': 4 of 16 channels
                if li == 0:
                    self.packs.append(None)
                    continue
                pk = dict(f32, dtype=torch.float16) if self.f16[li] else f32     # the same layout, halfs under fp16 operands
                fwd = torch.zeros(size_query(self.lib.kfn_pack_conv_weights_floats, k, k, ci, co, _lib.PACK_FORWARD), **pk)
                kind = _lib.PACK_INPUT_GRAD_S2 if s == 2 else _lib.PACK_INPUT_GRAD_S1
                back = torch.zeros(size_query(self.lib.kfn_pack_conv_weights_floats, k, k, ci, co, kind), **pk)
                self.packs.append((fwd, back, kind))
                d = self._fwd_desc(li)
                ws_bytes = max(ws_bytes, size_query(self.lib.kfn_conv2d_grad_weights_workspace_bytes, C.byref(d)))
            self.workspace = torch.zeros(-(-ws_bytes // 4), **f32)
            self.stats = torch.zeros(8, **f32)
            if self.reproj_weight > 0.0:
                from .reproj import ReprojTerm
                self.reproj = ReprojTerm(batch, self.grid[0], self.grid[1], camera, self.transform, self.device)
            self.scale_state = None           # kfn_loss_scale_state on the device
            if precision == 'fp16':
                self.scale_state = torch.zeros(C.sizeof(_lib.LossScaleState), dtype=torch.uint8, device=self.device)
                self._write_scale_state(self.loss_scale, 0, 0, 0, 1.0, 1.0)

    # ---- descriptors ----------------------------------------------------------------------------------------------
    def _fwd_desc(self, li):
        """The forward convolution of layer li; as the weight gradient's descriptor its ldy is dZ's pixel stride."""
        name, k, ci, co, s, relu = LAYERS[li]
        hin, win, _, _ = self.shapes[li]
        return _lib.ConvDesc(N=self.batch, H=hin, W=win, Cin=ci, ldx=ci, Cout=co, cout_pad=-(-co // 32) * 32, ldy=co,
                             kh=k, kw=k, stride=s, transposed=0, relu=int(relu), operand_dtype=self._operands(li))

    def _operands(self, li):
        return _lib.OPERAND_F16 if self.f16[li] else _lib.OPERAND_F32

    @staticmethod
    def variable(li, kind):
        """The TF name of layer li's 'kernel' or 'bias'."""
        return '%s/%s/%s' % (SCOPE, LAYERS[li][0], kind)

    def _ptr(self, buf, li, kind):
        return buf.data_ptr() + 4 * self.slots[self.variable(li, kind)][0]

    # ---- the loss-scale record beside the store's optimiser state ---------------------------------------------------
    def _write_scale_state(self, scale, good_steps, skipped, adam_t, beta1_power, beta2_power):
        rec = _lib.LossScaleState(beta1_power=beta1_power, beta2_power=beta2_power, scale=scale, good_steps=good_steps,
                                  overflow=0, skipped=skipped, adam_t=adam_t)
        self.scale_state.copy_(self.torch.from_numpy(np.frombuffer(bytes(rec), dtype=np.uint8).copy()))

    def loss_scale_state(self):
        """precision='fp16': the device's record, read back -- dict(scale, good_steps, skipped, adam_t, beta1_power,
        beta2_power)."""
        rec = _lib.LossScaleState.from_buffer_copy(self.scale_state.cpu().numpy().tobytes())
        return dict(scale=float(rec.scale), good_steps=int(rec.good_steps), skipped=int(rec.skipped), adam_t=int(rec.adam_t),
                    beta1_power=float(rec.beta1_power), beta2_power=float(rec.beta2_power))

    def state(self):
        """The store's state; with precision='fp16' the loss-scale record too, whose adam_t counts the APPLIED steps."""
        if self.precision != 'fp16':
            return ParamStore.state(self)
        ls = self.loss_scale_state()
        self.adam_t = ls['adam_t']
        st = ParamStore.state(self)
        st.update(loss_scale=np.float32(ls['scale']), loss_scale_good_steps=np.int64(ls['good_steps']),
                  loss_scale_skipped=np.int64(ls['skipped']), adam_beta1_power=np.float64(ls['beta1_power']),
                  adam_beta2_power=np.float64(ls['beta2_power']))
        return st

    def load_state(self, st):
        """A state file written without the loss-scale record (before it existed, or by an fp32 run) loads with the
        constructor's scale, zero counters and the powers of beta that adam_t applied steps accumulate."""
        ParamStore.load_state(self, st)
        if self.precision == 'fp16':
            if 'loss_scale' in st:
                self._write_scale_state(float(st['loss_scale']), int(st['loss_scale_good_steps']), int(st['loss_scale_skipped']),
                                        self.adam_t, float(st['adam_beta1_power']), float(st['adam_beta2_power']))
            else:
                self._write_scale_state(self.loss_scale, 0, 0, self.adam_t, *beta_powers(self.adam_t))

    # ---- one step ----------------------------------------------------------------------------------------------------
    @staticmethod
    def needs_full_resolution(augmented):
        """The one statement of which labels a step needs: an augmented step (`augmented` true) the full-resolution ones,
        because it interpolates between label pixels; any other step only the pixels (8r, 8c) that the loss reads."""
        return bool(augmented)

    def label_shape(self, augmented=False):
        """The shape of the labels that a step expects, augmented (step(..., augment=params)) or not."""
        (H, Wd), (h, w) = self.image_size, self.grid
        return (self.batch, H, Wd, 4) if self.needs_full_resolution(augmented) else (self.batch, h, w, 4)

    def _repack(self, stream):
        for li, (name, k, ci, co, s, relu) in enumerate(LAYERS):
            if li == 0:
                continue          # conv1a's forward matrix [27][C] is the master copy
            fwd, back, kind = self.packs[li]
            w = self._ptr(self.params, li, 'kernel')
            pack = self.lib.kfn_pack_conv_weights_f16 if self.f16[li] else self.lib.kfn_pack_conv_weights
            _lib.check(pack(w, k, k, ci, co, _lib.PACK_FORWARD, fwd.data_ptr(), stream), 'kfn_pack_conv_weights[%s]' % name)
            _lib.check(pack(w, k, k, ci, co, kind, back.data_ptr(), stream), 'kfn_pack_conv_weights[%s, input gradient]' % name)
        self._packs_stale = False

    def stage(self, frames_u8, labels, augment=None, stream=None):
        """Brings a batch to self.frames and self.labels and returns the stride at which the loss reads the labels.  Without
        `augment` the labels may be grid-sized (stride 1) or full-resolution (stride 8).  With it the raw batch goes to the
        augmenter's staging buffers and kfn_augment_batch writes self.frames and grid-sized labels (output pixels (8r, 8c))."""
        torch = self.torch
        B, (H, Wd), (h, w) = self.batch, self.image_size, self.grid
        if augment is not None:
            if self._augmenter is None:
                from .augment import Augmenter
                self._augmenter = Augmenter(B, H, Wd, label_stride=8, device=self.device)
            aug = self._augmenter
            if labels is None:
                raise ValueError('training needs labels')
            fin, lin = aug.stage(frames_u8, labels)          # ValueError on grid-sized labels
            self.labels = aug.labels_out
            stream = staging.current_stream(self.device) if stream is None else stream
            aug.launch(augment, fin, lin, self.frames, self.labels, stream)
            if self.reproj is not None:       # the cells' rays go through the same rotation and zoom (KFNet/train.py:181-187)
                if self.pixel_map is None:
                    self.pixel_map = torch.zeros((h, w, 2), dtype=torch.float32, device=self.device)
                aug.pixel_map(augment, self.reproj.camera, self.pixel_map, stream)
                self._pixel_map_live = True
            return 1
        self._pixel_map_live = False
        staging.stage(self.frames, frames_u8, torch.uint8, (B, H, Wd, 3), 'frames')
        self.labels, stride = staging.stage_labels(self.labels, labels, B, (H, Wd), (h, w), self.device)
        return stride

    def forward_layer(self, li, stream):
        """Layer li's forward launch: self.act[li] from self.act[li - 1] (conv1a: from self.frames)."""
        name, co = LAYERS[li][0], LAYERS[li][3]
        bias = self._ptr(self.params, li, 'bias')
        if li == 0:
            H, Wd = self.image_size
            _lib.check(self.lib.kfn_first_conv_u8(self.frames.data_ptr(), self.batch, H, Wd, self._ptr(self.params, 0, 'kernel'),
                                                  bias, self.act[0].data_ptr(), co, None, None, None, 0, stream),
                       'kfn_first_conv_u8')
            return
        d = self._fwd_desc(li)
        _lib.check(self.lib.kfn_conv2d_nhwc(C.byref(d), self.act[li - 1].data_ptr(), self.packs[li][0].data_ptr(), bias,
                                            self.act[li].data_ptr(), stream), 'kfn_conv2d_nhwc[%s]' % name)

    def weight_gradient(self, li, stream):
        """Layer li's kernel and bias gradients into self.grads, from its input and self.dact[li]."""
        name, co = LAYERS[li][0], LAYERS[li][3]
        dw, db = self._ptr(self.grads, li, 'kernel'), self._ptr(self.grads, li, 'bias')
        if li == 0:
            H, Wd = self.image_size
            _lib.check(self.lib.kfn_first_conv_u8_grad_weights(self.frames.data_ptr(), self.batch, H, Wd,
                                                               self.dact[0].data_ptr(), co, dw, db,
                                                               self.workspace.data_ptr(), stream),
                       'kfn_first_conv_u8_grad_weights')
            return
        gd = self._fwd_desc(li)
        gd.ldy = self.dact[li].shape[3]
        _lib.check(self.lib.kfn_conv2d_grad_weights(C.byref(gd), self.act[li - 1].data_ptr(), self.dact[li].data_ptr(), dw, db,
                                                    self.workspace.data_ptr(), stream), 'kfn_conv2d_grad_weights[%s]' % name)

    def input_gradient(self, li, stream):
        """self.dact[li - 1] from self.dact[li] (li >= 1): the forward kernel on dZ with the pack kfn_pack_conv_weights made
        for it, then the ReLU of layer li - 1."""
        name, k, ci, co, s, relu = LAYERS[li]
        hin, win, ho, wo = self.shapes[li]
        dz, ldz = self.dact[li], self.dact[li].shape[3]
        bd = _lib.ConvDesc(N=self.batch, H=ho, W=wo, Cin=ldz, ldx=ldz, Cout=ci, cout_pad=-(-ci // 32) * 32, ldy=ci, kh=k,
                           kw=k, stride=s, transposed=int(s == 2), relu=0, operand_dtype=self._operands(li))
        _lib.check(self.lib.kfn_conv2d_nhwc(C.byref(bd), dz.data_ptr(), self.packs[li][1].data_ptr(), None,
                                            self.dact[li - 1].data_ptr(), stream), 'kfn_conv2d_nhwc[%s, input gradient]' % name)
        _lib.check(self.lib.kfn_relu_grad(self.act[li - 1].data_ptr(), ci, self.dact[li - 1].data_ptr(), ci,
                                          self.batch * hin * win, ci, stream), 'kfn_relu_grad[%s]' % LAYERS[li - 1][0])

    def forward(self, stream=None):
        """The forward pass on the uploaded frames; every layer's output stays in self.act."""
        stream = staging.current_stream(self.device) if stream is None else stream
        if self._packs_stale:
            self._repack(stream)
        for li in range(len(LAYERS)):
            self.forward_layer(li, stream)

    def loss(self, label_stride, stream=None):
        """The loss launch: self.stats, and d(loss)/d(prediction) into self.dact[-1]; with the reprojection term on, its launch
        behind it (self.reproj.stats; the poses of the staged batch must have been set, self.reproj.set_poses)."""
        stream = staging.current_stream(self.device) if stream is None else stream
        B, (h, w) = self.batch, self.grid
        last = len(LAYERS) - 1
        d = _lib.CoordLossDesc(B=B, h=h, w=w, ld_pred=LAYERS[last][3], ld_dpred=self.dact[last].shape[3],
                               label_stride=label_stride, img_stride=8, has_transform=int(self.transform is not None),
                               has_loss_clip=int(self.loss_clip is not None), loss_clip=self.loss_clip or 0.0,
                               smooth_weight=self.smooth_weight, dist_threshold=0.05, min_uncertainty=1e-5)
        if self.transform is not None:
            d.transform = (C.c_float * 12)(*[float(x) for x in self.transform[:3].reshape(-1)])
        _lib.check(self.lib.kfn_coord_loss_grad(C.byref(d), self.act[last].data_ptr(), self.labels.data_ptr(),
                                                self.frames.data_ptr(), self.dact[last].data_ptr(), self.stats.data_ptr(),
                                                stream), 'kfn_coord_loss_grad')
        if self.reproj is not None:           # adds into self.dact[last], so behind the NLL and in front of the loss scale
            self.reproj.launch([(self.act[last], self.dact[last], self.reproj_weight)], self.labels, label_stride,
                               self.pixel_map if self._pixel_map_live else None, self.stats, 3, stream)
        if self.precision == 'fp16':          # everything behind this point of the backward pass carries the scale
            _lib.check(self.lib.kfn_loss_scale_apply(self.dact[last].data_ptr(), self.dact[last].numel(),
                                                     self.scale_state.data_ptr(), stream), 'kfn_loss_scale_apply')

    def backward(self, stream=None):
        """The backward pass from self.dact[-1] (the gradient with respect to the prediction) into self.grads.  With
        precision='fp16' self.dact[-1] carries the loss scale; self.grads is divided by it here and the overflow flag set, so
        that gradients() returns plain gradients either way."""
        stream = staging.current_stream(self.device) if stream is None else stream
        last = len(LAYERS) - 1
        for li in range(last, 0, -1):
            self.weight_gradient(li, stream)
            self.input_gradient(li, stream)
        self.weight_gradient(0, stream)
        if self.precision == 'fp16':
            _lib.check(self.lib.kfn_loss_scale_unscale_check(self.grads.data_ptr(), self.num_floats, self.scale_state.data_ptr(),
                                                             stream), 'kfn_loss_scale_unscale_check')

    def loss_and_gradients(self, label_stride, stream=None):
        """Loss on self.act[-1], then the backward pass into self.grads."""
        self.loss(label_stride, stream)
        self.backward(stream)

    def apply_gradients(self, stream=None):
        """The store's Adam step; with precision='fp16' the guarded one: applied or skipped, the device decides, and its
        record supplies Adam's bias correction."""
        if self.precision != 'fp16':
            return ParamStore.apply_gradients(self, stream)
        stream = staging.current_stream(self.device) if stream is None else stream
        lr = learning_rate(self.base_lr, self.gamma, self.stepvalue, self.global_step)
        _lib.check(self.lib.kfn_adam_step_guarded(self.params.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                                  self.grads.data_ptr(), self.num_floats, lr, BETA1, BETA2, EPSILON,
                                                  self.weight_decay, self.growth_interval, self.scale_state.data_ptr(),
                                                  stream), 'kfn_adam_step_guarded')
        self.global_step += 1
        self._packs_stale = True
        return lr

    def set_poses(self, poses):
        """The camera-to-world 4x4 of each frame of the NEXT step's batch ([B,4,4]): what the reprojection term reads.  Every
        step with reproj_weight > 0 needs its own call (step() keeps the signature its callers know); without the term the
        poses are not looked at."""
        if self.reproj is not None:
            with self.torch.cuda.device(self.device):
                self.reproj.set_poses(poses)
            self._poses_set = True

    def step(self, frames_u8, labels, augment=None):
        """One update on a batch: frames uint8 [B,H,W,3], labels float32 [B,H,W,4] or grid-sized [B,H/8,W/8,4] =
        (gt xyz, mask).  augment: None, or the kfnet_amd.augment.AugmentParams of this batch -- the labels must then be the
        full-resolution ones, and forward pass, loss and smoothness weights see the augmented frames.  Returns
        StepStats (loss, l_measure, l_smooth, a_measure, pixels, lr of THIS step's loss, before the update), read back only
        when accessed.  With reproj_weight > 0 set_poses() must have handed over this batch's poses (ValueError otherwise);
        the stats then hold l_reproj too, and loss includes reproj_weight * l_reproj."""
        if self.reproj is not None and not self._poses_set:
            raise ValueError('the reprojection term needs the poses of this batch: call set_poses(poses) before every step')
        self._poses_set = False
        with self.torch.cuda.device(self.device):
            stream = staging.current_stream(self.device)
            stride = self.stage(frames_u8, labels, augment, stream)
            self.forward(stream)
            self.loss_and_gradients(stride, stream)
            stats = self.stats.clone()
            lr = self.apply_gradients(stream)
            self._repack(stream)
            scale = self.scale_state.clone() if self.precision == 'fp16' else None
            reproj = self.reproj.stats.clone() if self.reproj is not None else None
        return StepStats(stats, lr, scale, reproj)


def restore(model_folder, verbose=True, scope=SCOPE):
    """The newest snapshot of a model folder for resuming: (weights of `scope` or None, state or None, step).  The snapshot may
    be a TF checkpoint or a kfnet_weights*.npz, with or without a kfnet_train_state-<step>.npz beside it."""
    W, state, step = read_snapshot(model_folder, (scope,), verbose)
    if W is not None:
        W = {k: v for k, v in W.items() if k.startswith(scope + '/')}
    return W, state, step
