"""Reference of mixed-precision training (kfnet_amd.train.SCoordNetTrainer(precision='fp16')), test
infrastructure only: tests/train_ref.py with the convolutions that the trainer runs on fp16 operands replaced by a
torch.autograd.Function that rounds what the kernels round, and a numpy restatement of the loss-scale state machine with
TensorFlow's Adam behind it."""
import numpy as np
import torch
import torch.nn.functional as F

import train_ref as R
from oracle.kfnet_oracle_torch import SCOORD, conv_same

FP32_LAYERS = ('conv1a', 'prediction')     # the layers that stay on fp32 operands (the issue's table); every other one is fp16
MAX_SCALE = 2.0 ** 24


def r16(t):
    """Round to IEEE half (nearest even) and widen again."""
    return t.to(torch.float16).to(t.dtype)


class HalfConv(torch.autograd.Function):
    """conv_same without its ReLU as the fp16-operand launches compute it.  Forward: input and kernel rounded to halfs, exact
    products, the bias added unrounded.  Backward: the incoming gradient times the loss scale is rounded to halfs (the scale
    is a power of two, so dividing it out again is exact), then multiplied with the rounded kernel (input gradient) and the
    rounded input (kernel gradient); the bias gradient sums the rounded gradient (the GEMM's constant-1 row)."""

    @staticmethod
    def forward(ctx, x, w, b, stride, scale):
        x16, w16 = r16(x), r16(w)
        ctx.save_for_backward(x16, w16)
        ctx.stride, ctx.scale = stride, scale
        return conv_same(x16, w16, b, stride, False)

    @staticmethod
    def backward(ctx, g):
        x16, w16 = ctx.saved_tensors
        g16 = r16(g * ctx.scale) / ctx.scale
        with torch.enable_grad():
            xx, ww = x16.detach().requires_grad_(True), w16.detach().requires_grad_(True)
            gx, gw = torch.autograd.grad(conv_same(xx, ww, None, ctx.stride, False), [xx, ww], g16)
        return gx, gw, g16.sum((0, 2, 3)), None, None


def network(frames_u8, W, scale):
    """train_ref.network with HalfConv in the fp16 layers."""
    dt = W['ScoreNet/conv1a/kernel'].dtype
    x = torch.from_numpy(np.ascontiguousarray(frames_u8)).to(dt).permute(0, 3, 1, 2)
    x = (x - 128.0) * 0.00625
    for name, s, relu in SCOORD:
        k, b = W['ScoreNet/%s/kernel' % name], W['ScoreNet/%s/bias' % name]
        if name in FP32_LAYERS:
            x = conv_same(x, k, b, s, relu)
        else:
            x = HalfConv.apply(x, k, b, s, float(scale))
            x = F.relu(x) if relu else x
    return x.permute(0, 2, 3, 1)


def loss_and_grads(frames_u8, labels, Wnp, M=None, loss_clip=None, smooth_weight=50.0, dtype=torch.float64, scale=2.0 ** 15):
    """train_ref.loss_and_grads of the mixed-precision network: (stats, {name: UNSCALED gradient, fp64 ndarray})."""
    W = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)).to(dtype).requires_grad_(True) for k, v in Wnp.items()
         if k.startswith('ScoreNet/')}
    pred = network(frames_u8, W, scale)
    h, w = pred.shape[1:3]
    L, nll, sm, acc, valid = R.coord_loss(pred, R.grid_labels(labels, (h, w)), np.asarray(frames_u8)[:, ::8, ::8][:, :h, :w], M,
                                          loss_clip, smooth_weight)
    names = sorted(W)
    grads = torch.autograd.grad(L, [W[n] for n in names])
    stats = dict(loss=L.item(), l_measure=nll.item(), l_smooth=sm.item(), a_measure=acc.item(), pixels=valid.item() - 1.0)
    return stats, {n: g.detach().to(torch.float64).numpy() for n, g in zip(names, grads)}


def smallest_preactivation(frames_u8, Wnp, scale=2.0 ** 15):
    """The smallest fp64 |pre-activation| over every ReLU unit of the mixed-precision network (DESIGN.md 6f's rule for
    choosing the seeds of a whole-step test)."""
    from joint_train_ref import recorded_relu_inputs
    seen = []
    W = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)) for k, v in Wnp.items() if k.startswith('ScoreNet/')}
    with torch.no_grad(), recorded_relu_inputs(seen):
        network(frames_u8, W, scale)
    return min(seen)


class LossScale(object):
    """kfn_loss_scale_state and the three launches that drive it (include/kfnet_hip.h), in numpy: the scale is a power of two
    (float32), the powers of beta are fp64 products accumulated once per applied step."""

    def __init__(self, scale=2.0 ** 15, growth_interval=2000):
        self.scale = np.float32(scale)
        self.growth_interval = int(growth_interval)
        self.good_steps = self.skipped = self.adam_t = 0
        self.beta1_power = self.beta2_power = np.float64(1.0)

    def unscale(self, g):
        """(g / scale as float32, overflow): what kfn_loss_scale_unscale_check leaves in the buffer and in the flag."""
        g = np.asarray(g, np.float32)
        return g * (np.float32(1.0) / self.scale), bool(not np.all(np.isfinite(g)))

    def lr_t(self, lr):
        """Of the update about to be applied."""
        p1, p2 = self.beta1_power * R.BETA1, self.beta2_power * R.BETA2
        return lr * np.sqrt(1.0 - p2) / (1.0 - p1)

    def update(self, overflow):
        if overflow:
            self.scale = np.float32(max(float(self.scale) * 0.5, 1.0))
            self.good_steps = 0
            self.skipped += 1
            return
        self.beta1_power = np.float64(self.beta1_power * R.BETA1)
        self.beta2_power = np.float64(self.beta2_power * R.BETA2)
        self.adam_t += 1
        self.good_steps += 1
        if self.good_steps >= self.growth_interval:
            self.scale = np.float32(min(float(self.scale) * 2.0, MAX_SCALE))
            self.good_steps = 0

    def adam(self, w, m, v, g, lr, weight_decay=0.0):
        """TensorFlow's Adam on fp32 variables from the UNSCALED gradient with this record's bias correction (fp64
        arithmetic, one rounding per stored value); the record itself moves in update()."""
        w64 = w.astype(np.float64)
        g64 = g.astype(np.float64) + weight_decay * w64
        m = (R.BETA1 * m.astype(np.float64) + (1.0 - R.BETA1) * g64).astype(np.float32)
        v = (R.BETA2 * v.astype(np.float64) + (1.0 - R.BETA2) * (g64 * g64)).astype(np.float32)
        w = (w64 - self.lr_t(lr) * m.astype(np.float64) / (np.sqrt(v.astype(np.float64)) + R.EPSILON)).astype(np.float32)
        return w, m, v

    def step(self, w, m, v, g_scaled, lr, weight_decay=0.0):
        """One guarded update of one buffer from the SCALED gradient: returns (w, m, v), unchanged on overflow."""
        g, overflow = self.unscale(g_scaled)
        if not overflow:
            w, m, v = self.adam(w, m, v, g, lr, weight_decay)
        self.update(overflow)
        return w, m, v
