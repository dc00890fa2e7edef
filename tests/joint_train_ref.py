"""Reference of joint stage 3 (kfnet_amd/train_kfnet.py with train_flownet), test infrastructure only: the
composition of the two restatements that exist.  tests/flow_train_ref.py supplies OFlowNet's forward pass up to
(flow, sigma_trans), tests/kf_train_ref.py the sampler, the loss and the filter's arithmetic; here the filter is restated with
flow and sigma_trans as tensors, so that autograd -- in fp64 unless told otherwise -- differentiates by them and, through them,
by Temporal/*.  And a float32 numpy restatement of the two formulas kfn_filter_backward_joint adds, in its order of
operations."""
import contextlib

import numpy as np
import torch

import flow_train_ref as FR
import kf_train_ref as KR
import train_ref as R

EPS2 = KR.EPS2


def pair_table(S, T):
    """(a_idx, b_idx): pair s (T - 1) + t - 1 = frames (s T + t - 1, s T + t), t = 1 .. T - 1 -- written out, not imported."""
    a, b = [], []
    for s in range(S):
        for t in range(1, T):
            a.append(s * T + t - 1)
            b.append(s * T + t)
    return np.array(a, dtype=np.int64), np.array(b, dtype=np.int64)


def tensor(a, dtype, grad=False):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dtype).requires_grad_(grad)


def filter_forward(meas, flow, sigma_trans):
    """KR.filter_forward with flow [S,T,h,w,2] and sigma_trans [S,T,h,w] as torch tensors of meas's dtype (frame 0's are
    ignored): KR.sampler passes the gradient to the coordinates through its weights, its corner indices come from floor."""
    S, T, h, w, _ = meas.shape
    pm = KR.pixel_map(h, w, meas.dtype)
    temps, kfs = [meas[:, 0]], [meas[:, 0]]
    for t in range(1, T):
        warped = KR.sampler(kfs[-1], pm + flow[:, t])
        lx, ls = warped[..., 0:3], warped[..., 3:4]
        last_var = torch.clamp(ls * ls, min=EPS2)
        trans_var = torch.clamp(sigma_trans[:, t][..., None] ** 2, min=EPS2)
        su = torch.sqrt(trans_var + last_var)
        z, sz = meas[:, t, ..., 0:3], meas[:, t, ..., 3:4]
        lv, mv = su * su, sz * sz
        K = lv / (lv + mv)
        om = torch.clamp(1.0 - K, min=0.0)
        temps.append(torch.cat([lx, su], -1))
        kfs.append(torch.cat([om * lx + K * z, torch.sqrt(om * lv)], -1))
    return torch.stack(temps, 1), torch.stack(kfs, 1)


def backward_grads(pred, flow, st, d_temp, d_kf, dtype=torch.float64):
    """(d_pred, d_flow, d_sigma_trans) of sum(d_temp temp + d_kf kf) through the filter, numpy fp64, by autograd in `dtype`.
    Frame 0's flow and sigma_trans receive zeros."""
    p, fl, s = tensor(pred, dtype, True), tensor(flow, dtype, True), tensor(st, dtype, True)
    temp, kf = filter_forward(KR.measurement(p), fl, s)
    obj = (temp * tensor(d_temp, dtype)).sum() + (kf * tensor(d_kf, dtype)).sum()
    grads = torch.autograd.grad(obj, [p, fl, s])
    return [g.to(torch.float64).numpy() for g in grads]


# -- the two formulas, as the device orders them ---------------------------------------------------------------------------------
def taps(flow, h, w):
    """The forward's clamped corners and weights in float32: (ix0, ix1, iy0, iy1, wx0, wx1, wy0, wy1), each [h,w]."""
    f = np.float32
    ys, xs = np.meshgrid(np.arange(h, dtype=f), np.arange(w, dtype=f), indexing='ij')
    px, py = xs + flow[..., 0].astype(f), ys + flow[..., 1].astype(f)
    x0, y0 = np.floor(px), np.floor(py)
    x0s, x1s = np.clip(x0, 0, w - 1), np.clip(x0 + f(1), 0, w - 1)
    y0s, y1s = np.clip(y0, 0, h - 1), np.clip(y0 + f(1), 0, h - 1)
    return (x0s.astype(int), x1s.astype(int), y0s.astype(int), y1s.astype(int), x1s - px, px - x0s, y1s - py, py - y0s)


def flow_sigma_grads(prev, flow, st, g_x, d_lvar):
    """Float32, unfused, in kfn_filter_backward_joint's order.  prev [h,w,4] = KF_{t-1}; flow [h,w,2]; st [h,w]; g_x [h,w,3] the
    gradient with respect to the sampled coordinates; d_lvar [h,w] the gradient with respect to sigma^-^2.  Returns
    (d_flow [h,w,2], d_sigma_trans [h,w], s_l [h,w])."""
    f = np.float32
    prev, st, g_x, d_lvar = (np.asarray(a, dtype=f) for a in (prev, st, g_x, d_lvar))
    h, w, _ = prev.shape
    ix0, ix1, iy0, iy1, wx0, wx1, wy0, wy1 = taps(np.asarray(flow, dtype=f), h, w)
    v00, v01, v10, v11 = prev[iy0, ix0], prev[iy1, ix0], prev[iy0, ix1], prev[iy1, ix1]
    s_l = (((wx0 * wy0) * v00[..., 3] + (wx0 * wy1) * v01[..., 3]) + (wx1 * wy0) * v10[..., 3]) + (wx1 * wy1) * v11[..., 3]
    av = np.empty((h, w, 4), f)
    av[..., :3] = g_x
    av[..., 3] = np.where(s_l * s_l > f(EPS2), d_lvar * (f(2) * s_l), f(0))
    gu = wy0[..., None] * (v10 - v00) + wy1[..., None] * (v11 - v01)
    gv = wx0[..., None] * (v01 - v00) + wx1[..., None] * (v11 - v10)
    du = ((av[..., 0] * gu[..., 0] + av[..., 1] * gu[..., 1]) + av[..., 2] * gu[..., 2]) + av[..., 3] * gu[..., 3]
    dv = ((av[..., 0] * gv[..., 0] + av[..., 1] * gv[..., 1]) + av[..., 2] * gv[..., 2]) + av[..., 3] * gv[..., 3]
    ds = np.where(st * st > f(EPS2), d_lvar * (f(2) * st), f(0))
    return np.stack([du, dv], -1), ds, s_l


def warp_objective(prev, flow, st, g_x, d_lvar):
    """sum(g_x . x^-) + sum(d_lvar sigma^-^2) of one frame, torch: what flow_sigma_grads differentiates."""
    h, w, _ = prev.shape
    warped = KR.sampler(prev[None], KR.pixel_map(h, w, prev.dtype) + flow[None])[0]
    var = torch.clamp(warped[..., 3] ** 2, min=EPS2) + torch.clamp(st ** 2, min=EPS2)
    return (warped[..., :3] * g_x).sum() + (var * d_lvar).sum()


# -- the whole step -------------------------------------------------------------------------------------------------------------
def flow_forward(frames_u8, Wf, S, T):
    """OFlowNet on the S (T - 1) overlapping pairs of S groups of T frames, the tower once per frame.  Returns (flow [S,T,h,w,2],
    sigma_trans [S,T,h,w]) with zeros in slot 0 of every group."""
    f = FR.l2_normalize(FR.tower(frames_u8, Wf))
    _, h, w, _ = f.shape
    a, b = pair_table(S, T)
    _, flow, st = FR.flow_head(*FR.unet(FR.coord_volume(f[a], f[b]), Wf))
    flow, st = flow.reshape(S, T - 1, h, w, 2), st.reshape(S, T - 1, h, w)
    return (torch.cat([torch.zeros_like(flow[:, :1]), flow], 1), torch.cat([torch.zeros_like(st[:, :1]), st], 1))


def loss_and_grads(frames_u8, labels, Wnp, S, T, M=None, loss_clip=None, smooth_weight=50.0, dtype=torch.float64,
                   train_flownet=True):
    """(stats dict, {name: gradient fp64}, flow [S,T,h,w,2] fp64) of a joint step's data loss with respect to ScoreNet/* and
    Temporal/* (train_flownet=False: flow and sigma_trans detached, Temporal/* left out), by autograd in `dtype`."""
    Ws = {k: tensor(v, dtype, True) for k, v in Wnp.items() if k.startswith('ScoreNet/')}
    Wf = FR.tensors(Wnp, dtype, grad=train_flownet)
    flow, st = flow_forward(frames_u8, Wf, S, T)
    pred = R.network(frames_u8, Ws)
    B, h, w, _ = pred.shape
    temp, kf = filter_forward(KR.measurement(pred).reshape(S, T, h, w, 4), flow, st)
    L, s, terms = KR.filter_loss(pred, temp.reshape(B, h, w, 4), kf.reshape(B, h, w, 4), R.grid_labels(labels, (h, w)),
                                 np.asarray(frames_u8)[:, ::8, ::8][:, :h, :w], M, loss_clip, smooth_weight)
    W = dict(Ws)
    if train_flownet:
        W.update(Wf)
    names = sorted(W)
    grads = torch.autograd.grad(L, [W[n] for n in names])
    stats = dict(loss=L.item(), l_measure=terms[0].item(), l_temp=terms[1].item(), l_KF=terms[2].item(), a_measure=s[7].item(),
                 a_temp=s[8].item(), a_KF=s[9].item(), pixels=s[10].item() - 1.0)
    return stats, {n: g.detach().to(torch.float64).numpy() for n, g in zip(names, grads)}, flow.detach().to(torch.float64).numpy()


@contextlib.contextmanager
def recorded_relu_inputs(out):
    """While active, every torch.nn.functional.relu appends min |input| to `out`: the two restatements call it by that name."""
    import torch.nn.functional as F
    plain = F.relu

    def relu(x, *args, **kw):
        out.append(float(x.detach().abs().min()))
        return plain(x, *args, **kw)
    F.relu = relu
    try:
        yield out
    finally:
        F.relu = plain


def smallest_preactivation(frames_u8, Wnp, S, T):
    """The smallest fp64 |pre-activation| over every ReLU unit of both networks on these frames: the figure by which the seeds
    of the whole-step tests are chosen (DESIGN.md 6f's rule)."""
    seen = []
    with torch.no_grad(), recorded_relu_inputs(seen):
        flow_forward(frames_u8, FR.tensors(Wnp, torch.float64), S, T)
        R.network(frames_u8, {k: tensor(v, torch.float64) for k, v in Wnp.items() if k.startswith('ScoreNet/')})
    return min(seen)
