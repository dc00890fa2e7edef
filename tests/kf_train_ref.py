"""Reference of fine-tuning SCoordNet through the Kalman filter (kfnet_amd/train_kfnet.py), test infrastructure
only: a torch restatement of KFNet.GetKFCoordBatch (KFNet/KFNet.py:102-162), the process model's warp and variance chain
(:386-401 with tools/util.py:36-93) and the three-term loss of KFNet/train.py:286-295, differentiated by autograd -- in fp64
unless told otherwise.  Flow and sigma_trans are constants (--fix_flownet).  tests/train_ref.py supplies the network and the
single-term loss."""
import numpy as np
import torch

import train_ref as R

MIN_UNCERTAINTY = 1e-5
EPS2 = float(np.float32(MIN_UNCERTAINTY * MIN_UNCERTAINTY))     # the double product rounded once, as TensorFlow folds it
LOSS_WEIGHTS = (0.2, 0.2, 0.6)


def sampler(img, coords):
    """tools/util.py:36-93, differentiable in `img` [B,h,w,C] (torch); coords [B,h,w,2] = (x, y), a constant tensor of img's
    dtype.  Clamped corners, weights from the clamped corners, the sum in add_n order."""
    B, H, Wd, Cc = img.shape
    x, y = coords[..., 0:1], coords[..., 1:2]
    x0 = torch.floor(x); x1 = x0 + 1
    y0 = torch.floor(y); y1 = y0 + 1
    x0s = x0.clamp(0, Wd - 1); x1s = x1.clamp(0, Wd - 1)
    y0s = y0.clamp(0, H - 1); y1s = y1.clamp(0, H - 1)
    wx0 = x1s - x; wx1 = x - x0s
    wy0 = y1s - y; wy1 = y - y0s
    base = (torch.arange(B, dtype=torch.int64) * (H * Wd)).view(B, 1, 1)
    flat = img.reshape(-1, Cc)

    def g(xx, yy):
        return flat[(xx + yy * Wd).to(torch.int64)[..., 0] + base]
    out = (wx0 * wy0) * g(x0s, y0s) + (wx0 * wy1) * g(x0s, y1s)
    out = out + (wx1 * wy0) * g(x1s, y0s)
    out = out + (wx1 * wy1) * g(x1s, y1s)
    return out


def pixel_map(h, w, dtype):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing='ij')
    return torch.stack([xs, ys], -1)[None]


def filter_forward(meas, flow, sigma_trans):
    """meas [S,T,h,w,4] torch = (z, sigma_z); flow [S,T,h,w,2] and sigma_trans [S,T,h,w] numpy (frame 0's are ignored).
    Returns (temp, kf), each [S,T,h,w,4] = (x, sigma): frame 0 is the measurement (KFNet.py:122-126), frame t >= 1 BuildOFlowNet's
    tail on KF_{t-1} followed by BuildKFCoord."""
    dt = meas.dtype
    S, T, h, w, _ = meas.shape
    fl = torch.from_numpy(np.asarray(flow, dtype=np.float64)).to(dt)
    st = torch.from_numpy(np.asarray(sigma_trans, dtype=np.float64)).to(dt)
    pm = pixel_map(h, w, dt)
    temps, kfs = [meas[:, 0]], [meas[:, 0]]
    for t in range(1, T):
        warped = sampler(kfs[-1], pm + fl[:, t])
        lx, ls = warped[..., 0:3], warped[..., 3:4]
        last_var = torch.clamp(ls * ls, min=EPS2)
        trans_var = torch.clamp(st[:, t][..., None] ** 2, min=EPS2)
        su = torch.sqrt(trans_var + last_var)
        z, sz = meas[:, t, ..., 0:3], meas[:, t, ..., 3:4]
        lv, mv = su * su, sz * sz
        K = lv / (lv + mv)
        om = torch.clamp(1.0 - K, min=0.0)
        temps.append(torch.cat([lx, su], -1))
        kfs.append(torch.cat([om * lx + K * z, torch.sqrt(om * lv)], -1))
    return torch.stack(temps, 1), torch.stack(kfs, 1)


def term_loss(x, sigma, labels_grid, img_grid, M=None, loss_clip=None, smooth_weight=50.0, dist_threshold=0.05):
    """CoordLossWithUncertainty + smooth_weight SmoothLoss of one output: x [B,h,w,3], sigma [B,h,w,1] (the uncertainty
    itself).  R.coord_loss with sigma given instead of its logarithm.  Returns (L, nll, smooth, accuracy, valid)."""
    dt = x.dtype
    lab = torch.from_numpy(np.asarray(labels_grid, dtype=np.float64)).to(dt)
    gt = lab[..., 0:3]
    mask = (lab[..., 3:4] == 1.0).to(dt)
    if M is not None:
        Mt = torch.from_numpy(np.asarray(M, dtype=np.float64)).to(dt)
        gt = gt @ Mt[:3, :3].T + Mt[:3, 3]
    u = torch.clamp(sigma, min=MIN_UNCERTAINTY)
    d = ((x - gt) ** 2).sum(-1, keepdim=True)
    l = 3.0 * torch.log(u) + d / (2.0 * u * u)
    if loss_clip is not None:
        l = torch.minimum(l, torch.tensor(loss_clip, dtype=dt))
    valid = mask.sum() + 1.0
    nll = (mask * l).sum() / valid
    bad = ((mask * d - dist_threshold * dist_threshold) > 0).to(dt).sum()
    acc = (valid - bad) / valid
    smooth = torch.zeros((), dtype=dt)
    if smooth_weight != 0.0:
        img = torch.from_numpy(np.asarray(img_grid, dtype=np.float64)).to(dt)
        gx = (x[:, :, :-1] - x[:, :, 1:]).pow(2).mean(-1, keepdim=True)
        gy = (x[:, :-1] - x[:, 1:]).pow(2).mean(-1, keepdim=True)
        wx = torch.exp(-0.625 * (img[:, :, :-1] - img[:, :, 1:]).abs().mean(-1, keepdim=True))
        wy = torch.exp(-0.625 * (img[:, :-1] - img[:, 1:]).abs().mean(-1, keepdim=True))
        smooth = ((gx * wx * mask[:, :, :-1]).sum() + (gy * wy * mask[:, :-1]).sum()) / valid
    return nll + smooth_weight * smooth, nll, smooth, acc, valid


def filter_loss(pred, temp, kf, labels_grid, img_grid, M=None, loss_clip=None, smooth_weight=50.0, weights=LOSS_WEIGHTS):
    """pred [B,h,w,4] raw (channel 3 = log sigma), temp and kf [B,h,w,4] = (x, sigma).  Returns (L, stats) with stats the
    eleven numbers of kfn_filter_loss_grad's stats: L, 3 NLLs, 3 smoothness terms, 3 accuracies, valid (torch scalars)."""
    m = R.coord_loss(pred, labels_grid, img_grid, M, loss_clip, smooth_weight)
    t = term_loss(temp[..., 0:3], temp[..., 3:4], labels_grid, img_grid, M, loss_clip, smooth_weight)
    k = term_loss(kf[..., 0:3], kf[..., 3:4], labels_grid, img_grid, M, loss_clip, smooth_weight)
    L = weights[0] * m[0] + weights[1] * t[0] + weights[2] * k[0]
    return L, [L, m[1], t[1], k[1], m[2], t[2], k[2], m[3], t[3], k[3], m[4]], (m[0], t[0], k[0])


def measurement(pred):
    return torch.cat([pred[..., 0:3], torch.exp(pred[..., 3:4])], -1)


def step_loss(pred, S, T, flow, sigma_trans, labels_grid, img_grid, M=None, loss_clip=None, smooth_weight=50.0,
              weights=LOSS_WEIGHTS):
    """The whole loss of a step from the raw prediction [S T,h,w,4]: measurement, filter, three terms."""
    B, h, w, _ = pred.shape
    meas = measurement(pred).reshape(S, T, h, w, 4)
    fl = np.asarray(flow).reshape(S, T, h, w, 2)
    st = np.asarray(sigma_trans).reshape(S, T, h, w)
    temp, kf = filter_forward(meas, fl, st)
    return filter_loss(pred, temp.reshape(B, h, w, 4), kf.reshape(B, h, w, 4), labels_grid, img_grid, M, loss_clip, smooth_weight,
                       weights)


def loss_and_grads(frames_u8, labels, Wnp, S, T, flow, sigma_trans, M=None, loss_clip=None, smooth_weight=50.0,
                   dtype=torch.float64):
    """(stats dict, {name: gradient ndarray fp64}) of a step's data loss with respect to ScoreNet/*, by autograd in `dtype`."""
    W = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)).to(dtype).requires_grad_(True) for k, v in Wnp.items()
         if k.startswith('ScoreNet/')}
    pred = R.network(frames_u8, W)
    h, w = pred.shape[1:3]
    L, st, terms = step_loss(pred, S, T, flow, sigma_trans, R.grid_labels(labels, (h, w)),
                             np.asarray(frames_u8)[:, ::8, ::8][:, :h, :w], M, loss_clip, smooth_weight)
    names = sorted(W)
    grads = torch.autograd.grad(L, [W[n] for n in names])
    stats = dict(loss=L.item(), l_measure=terms[0].item(), l_temp=terms[1].item(), l_KF=terms[2].item(), a_measure=st[7].item(),
                 a_temp=st[8].item(), a_KF=st[9].item(), pixels=st[10].item() - 1.0)
    return stats, {n: g.detach().to(torch.float64).numpy() for n, g in zip(names, grads)}
