"""Reference of training OFlowNet (stage 2), test infrastructure only: a differentiable torch restatement of the
Temporal scope -- the feature tower with l2_normalize, the cost volume, the window U-Net with its two heads
(cnn_wrapper/OFlowNet.py:17-57, KFNet/KFNet.py:315-403) -- and of the loss of stage 2, generic over dtype and differentiated by
autograd; and float32 restatements with sequential adds of the two gather sums of kfn_cost_volume_backward.  The values in
fp32 are those of oracle.kfnet_oracle_torch's oflow_feat / coord_volume / oflownet / process_model."""
import numpy as np
import torch
import torch.nn.functional as F

import kf_train_ref as KR
from oracle.kfnet_oracle_torch import FEAT, conv_same, deconv_same

MIN_UNCERTAINTY = KR.MIN_UNCERTAINTY
EPS2 = KR.EPS2                                                  # float32(1e-5 * 1e-5), the double product rounded once
THR2_BITS = 0x3B23D70A                                          # float32(0.05 * 0.05)
WINDOW = 8
OFFSETS = np.array([(j - 4, i - 4) for i in range(WINDOW) for j in range(WINDOW)], dtype=np.float64)   # (x, y) of cell k = 8 i + j
S = 'Temporal'


def tensors(Wnp, dtype, grad=False):
    return {k: torch.from_numpy(np.asarray(v, dtype=np.float64)).to(dtype).requires_grad_(grad) for k, v in Wnp.items()
            if k.startswith(S + '/')}


def _kb(W, name):
    return W['%s/%s/kernel' % (S, name)], W.get('%s/%s/bias' % (S, name))


# -- forward -----------------------------------------------------------------------------------------------------------------
def tower(frames_u8, W):
    """feat1 .. feat7 on uint8 frames [B,H,W,3]: [B,h,w,32] before the normalisation.  W's dtype rules."""
    dt = W[S + '/feat1/kernel'].dtype
    x = torch.from_numpy(np.ascontiguousarray(frames_u8)).to(dt).permute(0, 3, 1, 2)
    x = (x - 128.0) * 0.00625
    for name, s, relu in FEAT:
        x = conv_same(x, *_kb(W, name), s, relu)
    return x.permute(0, 2, 3, 1)


def l2_normalize(x):
    ss = (x * x).sum(-1, keepdim=True)
    return x * torch.rsqrt(torch.clamp(ss, min=1e-12))


def coord_volume(f_a, f_b):
    """vol[p,i,j,c] = f_b[p,c] - f_a[p + (i-4, j-4), c], 0 outside: [P h w, 8, 8, C], differentiable in both."""
    P, h, w, Cc = f_a.shape
    half = WINDOW // 2
    pad = F.pad(f_a, (0, 0, half, half, half, half))
    diffs = []
    for i in range(WINDOW):
        for j in range(WINDOW):
            diffs.append(f_b - pad[:, i:i + h, j:j + w])        # pad row half + (y + i - half)
    return torch.stack(diffs, 3).reshape(-1, WINDOW, WINDOW, Cc)


def unet(vol, W):
    """(logits [N,64], pre [N]): 'prediction' over the window and fc(conv3b) before exp, as oracle oflownet computes them."""
    x = vol.permute(0, 3, 1, 2).contiguous()        # the oracle's memory format: the conv engine chooses its kernel by it
    c0 = conv_same(x, *_kb(W, 'conv0'), 1, True)
    c1a = conv_same(c0, *_kb(W, 'conv1a'), 2, True)
    c1b = conv_same(c1a, *_kb(W, 'conv1b'), 1, True)
    c2a = conv_same(c1b, *_kb(W, 'conv2a'), 2, True)
    c2b = conv_same(c2a, *_kb(W, 'conv2b'), 1, True)
    c3a = conv_same(c2b, *_kb(W, 'conv3a'), 2, True)
    c3b = conv_same(c3a, *_kb(W, 'conv3b'), 1, True)
    u2 = deconv_same(c3b, *_kb(W, 'upconv2'), 2, True)
    c4 = conv_same(torch.cat([u2, c2b], 1), *_kb(W, 'conv4'), 1, True)
    u1 = deconv_same(c4, *_kb(W, 'upconv1'), 2, True)
    c5 = conv_same(torch.cat([u1, c1b], 1), *_kb(W, 'conv5'), 1, True)
    u0 = deconv_same(c5, *_kb(W, 'upconv0'), 2, True)
    c6 = conv_same(torch.cat([u0, c0], 1), *_kb(W, 'conv6'), 1, True)
    pr = conv_same(c6, *_kb(W, 'prediction'), 1, False)
    n = x.shape[0]
    feat = c3b.reshape(n, -1)
    k1, b1 = _kb(W, 'fc1')
    k2, b2 = _kb(W, 'fc2')
    k3, b3 = _kb(W, 'uncertainty')
    f1 = F.relu(feat @ k1 + b1)
    f2 = F.relu(f1 @ k2 + b2)
    return pr[:, 0].reshape(n, -1), (f2 @ k3 + b3).reshape(n)


def flow_head(logits, pre):
    """(prob [N,64], flow [N,2] = (u, v), sigma_trans [N])."""
    prob = torch.softmax(logits, dim=-1)
    flow = prob @ torch.from_numpy(OFFSETS).to(logits.dtype)
    return prob, flow, torch.exp(pre) * 1e-2


def forward(frames_u8, W):
    """Frames [2P,H,W,3], pair p = (2p, 2p + 1) = (a, b).  Returns (prob, flow [P,h,w,2], sigma_trans [P,h,w])."""
    f = l2_normalize(tower(frames_u8, W))
    _, h, w, _ = f.shape
    prob, flow, st = flow_head(*unet(coord_volume(f[0::2], f[1::2]), W))
    return prob, flow.reshape(-1, h, w, 2), st.reshape(-1, h, w)


# -- the loss ------------------------------------------------------------------------------------------------------------------
def warp_labels(flow, labels_grid):
    """(x^- [P,h,w,3], valid_a [P,h,w], m_b [P,h,w]): label a's coordinates through KR.sampler at (x + u, y + v); valid_a = the
    four UNCLAMPED corners lie in the grid and have m_a = 1.  Differentiable in flow through the sampler's weights."""
    dt = flow.dtype
    lab = torch.from_numpy(np.asarray(labels_grid, dtype=np.float64)).to(dt)
    la, lb = lab[0::2], lab[1::2]
    P, h, w, _ = la.shape
    coords = KR.pixel_map(h, w, dt) + flow
    # KR.sampler takes coords as they are: its corner indices come from floor, piecewise constant, autograd passes the weights
    xm = KR.sampler(la[..., 0:3], coords)
    with torch.no_grad():
        x0 = torch.floor(coords[..., 0]); y0 = torch.floor(coords[..., 1])
        inside = (x0 >= 0) & (x0 + 1 <= w - 1) & (y0 >= 0) & (y0 + 1 <= h - 1)
        xi = x0.clamp(0, w - 2).to(torch.int64); yi = y0.clamp(0, h - 2).to(torch.int64)
        ma = (la[..., 3] == 1.0).reshape(P, h * w)
        base = yi * w + xi
        corners = [torch.gather(ma, 1, (base + o).reshape(P, -1)).reshape(P, h, w) for o in (0, 1, w, w + 1)]
        valid_a = (inside & corners[0] & corners[1] & corners[2] & corners[3]).to(dt)
        m_b = (lb[..., 3] == 1.0).to(dt)
    return xm, valid_a, m_b


def flow_loss(flow, sigma_trans, labels_grid, loss_clip=None, dist_threshold=0.05):
    """flow [P,h,w,2], sigma_trans [P,h,w] torch; labels_grid [2P,h,w,4].  Returns (L, accuracy, valid = sum M + 1,
    #{valid_a == 0}) as torch scalars."""
    dt = flow.dtype
    gb = torch.from_numpy(np.asarray(labels_grid, dtype=np.float64)).to(dt)[1::2, ..., 0:3]
    xm, valid_a, m_b = warp_labels(flow, labels_grid)
    M = m_b * valid_a
    eps2 = torch.tensor(EPS2, dtype=dt)
    sm = torch.sqrt(eps2 + torch.maximum(sigma_trans * sigma_trans, eps2))
    u = torch.clamp(sm, min=MIN_UNCERTAINTY)
    d = ((xm - gb) ** 2).sum(-1)
    l = 3.0 * torch.log(u) + d / (2.0 * u * u)
    if loss_clip is not None:
        l = torch.minimum(l, torch.tensor(loss_clip, dtype=dt))
    valid = M.sum() + 1.0
    # where M = 0 the warp may have left the grid: the cell adds nothing, whatever l holds
    L = torch.where(M > 0, l, torch.zeros_like(l)).sum() / valid
    bad = ((M * d - dist_threshold * dist_threshold) > 0).to(dt).sum()
    return L, (valid - bad) / valid, valid, (valid_a == 0).to(dt).sum()


def loss_grads(flow, sigma_trans, labels_grid, loss_clip=None, dtype=torch.float64):
    """(stats [L, accuracy, valid, lost], d_flow, d_sigma) by autograd in `dtype` from numpy inputs."""
    fl = torch.from_numpy(np.asarray(flow, dtype=np.float64)).to(dtype).requires_grad_(True)
    st = torch.from_numpy(np.asarray(sigma_trans, dtype=np.float64)).to(dtype).requires_grad_(True)
    out = flow_loss(fl, st, labels_grid, loss_clip)
    gf, gs = torch.autograd.grad(out[0], [fl, st], allow_unused=True)
    gf = torch.zeros_like(fl) if gf is None else gf
    gs = torch.zeros_like(st) if gs is None else gs
    return [o.item() for o in out], gf.to(torch.float64).numpy(), gs.to(torch.float64).numpy()


def step_loss_and_grads(frames_u8, labels_grid, Wnp, loss_clip=None, dtype=torch.float64):
    """(L, {name: gradient fp64}) of the whole step's data loss with respect to every Temporal/* variable."""
    W = tensors(Wnp, dtype, grad=True)
    _, flow, st = forward(frames_u8, W)
    L = flow_loss(flow, st, labels_grid, loss_clip)[0]
    names = sorted(W)
    grads = torch.autograd.grad(L, [W[n] for n in names])
    return L.item(), {n: g.detach().to(torch.float64).numpy() for n, g in zip(names, grads)}


# -- the two gather sums of kfn_cost_volume_backward --------------------------------------------------------------------------
def cost_volume_backward(d_vol, grid, dtype=np.float32):
    """d_vol [P h w, 8, 8, C] -> (d_f2, d_f1) [P,h,w,C], each element a sum that starts from 0 and adds its cells one by one in
    `dtype`, i then j ascending; d_f1 skips the cells outside the frame and negates the finished sum.  In float32 this is the
    device's order of operations."""
    P, h, w = grid
    v = np.asarray(d_vol).astype(dtype).reshape(P, h, w, WINDOW, WINDOW, -1)
    d_f2 = np.zeros((P, h, w, v.shape[-1]), dtype)
    d_f1 = np.zeros_like(d_f2)
    for i in range(WINDOW):
        for j in range(WINDOW):
            d_f2 += v[:, :, :, i, j]
            dy, dx = i - WINDOW // 2, j - WINDOW // 2          # cell p = q - (dy, dx) reads f_a[q] at (i, j)
            y0, y1 = max(0, dy), min(h, h + dy)
            x0, x1 = max(0, dx), min(w, w + dx)
            if y1 > y0 and x1 > x0:
                d_f1[:, y0:y1, x0:x1] += v[:, y0 - dy:y1 - dy, x0 - dx:x1 - dx, i, j]
    return d_f2, -d_f1


def rel_err(g, g64):
    """max |g - g64| / max |g64| (0 / 0 = 0)."""
    g64 = np.asarray(g64, dtype=np.float64)
    top = float(np.abs(np.asarray(g, dtype=np.float64) - g64).max())
    scale = float(np.abs(g64).max())
    return top / scale if scale > 0 else top
