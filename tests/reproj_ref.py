"""Restatements of the reprojection loss of DESIGN.md 6i (kfnet_amd/reproj.py, kfnet_amd/csrc/kfn_reproj.hip), test
infrastructure only:

    reproj_loss      KFNet.ReprojectionLoss (KFNet/KFNet.py:405-428) in its masked form, in torch, differentiable, fp64 unless
                     the inputs say otherwise
    closed_gradient  d(rho)/d(x) by the closed form of DESIGN.md 6i, numpy fp64
    pixel_map32      the augmented pixel map in numpy float32, in the kernel's operation order: what kfn_augment_pixel_map must
                     equal bit for bit
    pixel_map64      the same built as the reference builds it, in fp64 passes: the plain map, rotate (NEAREST), resample
"""
import numpy as np
import torch

from augment_ref import F, _gather32, resample64, rotate64
from kfnet_amd.augment import TRANSLATE, descriptor

FLOOR = 1e-12


def pose_matrices64(poses, G=None):
    """[B,3,4] fp64: the first three rows of inv(pose_b) inv(G)."""
    Gi = np.eye(4) if G is None else np.linalg.inv(np.asarray(G, dtype=np.float64))
    return np.stack([(np.linalg.inv(np.asarray(p, dtype=np.float64)) @ Gi)[:3] for p in poses])


def analytic_rays(h, w, camera, dtype=np.float64):
    """[h,w,2]: ((8c - u) / fx, (8r - v) / fy) with the constants the device gets: u, v, float32(1 / fx), float32(1 / fy)."""
    u, v = np.float32(camera.u), np.float32(camera.v)
    ifx, ify = np.float32(1.0 / camera.fx), np.float32(1.0 / camera.fy)
    r, c = np.meshgrid(np.arange(h) * 8, np.arange(w) * 8, indexing='ij')
    if dtype == np.float32:
        return np.stack([(c.astype(F) - u) * ifx, (r.astype(F) - v) * ify], -1)
    return np.stack([(c - float(u)) * float(ifx), (r - float(v)) * float(ify)], -1)


def l2_normalize(a):
    """tf.nn.l2_normalize: a * rsqrt(max(sum a^2, 1e-12))."""
    s = (a * a).sum(-1, keepdim=True)
    return a * torch.rsqrt(torch.clamp(s, min=FLOOR))


def reproj_loss(x, M, rays, mask, valid=None):
    """x [B,h,w,3] torch; M [B,3,4], rays [h,w,2] (or [B,h,w,2]), mask [B,h,w] (0/1) numpy or torch.  Returns (R, rho [B,h,w])
    in x's dtype: R = sum(mask rho) / (valid + 1), valid = sum(mask) + 1 unless given."""
    dt = x.dtype
    M = torch.as_tensor(np.asarray(M), dtype=dt) if not torch.is_tensor(M) else M.to(dt)
    q = torch.as_tensor(np.asarray(rays), dtype=dt) if not torch.is_tensor(rays) else rays.to(dt)
    m = torch.as_tensor(np.asarray(mask), dtype=dt) if not torch.is_tensor(mask) else mask.to(dt)
    cam = torch.einsum('bij,bhwj->bhwi', M[:, :, :3], x) + M[:, None, None, :, 3]
    q = torch.cat([q, torch.ones_like(q[..., :1])], -1)
    e = l2_normalize(cam) - l2_normalize(q)
    rho = (e * e).sum(-1)
    if valid is None:
        valid = m.sum() + 1.0
    return (m * rho).sum() / (valid + 1.0), rho


def closed_gradient(x, M, rays):
    """d(rho)/d(x) [B,h,w,3] in numpy fp64 by the closed form: (2 / sqrt(s)) (n (n . nq) - nq) above the floor, 2e6 e at or
    below it, then M[:, :3]^T."""
    x, M, q = np.asarray(x, np.float64), np.asarray(M, np.float64), np.asarray(rays, np.float64)
    cam = np.einsum('bij,bhwj->bhwi', M[:, :, :3], x) + M[:, None, None, :, 3]
    q = np.concatenate([q, np.ones_like(q[..., :1])], -1)
    nq = q / np.sqrt(np.maximum((q * q).sum(-1, keepdims=True), FLOOR))
    s = (cam * cam).sum(-1, keepdims=True)
    above = s > FLOOR
    inv = np.where(above, 1.0 / np.sqrt(np.where(above, s, 1.0)), 1e6)
    n = cam * inv
    g = np.where(above, 2.0 * inv * (n * (n * nq).sum(-1, keepdims=True) - nq), 2.0e6 * (n - nq))
    return np.einsum('bij,bhwi->bhwj', M[:, :, :3], g)


# ---- the augmented pixel map ---------------------------------------------------------------------------------------------
def plain_map32(H, W, camera):
    """[1,H,W,2] float32: ((float(x) - u) inv_fx, (float(y) - v) inv_fy), each operation rounded."""
    u, v = F(camera.u), F(camera.v)
    ifx, ify = F(1.0 / camera.fx), F(1.0 / camera.fy)
    y, x = np.meshgrid(np.arange(H).astype(F), np.arange(W).astype(F), indexing='ij')
    out = np.stack([(x - u) * ifx, (y - v) * ify], -1)[None]
    assert out.dtype == F
    return out


def pixel_map32(params, H, W, camera, stride=8):
    """[H/s,W/s,2] float32.  A gathered entry of the plain map IS the analytic value at the gathered pixel, so the label
    path of augment_ref on the plain map restates the kernel."""
    d = descriptor(params, 1, H, W, stride)
    val, _ = _gather32(plain_map32(H, W, camera), d, np.arange(0, H, stride), np.arange(0, W, stride))
    return np.ascontiguousarray(val[0])


def pixel_map64(params, H, W, camera):
    """([H,W,2] fp64 at full resolution, ambiguous [H,W]): the plain map with the device's constants, through rotate64 and
    resample64 as data_augmentation's bundle goes (KFNet/train.py:181-187)."""
    u, v = float(F(camera.u)), float(F(camera.v))
    ifx, ify = float(F(1.0 / camera.fx)), float(F(1.0 / camera.fy))
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    pm = np.stack([(x - u) * ifx, (y - v) * ify], -1)[None]
    if params.mode == TRANSLATE:
        return pm[0], np.zeros((H, W), bool)
    rot, amb = rotate64(pm, params.angle)
    out, touched = resample64(rot, params, amb)
    return out[0], touched
