"""Restatements of DESIGN.md 6d (training labels from depth maps and poses) for tests/test_labels_host.py and
tests/test_gpu_labels.py, and the small writers and generators those tests share.

labels32  the operation list in numpy float32, one rounded operation per line: what kfn_depth_labels must equal bit for bit.
labels64  the same geometry in fp64 from the unrounded inputs (pose entries, 1/fx, 0.001 as Python doubles).
bound     the derived distance between the two, below.

The bound, with u = 2**-24 = eps32 / 2 the unit round-off and every test camera's principal point an fp32 number (so x - u
and y - v are exact: small integers minus an fp32 number of the same magnitude):
    z   = f32(raw) * scale32         scale32 = 0.001 (1 + d), one product                      -> relative error 2u
    X   = ((x - u) * inv_fx32) * z   inv_fx32 = (1 / fx)(1 + d), two products, z's 2u           -> 5u
    Y   likewise                                                                               -> 5u
    w_i = ((P0 X + P1 Y) + P2 z) + t, every P and t rounded to fp32 once (1u each):
          P0 X and P1 Y carry 5u + 1u + 1u (product) = 7u, + 1u per following sum, three sums   -> 10u
          P2 z carries 2u + 1u + 1u = 4u, + two sums                                            -> 6u
          t carries 1u + the last sum                                                           -> 2u
so |w32_i - w64_i| <= 10u (|P_i0 X| + |P_i1 Y| + |P_i2 z|) + 2u |t_i| to first order.  `bound` returns
6 eps32 (sum_j |P_ij| |p_j| + |t_i|): 12u on every term, the slack over 10u covering the second-order products.  By
Cauchy-Schwarz that is at most 6 eps32 (|R_i| |p| + |t_i|), a few eps32 (|R| |p| + |t|).
"""
import struct
import zlib

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)


def round_half_away(t):
    """C's round() / roundf(): halves away from zero.  t - trunc(t) is exact in either format."""
    r = np.trunc(t)
    return r + np.sign(t) * (np.abs(t - r) >= 0.5).astype(t.dtype)


def constants(cam, dtype):
    """The constants of the operation list: the fp64 expressions, rounded once to `dtype`."""
    f = dtype
    return dict(u=f(cam.u), v=f(cam.v), inv_fx=f(1.0 / cam.fx), inv_fy=f(1.0 / cam.fy), kx=f(cam.depth_fx / cam.fx),
                ky=f(cam.depth_fy / cam.fy), ud=f(cam.depth_u), vd=f(cam.depth_v), scale=f(cam.scale))


def depth_pixels(cam, H, W, stride, dtype):
    """(x [w], y [h]) colour pixels of the output grid and (xd [w], yd [h], ok_x [w], ok_y [h]): their depth pixels."""
    k = constants(cam, dtype)
    x = np.arange(0, W, stride)
    y = np.arange(0, H, stride)
    if not cam.register:
        return x, y, x.copy(), y.copy(), np.ones(x.size, bool), np.ones(y.size, bool)
    xd = round_half_away((x.astype(dtype) - k['u']) * k['kx'] + k['ud'])
    yd = round_half_away((y.astype(dtype) - k['v']) * k['ky'] + k['vd'])
    ok_x = (xd >= 0) & (xd <= W - 1)
    ok_y = (yd >= 0) & (yd <= H - 1)
    return x, y, np.where(ok_x, xd, 0).astype(np.int64), np.where(ok_y, yd, 0).astype(np.int64), ok_x, ok_y


def _gather(depth, cam, stride, dtype):
    B, H, W = depth.shape
    x, y, xd, yd, ok_x, ok_y = depth_pixels(cam, H, W, stride, dtype)
    raw = depth[:, yd[:, None], xd[None, :]].astype(np.int64)
    valid = (ok_y[:, None] & ok_x[None, :])[None] & (raw >= cam.raw_min) & (raw <= cam.raw_max)
    return x, y, raw, valid


def labels32(depth, poses, cam, stride):
    """depth uint16 [B,H,W], poses [B,4,4] (any float type) -> float32 [B,H/stride,W/stride,4], every operation in float32."""
    f = np.float32
    k = constants(cam, f)
    x, y, raw, valid = _gather(depth, cam, stride, f)
    P = np.asarray(poses, dtype=np.float64)[:, :3, :].astype(f)
    xf = (x.astype(f) - k['u']) * k['inv_fx']
    yf = (y.astype(f) - k['v']) * k['inv_fy']
    out = np.zeros(raw.shape + (4,), dtype=f)
    for b in range(depth.shape[0]):
        z = raw[b].astype(f) * k['scale']
        X = xf[None, :] * z
        Y = yf[:, None] * z
        assert z.dtype == f and X.dtype == f and Y.dtype == f
        for i in range(3):
            t = P[b, i, 0] * X + P[b, i, 1] * Y
            t = t + P[b, i, 2] * z
            t = t + P[b, i, 3]
            assert t.dtype == f
            out[b, ..., i] = np.where(valid[b], t, f(0))
        out[b, ..., 3] = valid[b].astype(f)
    return out


def camera_points64(depth, cam, stride):
    """(X, Y, z) [B,h,w,3] in fp64 and the validity mask."""
    x, y, raw, valid = _gather(depth, cam, stride, np.float64)
    z = raw.astype(np.float64) * cam.scale
    X = ((x - cam.u) / cam.fx)[None, None, :] * z
    Y = ((y - cam.v) / cam.fy)[None, :, None] * z
    return np.stack([X, Y, z], axis=-1), valid


def labels64(depth, poses, cam, stride):
    p, valid = camera_points64(depth, cam, stride)
    P = np.asarray(poses, dtype=np.float64)
    w = np.einsum('bij,bhwj->bhwi', P[:, :3, :3], p) + P[:, None, None, :3, 3]
    out = np.zeros(p.shape[:3] + (4,), dtype=np.float64)
    out[..., :3] = np.where(valid[..., None], w, 0.0)
    out[..., 3] = valid
    return out


def bound(depth, poses, cam, stride):
    """[B,h,w,3]: 6 eps32 (sum_j |P_ij| |p_j| + |t_i|), the module docstring's derivation."""
    p, _ = camera_points64(depth, cam, stride)
    P = np.abs(np.asarray(poses, dtype=np.float64))
    return 6.0 * EPS32 * (np.einsum('bij,bhwj->bhwi', P[:, :3, :3], np.abs(p)) + P[:, None, None, :3, 3])


def moments64(labels, pivot):
    """(sums [B,10], sums of |term| [B,10], counts [B]) of kfn_label_moments' ten sums per frame, in fp64 (numpy's pairwise
    order)."""
    lab = np.asarray(labels)
    B = lab.shape[0]
    sums, mags, counts = np.zeros((B, 10)), np.zeros((B, 10)), np.zeros(B, dtype=np.int64)
    for b in range(B):
        q = lab[b].reshape(-1, lab.shape[-1])
        d = q[q[:, 3] == 1.0, :3].astype(np.float64) - np.asarray(pivot, dtype=np.float64)
        terms = [np.ones(d.shape[0]), d[:, 0], d[:, 1], d[:, 2], d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2],
                 d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]]
        sums[b] = [t.sum() for t in terms]
        mags[b] = [np.abs(t).sum() for t in terms]
        counts[b] = d.shape[0]
    return sums, mags, counts


# ---- generators ----------------------------------------------------------------------------------------------------------
def random_pose(rng, centre_scale=2.0):
    """A random rigid camera-to-world pose [4,4] fp64: a proper rotation from the QR of a normal matrix, a normal centre."""
    Q, R = np.linalg.qr(rng.normal(size=(3, 3)))
    Q = Q * np.sign(np.diag(R))
    if np.linalg.det(Q) < 0:
        Q[:, 2] *= -1.0
    T = np.eye(4)
    T[:3, :3] = Q
    T[:3, 3] = centre_scale * rng.normal(size=3)
    return T


def random_depth(rng, B, H, W):
    """Random raw values over the whole uint16 range with the two invalid codes 0 and 65535 mixed in (about one pixel in
    eight each)."""
    d = rng.integers(1, 65535, size=(B, H, W)).astype(np.uint16)
    pick = rng.random((B, H, W))
    d[pick < 0.125] = 0
    d[pick > 0.875] = 65535
    return d


def plane_depth(H, W, cam, planes):
    """uint16 [H,W] depth of a few tilted planes z = a + b x' + c y' (x', y' normalised pixel coordinates), one plane per
    vertical band, in millimetres."""
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    xn, yn = (xs - cam.u) / cam.fx, (ys - cam.v) / cam.fy
    out = np.zeros((H, W))
    band = np.minimum(xs * len(planes) // W, len(planes) - 1)
    for k, (a, b, c) in enumerate(planes):
        out = np.where(band == k, a + b * xn + c * yn, out)
    return np.clip(np.rint(out * 1000.0), 1, 65534).astype(np.uint16)


# ---- a 16-bit PNG writer ---------------------------------------------------------------------------------------------------
def chunk(tag, body):
    return struct.pack('>I', len(body)) + tag + body + struct.pack('>I', zlib.crc32(tag + body) & 0xffffffff)


def filter_row(ft, cur, prev, bpp):
    """forward filter of the PNG specification (section 9.2) on one row of bytes"""
    out = bytearray(len(cur))
    for i in range(len(cur)):
        a = cur[i - bpp] if i >= bpp else 0
        b = prev[i] if prev is not None else 0
        c = prev[i - bpp] if (prev is not None and i >= bpp) else 0
        if ft == 0:
            pred = 0
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = b
        elif ft == 3:
            pred = (a + b) // 2
        else:
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
        out[i] = (cur[i] - pred) & 255
    return bytes(out)


def png_bytes(rows, width, ctype, depth, filters, idat_pieces=1, interlace=0):
    """rows: packed scanlines (bytes); filters: one filter type per row"""
    channels = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
    bpp = max(1, channels * depth // 8)
    raw, prev = b'', None
    for r, ft in zip(rows, filters):
        raw += bytes([ft]) + filter_row(ft, r, prev, bpp)
        prev = r
    z = zlib.compress(raw, 6)
    cut = [len(z) * k // idat_pieces for k in range(idat_pieces + 1)]
    data = b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', width, len(rows), depth, ctype, 0, 0, interlace))
    data += chunk(b'tEXt', b'Comment\x00hand-built')          # an ancillary chunk in front of the data
    for k in range(idat_pieces):
        data += chunk(b'IDAT', z[cut[k]:cut[k + 1]])
    return data + chunk(b'IEND', b'')


def write_png16(path, a, filters=None, idat_pieces=1):
    """uint16 [H,W] -> a non-interlaced 16-bit gray PNG (big-endian samples); filters default to type 1 (sub) on every row."""
    a = np.asarray(a)
    assert a.dtype == np.uint16 and a.ndim == 2
    rows = [a[y].astype('>u2').tobytes() for y in range(a.shape[0])]
    filters = [1] * a.shape[0] if filters is None else filters
    with open(path, 'wb') as f:
        f.write(png_bytes(rows, a.shape[1], 0, 16, filters, idat_pieces))


def write_pose_txt(path, T):
    with open(path, 'w') as f:
        for row in np.asarray(T, dtype=np.float64).reshape(4, 4):
            f.write('\t'.join('%.9e' % x for x in row) + '\t\n')


def write_sequence(folder, depth, poses, frames=None):
    """A 7-Scenes sequence folder: frame-%06d.color.png (8-bit RGB), .depth.png (16-bit gray), .pose.txt."""
    B, H, W = depth.shape
    for i in range(B):
        stem = '%s/frame-%06d.' % (folder, i)
        rgb = np.zeros((H, W, 3), np.uint8) if frames is None else frames[i]
        with open(stem + 'color.png', 'wb') as f:
            f.write(png_bytes([rgb[y].tobytes() for y in range(H)], W, 2, 8, [0] * H))
        write_png16(stem + 'depth.png', depth[i])
        write_pose_txt(stem + 'pose.txt', poses[i])
