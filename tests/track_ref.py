"""Restatement of the kfn_track_* launches (include/kfnet_hip.h) in numpy, written from the header's text.

The live maps, the ray cast and the per-pixel ICP rows are numpy float32, operation by operation in the header's order, so
they reproduce the device's bits.  The 29 sums are math.fsum over the exact fp64 products; solve, exponential and commit
are numpy fp64.  Tracker puts them together on top of fuse_ref.integrate.  Nothing of the product path is imported.
"""
import math

import numpy as np

import fuse_ref as F

f32 = np.float32
SUMS = 29
TRAJ_LD = 20
MAX_STEPS = 8191
PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]


class Params(object):
    """The tracking constants of kfn_track_desc, rounded to fp32 where the descriptor holds floats."""

    def __init__(self, levels=3, iterations=(10, 5, 4), far=8.0, min_weight=1.0, pyr_dist=0.1, jump=0.1, dist_max=0.1,
                 angle_max=20.0, min_pairs=50, pivot_floor=1e-10, min_share=0.1, max_rms=0.04, max_step_m=0.3, max_step_rad=0.35):
        r = lambda x: float(f32(x))
        self.levels, self.iterations = int(levels), tuple(int(x) for x in iterations)
        assert len(self.iterations) == self.levels
        self.far, self.min_weight, self.pyr_dist, self.jump, self.dist_max = r(far), r(min_weight), r(pyr_dist), r(jump), r(dist_max)
        self.angle_max, self.cos_min = float(angle_max), r(math.cos(math.radians(angle_max)))
        self.min_pairs, self.pivot_floor = int(min_pairs), r(pivot_floor)
        self.min_share, self.max_rms, self.max_step_m, self.max_step_rad = r(min_share), r(max_rms), r(max_step_m), r(max_step_rad)


def levels_of(S, count):
    """[(H, W, offset, fx, fy, cu, cv)] of the levels: the size halves (floor), f = f 0.5, c = (c - 0.5) 0.5, in fp32."""
    H, W = S.image_size
    fx, fy, cu, cv, off = f32(S.dfx), f32(S.dfy), f32(S.du), f32(S.dv), 0
    out = []
    for l in range(count):
        out.append((H, W, off, fx, fy, cu, cv))
        off += H * W
        H, W = H // 2, W // 2
        fx, fy = fx * f32(0.5), fy * f32(0.5)
        cu, cv = (cu - f32(0.5)) * f32(0.5), (cv - f32(0.5)) * f32(0.5)
    return out


def map_size(S, count):
    return sum(l[0] * l[1] for l in levels_of(S, count))


def _normalised(cx, cy, cz, ok):
    ln = np.sqrt((cx * cx + cy * cy) + cz * cz)
    ok = ok & (ln > 0) & np.isfinite(ln)
    out = np.zeros(cx.shape + (4,), dtype=f32)
    for k, c in enumerate((cx, cy, cz)):
        out[..., k] = np.where(ok, c / ln, f32(0))
    out[..., 3] = ok.astype(f32)
    return out


def live_maps(depth, S, T):
    """depth uint16 [H,W] -> (live_v, live_n) float32 [sum H_l W_l, 4]."""
    depth = np.asarray(depth)
    lv = levels_of(S, T.levels)
    assert depth.dtype == np.uint16 and depth.shape == (lv[0][0], lv[0][1])
    V, N = [], []
    old = np.seterr(all='ignore')
    try:
        z, ok = None, None
        for l, (H, W, off, fx, fy, cu, cv) in enumerate(lv):
            if l == 0:
                raw = depth.astype(np.int64)
                ok = (raw >= S.raw_min) & (raw <= S.raw_max)
                z = raw.astype(f32) * f32(S.scale)
            else:
                zs = [z[dy:2 * H:2, dx:2 * W:2] for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
                oks = [ok[dy:2 * H:2, dx:2 * W:2] for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
                zmin = np.full((H, W), np.finfo(f32).max, dtype=f32)
                for zk, okk in zip(zs, oks):
                    zmin = np.where(okk, np.fmin(zmin, zk), zmin)
                total, cnt = np.zeros((H, W), dtype=f32), np.zeros((H, W), dtype=f32)
                for zk, okk in zip(zs, oks):
                    take = okk & (zk - zmin <= f32(T.pyr_dist))
                    total = np.where(take, total + zk, total)
                    cnt = np.where(take, cnt + f32(1), cnt)
                ok = oks[0] | oks[1] | oks[2] | oks[3]
                z = total / cnt
            v = np.zeros((H, W, 4), dtype=f32)
            xs, ys = np.arange(W).astype(f32)[None, :], np.arange(H).astype(f32)[:, None]
            v[..., 0] = np.where(ok, ((xs - cu) / fx) * z, f32(0))
            v[..., 1] = np.where(ok, ((ys - cv) / fy) * z, f32(0))
            v[..., 2] = np.where(ok, z, f32(0))
            v[..., 3] = ok.astype(f32)
            z = v[..., 2]
            # normals
            c, r, d = v[:-1, :-1], v[:-1, 1:], v[1:, :-1]
            good = (c[..., 3] != 0) & (r[..., 3] != 0) & (d[..., 3] != 0)
            good &= (np.abs(r[..., 2] - c[..., 2]) <= f32(T.jump)) & (np.abs(d[..., 2] - c[..., 2]) <= f32(T.jump))
            ax, ay, az = d[..., 0] - c[..., 0], d[..., 1] - c[..., 1], d[..., 2] - c[..., 2]
            bx, by, bz = r[..., 0] - c[..., 0], r[..., 1] - c[..., 1], r[..., 2] - c[..., 2]
            n = np.zeros((H, W, 4), dtype=f32)
            n[:-1, :-1] = _normalised(ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx, good)
            V.append(v.reshape(-1, 4))
            N.append(n.reshape(-1, 4))
    finally:
        np.seterr(**old)
    return np.concatenate(V), np.concatenate(N)


def _sample(tsdf, dims, gx, gy, gz, min_weight):
    nx, ny, nz = dims
    x0, y0, z0 = np.floor(gx), np.floor(gy), np.floor(gz)
    ok = (x0 >= 0) & (x0 <= f32(nx - 2)) & (y0 >= 0) & (y0 <= f32(ny - 2)) & (z0 >= 0) & (z0 <= f32(nz - 2))
    xi, yi, zi = (np.where(ok, c, 0).astype(np.int64) for c in (x0, y0, z0))
    d = dict()
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                e = tsdf[zi + dz, yi + dy, xi + dx]
                d[dx, dy, dz] = e[..., 0]
                ok = ok & (e[..., 1] >= f32(min_weight))
    a, b, c = gx - x0, gy - y0, gz - z0
    c00 = d[0, 0, 0] + a * (d[1, 0, 0] - d[0, 0, 0])
    c10 = d[0, 1, 0] + a * (d[1, 1, 0] - d[0, 1, 0])
    c01 = d[0, 0, 1] + a * (d[1, 0, 1] - d[0, 0, 1])
    c11 = d[0, 1, 1] + a * (d[1, 1, 1] - d[0, 1, 1])
    c0 = c00 + b * (c10 - c00)
    c1 = c01 + b * (c11 - c01)
    return ok, c0 + c * (c1 - c0)


def raycast(tsdf, committed, S, T, level):
    """-> (model_v, model_n) float32 [H_l W_l, 4] of one level, from the committed pose (12 doubles)."""
    H, W, off, fx, fy, cu, cv = levels_of(S, T.levels)[level]
    tsdf = np.asarray(tsdf, dtype=f32)
    P = np.asarray(committed, dtype=np.float64).reshape(12).astype(f32)
    nx, ny, nz = S.dims
    vox = f32(S.voxel)
    old = np.seterr(all='ignore')
    try:
        xs = np.tile(np.arange(W).astype(f32), H)
        ys = np.repeat(np.arange(H).astype(f32), W)
        qx, qy = (xs - cu) / fx, (ys - cv) / fy
        wx = (P[0] * qx + P[1] * qy) + P[2]
        wy = (P[4] * qx + P[5] * qy) + P[6]
        wz = (P[8] * qx + P[9] * qy) + P[10]
        ln = np.sqrt((qx * qx + qy * qy) + f32(1))
        dt = (f32(S.trunc) * f32(0.5)) / ln
        gc = [(P[3] - f32(S.origin[0])) / vox, (P[7] - f32(S.origin[1])) / vox, (P[11] - f32(S.origin[2])) / vox]
        gd = [wx / vox, wy / vox, wz / vox]
        tmin = np.full(H * W, f32(S.near), dtype=f32)
        tmax = np.full(H * W, f32(T.far), dtype=f32)
        for k, n in enumerate((nx, ny, nz)):
            inv = f32(1) / gd[k]
            a, b = (f32(0) - gc[k]) * inv, (f32(n - 1) - gc[k]) * inv
            tmin, tmax = np.fmax(tmin, np.fmin(a, b)), np.fmin(tmax, np.fmax(a, b))
        kf = np.floor((tmax - tmin) / dt)
        valid = np.isfinite(P).all() & (tmin < tmax) & (kf >= 0)
        kmax = np.where(valid, np.fmin(kf, f32(MAX_STEPS)), -1).astype(np.int64)
        positive = np.zeros(H * W, dtype=bool)
        done, hit = ~valid, np.zeros(H * W, dtype=bool)
        Dp, tp, Dc, tc = (np.zeros(H * W, dtype=f32) for _ in range(4))
        for k in range(int(kmax.max()) + 1 if valid.any() else 0):
            act = ~done & (k <= kmax)
            if not act.any():
                break
            t = tmin + f32(k) * dt
            ok, D = _sample(tsdf, S.dims, gc[0] + t * gd[0], gc[1] + t * gd[1], gc[2] + t * gd[2], T.min_weight)
            pos, neg = act & ok & (D > 0), act & ok & (D < 0)
            Dp, tp = np.where(pos, D, Dp), np.where(pos, t, tp)
            hit = hit | (neg & positive)
            Dc, tc = np.where(neg, D, Dc), np.where(neg, t, tc)
            done = done | neg
            positive = np.where(act, pos, positive)
        ts = tp + (Dp / (Dp - Dc)) * (tc - tp)
        v = np.zeros((H * W, 4), dtype=f32)
        v[:, 0] = np.where(hit, P[3] + ts * wx, f32(0))
        v[:, 1] = np.where(hit, P[7] + ts * wy, f32(0))
        v[:, 2] = np.where(hit, P[11] + ts * wz, f32(0))
        v[:, 3] = hit.astype(f32)
        g = [gc[k] + ts * gd[k] for k in range(3)]
        good, grad = hit.copy(), []
        for k in range(3):
            hi = [g[j] + (f32(1) if j == k else f32(0)) for j in range(3)]
            lo = [g[j] - (f32(1) if j == k else f32(0)) for j in range(3)]
            okp, Dq = _sample(tsdf, S.dims, hi[0], hi[1], hi[2], T.min_weight)
            okm, Dm = _sample(tsdf, S.dims, lo[0], lo[1], lo[2], T.min_weight)
            good &= okp & okm
            grad.append(Dq - Dm)
        n = _normalised(grad[0], grad[1], grad[2], good)
    finally:
        np.seterr(**old)
    return v, n


def icp_rows(live_v, live_n, model_v, model_n, estimate, committed, S, T, level):
    """The per-pixel rows of one level (the maps are the whole pyramids): -> (J float32 [n,6], r float32 [n]) of the accepted
    pairs, in pixel order."""
    H, W, off, fx, fy, cu, cv = levels_of(S, T.levels)[level]
    E = np.asarray(estimate, dtype=np.float64).reshape(12).astype(f32)
    C = np.asarray(committed, dtype=np.float64).reshape(12).astype(f32)
    v, nl = live_v[off:off + H * W], live_n[off:off + H * W]
    old = np.seterr(all='ignore')
    try:
        ok = (v[:, 3] != 0) & (nl[:, 3] != 0)
        px = ((E[0] * v[:, 0] + E[1] * v[:, 1]) + E[2] * v[:, 2]) + E[3]
        py = ((E[4] * v[:, 0] + E[5] * v[:, 1]) + E[6] * v[:, 2]) + E[7]
        pz = ((E[8] * v[:, 0] + E[9] * v[:, 1]) + E[10] * v[:, 2]) + E[11]
        dx, dy, dz = px - C[3], py - C[7], pz - C[11]
        X = (C[0] * dx + C[4] * dy) + C[8] * dz
        Y = (C[1] * dx + C[5] * dy) + C[9] * dz
        Z = (C[2] * dx + C[6] * dy) + C[10] * dz
        ok &= np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & ~(Z < f32(S.near))
        cf, rf = np.rint((X / Z) * fx + cu), np.rint((Y / Z) * fy + cv)
        ok &= (cf >= 0) & (cf <= f32(W - 1)) & (rf >= 0) & (rf <= f32(H - 1))
        at = off + np.where(ok, rf, 0).astype(np.int64) * W + np.where(ok, cf, 0).astype(np.int64)
        m, n = model_v[at], model_n[at]
        ok &= (m[:, 3] != 0) & (n[:, 3] != 0)
        ex, ey, ez = m[:, 0] - px, m[:, 1] - py, m[:, 2] - pz
        ok &= np.sqrt((ex * ex + ey * ey) + ez * ez) <= f32(T.dist_max)
        rx = (E[0] * nl[:, 0] + E[1] * nl[:, 1]) + E[2] * nl[:, 2]
        ry = (E[4] * nl[:, 0] + E[5] * nl[:, 1]) + E[6] * nl[:, 2]
        rz = (E[8] * nl[:, 0] + E[9] * nl[:, 1]) + E[10] * nl[:, 2]
        ok &= ((rx * n[:, 0] + ry * n[:, 1]) + rz * n[:, 2]) >= f32(T.cos_min)
        r = (n[:, 0] * ex + n[:, 1] * ey) + n[:, 2] * ez
        J = np.stack([py * n[:, 2] - pz * n[:, 1], pz * n[:, 0] - px * n[:, 2], px * n[:, 1] - py * n[:, 0],
                      n[:, 0], n[:, 1], n[:, 2]], axis=1)
    finally:
        np.seterr(**old)
    return J[ok].astype(f32), r[ok].astype(f32)


def icp_sums(J, r, exact=True):
    """The 29 sums of the rows -> (sums fp64 [29], the sums of the terms' magnitudes [29]).  The terms are exact in fp64."""
    J64, r64 = J.astype(np.float64), r.astype(np.float64)
    terms = [J64[:, a] * J64[:, b] for a, b in PAIRS] + [J64[:, a] * r64 for a in range(6)] + [r64 * r64, np.ones(len(r64))]
    add = math.fsum if exact else (lambda t: float(np.sum(t)))
    return np.array([add(t) for t in terms]), np.array([math.fsum(np.abs(t)) for t in terms])


def new_state(pose):
    p = np.asarray(pose, dtype=np.float64)
    p = p[:3, :].reshape(12) if p.shape == (4, 4) else p.reshape(12)
    return dict(committed=p.copy(), estimate=p.copy(), last_share=0.0, last_rms=0.0, last_pairs=0.0, frame=1, lost=0, accepted=0,
                iterations=0)


def pose_of(row):
    P = np.eye(4)
    P[:3, :] = np.asarray(row, dtype=np.float64).reshape(3, 4)
    return P


def twist_exp(xi):
    """exp of the twist (omega, upsilon) as the header states it -> (R [3,3], t [3])."""
    w, u = np.asarray(xi[:3], dtype=np.float64), np.asarray(xi[3:], dtype=np.float64)
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = math.sqrt(th2)
    if th < 1e-4:
        A, B, C = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        A = math.sin(th) / th
        B = 2.0 * math.sin(0.5 * th) ** 2 / th2
        C = (1.0 - A) / th2
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    K2 = K @ K
    return np.eye(3) + A * K + B * K2, (np.eye(3) + B * K + C * K2) @ u


def solve(sums, pivot_floor):
    """Cholesky of the 6 x 6 system as the header states it -> xi, or None when a pivot fails or xi is not finite."""
    A, b = np.zeros((6, 6)), np.asarray(sums[21:27], dtype=np.float64)
    for s, (i, j) in enumerate(PAIRS):
        A[i, j] = A[j, i] = sums[s]
    L = np.zeros((6, 6))
    for j in range(6):
        d = A[j, j] - float(np.dot(L[j, :j], L[j, :j]))
        if not (d > pivot_floor * A[j, j]) or not np.isfinite(d):
            return None
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - float(np.dot(L[i, :j], L[j, :j]))) / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (b[i] - float(np.dot(L[i, :i], y[:i]))) / L[i, i]
    xi = np.zeros(6)
    for i in range(5, -1, -1):
        xi[i] = (y[i] - float(np.dot(L[i + 1:, i], xi[i + 1:]))) / L[i, i]
    return xi if np.isfinite(xi).all() else None


def orthonormalise(R):
    a, b = R[:, 0] / np.linalg.norm(R[:, 0]), R[:, 1]
    b = b - np.dot(a, b) * a
    b = b / np.linalg.norm(b)
    return np.stack([a, b, np.cross(a, b)], axis=1)


def update(sums, st, pixels, T):
    """kfn_track_update on the record `st` (a dict, changed in place) -> True when the iteration was accepted."""
    count = float(sums[28])
    st['last_pairs'], st['last_share'] = count, count / float(pixels)
    st['last_rms'] = math.sqrt(sums[27] / count) if count > 0 else 0.0
    st['iterations'] += 1
    if not count >= T.min_pairs:
        return False
    old = np.seterr(all='ignore')
    try:
        xi = solve(sums, T.pivot_floor)
        if xi is None:
            return False
        Ri, ti = twist_exp(xi)
        E = st['estimate'].reshape(3, 4)
        N = np.concatenate([orthonormalise(Ri @ E[:, :3]), (Ri @ E[:, 3] + ti)[:, None]], axis=1)
    finally:
        np.seterr(**old)
    if not np.isfinite(N).all():
        return False
    st['estimate'] = N.reshape(12)
    st['accepted'] += 1
    return True


def commit(st, T):
    """kfn_track_commit -> (pose row float32 [12], trajectory row fp64 [20]); the record is changed in place."""
    E, C = st['estimate'].reshape(3, 4), st['committed'].reshape(3, 4)
    step_m = float(np.linalg.norm(E[:, 3] - C[:, 3]))
    step_rad = math.acos(min(max((float(np.sum(E[:, :3] * C[:, :3])) - 1.0) * 0.5, -1.0), 1.0)) if np.isfinite(E).all() else np.nan
    tracked = bool(np.isfinite(E).all() and st['accepted'] > 0 and st['last_share'] >= T.min_share and st['last_rms'] <= T.max_rms and
                   step_m <= T.max_step_m and step_rad <= T.max_step_rad)
    row = np.zeros(TRAJ_LD)
    if tracked:
        st['committed'] = st['estimate'].copy()
        pose_row = st['estimate'].astype(f32)
        row[:12] = st['estimate']
    else:
        st['estimate'] = st['committed'].copy()
        st['lost'] += 1
        pose_row = np.full(12, np.nan, dtype=f32)
        row[:12] = np.nan
    row[12:20] = (0.0 if tracked else 1.0, st['last_pairs'], st['last_share'], st['last_rms'], st['accepted'], st['iterations'],
                  step_m, step_rad)
    st['frame'] += 1
    st['accepted'] = st['iterations'] = 0
    return pose_row, row


class Tracker(object):
    """The whole tracker on the CPU: start(pose, depth), push(depth) per frame, trajectory()."""

    def __init__(self, S, T, exact_sums=False):
        self.S, self.T, self.exact = S, T, exact_sums
        self.tsdf = S.empty(False)[0]
        self.rows, self.state, self.first = [], None, None

    def start(self, pose, depth):
        self.first = np.asarray(pose, dtype=np.float64).reshape(4, 4).copy()
        self.state = new_state(self.first)
        self.tsdf, _ = F.integrate(self.tsdf, None, np.asarray(depth)[None], None, self.first[None], self.S)

    def push(self, depth):
        S, T, st = self.S, self.T, self.state
        lv = levels_of(S, T.levels)
        live_v, live_n = live_maps(depth, S, T)
        mv, mn = np.zeros_like(live_v), np.zeros_like(live_n)
        for l, (H, W, off, _, _, _, _) in enumerate(lv):
            mv[off:off + H * W], mn[off:off + H * W] = raycast(self.tsdf, st['committed'], S, T, l)
        for l in range(T.levels - 1, -1, -1):
            for _ in range(T.iterations[l]):
                J, r = icp_rows(live_v, live_n, mv, mn, st['estimate'], st['committed'], S, T, l)
                update(icp_sums(J, r, self.exact)[0], st, lv[l][0] * lv[l][1], T)
        pose_row, row = commit(st, T)
        self.rows.append(row)
        self.tsdf, _ = F.integrate(self.tsdf, None, np.asarray(depth)[None], None, pose_row[None], S)
        return row

    def trajectory(self):
        """-> (poses [N,4,4] fp64 with frame 0 first, lost bool [N], diagnostics [N,8])."""
        rows = np.array(self.rows).reshape(-1, TRAJ_LD)
        poses = np.stack([self.first] + [pose_of(r[:12]) for r in rows])
        return poses, np.concatenate([[False], rows[:, 12] != 0]), np.concatenate([np.zeros((1, 8)), rows[:, 12:20]])


def pose_errors(est, truth):
    """(translation error in metres, rotation error in degrees) per frame of poses [N,4,4]."""
    est, truth = np.asarray(est, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    dt = np.linalg.norm(est[:, :3, 3] - truth[:, :3, 3], axis=1)
    M = np.einsum('nji,njk->nik', est[:, :3, :3], truth[:, :3, :3])
    skew = 0.5 * np.stack([M[:, 2, 1] - M[:, 1, 2], M[:, 0, 2] - M[:, 2, 0], M[:, 1, 0] - M[:, 0, 1]], axis=1)
    cos = (np.trace(M, axis1=1, axis2=2) - 1.0) * 0.5
    return dt, np.degrees(np.arctan2(np.linalg.norm(skew, axis=1), cos))


# ---- the shared sequence of the CPU and the GPU tests ---------------------------------------------------------------------------
SEQ_H, SEQ_W = 64, 96
SEQ_CAM = dict(fx=78.75, fy=78.75, u=48., v=32.)            # RT_CAM of tests/test_gpu_fuse.py
SEQ_VOXEL = 0.04
SEQ_DIMS, SEQ_ORIGIN = (106, 81, 69), (-0.1, -0.1, -0.1)   # the volume of test_round_trip_through_the_renderer
SEQ_FRAMES = 12
SEQ_PHASE_STEP = 0.03                                       # synthetic_trajectory's is 0.12: a quarter of its speed


def sequence_setup():
    return F.Setup(dims=SEQ_DIMS, origin=SEQ_ORIGIN, voxel=SEQ_VOXEL, image_size=(SEQ_H, SEQ_W), **SEQ_CAM)


def sequence_trajectory(count=SEQ_FRAMES, seed=3, step=SEQ_PHASE_STEP):
    """synthetic_trajectory's path through synthetic_scene's room, walked at `step` rad of phase a frame."""
    rng = np.random.default_rng([seed, 0x7a9ec])
    phase = rng.uniform(0.0, 2.0 * np.pi, size=6)
    out = np.zeros((count, 4, 4), dtype=np.float64)
    for i in range(count):
        a = step * i
        pos = np.array([1.05 + 0.5 * np.sin(a + phase[0]), 1.5 + 0.85 * np.sin(0.7 * a + phase[1]), 1.3 + 0.3 * np.sin(0.5 * a + phase[2])])
        target = np.array([3.0 + 0.2 * np.sin(0.3 * a + phase[3]), 1.5 + 0.5 * np.sin(0.4 * a + phase[4]),
                           0.6 + 0.2 * np.sin(0.6 * a + phase[5])])
        fwd = (target - pos) / np.linalg.norm(target - pos)
        right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
        right /= np.linalg.norm(right)
        out[i, :3, 0], out[i, :3, 1], out[i, :3, 2], out[i, :3, 3] = right, np.cross(fwd, right), fwd, pos
        out[i, 3, 3] = 1.0
    return out
