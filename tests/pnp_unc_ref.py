"""numpy fp64 restatement of kfn_pnp_ransac_unc and kfn_pose_filter (DESIGN.md 5c "Uncertainty"), on top of pnp_ref.

Test infrastructure only: the product path never imports it.  Candidates, sampling, P3P, scoring and selection are
pnp_ref's; this module adds the measurement covariance S_i, the weighted Gauss-Newton refinement, the pose covariance and
quality, the error-state pose filter, and the synthetic frames and trajectories the tests share.

Conventions: (R, t) maps world to camera; Sigma is in the coordinates (omega, tau) of its left perturbation
R <- exp(omega) R, t <- exp(omega) t + tau, which to first order is the covariance of the body-frame perturbation
(dtheta, drho) = -(omega, tau) of the camera-to-world pose [R^T | -R^T t].
"""
import math

import numpy as np

import pnp_ref as P

UPDATED, MISSING, REJECTED, INIT, NONE = 0, 1, 2, 3, 4


def candidate_sigma(rec, min_confidence=20.0):
    """sigma = 1 / record[3] of the candidates, in pnp_ref.candidates' (raster) order."""
    rec = np.asarray(rec, dtype=np.float32)
    keep = (rec[..., 3] > np.float32(min_confidence)) & np.isfinite(rec[..., :3]).all(axis=-1)
    return 1.0 / rec[..., 3][keep].astype(np.float64)


def weights(R, t, X, sigma, fx, fy, pixel_sigma):
    """S_i^-1 = (w00, w01, w11) of S_i = sigma_i^2 A_i A_i^T + pixel_sigma^2 I at pose (R, t)."""
    Xc = X @ R.T + t
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    iz = 1.0 / z
    a0, a2 = fx * iz, -fx * x * iz * iz
    b1, b2 = fy * iz, -fy * y * iz * iz
    s2, p2 = sigma * sigma, pixel_sigma * pixel_sigma
    s00 = s2 * (a0 * a0 + a2 * a2) + p2
    s01 = s2 * (a2 * b2)
    s11 = s2 * (b1 * b1 + b2 * b2) + p2
    idet = 1.0 / (s00 * s11 - s01 * s01)
    return s11 * idet, -s01 * idet, s00 * idet


def _jacobians(R, t, X, pix, fx, fy, u, v):
    Xc = X @ R.T + t
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    iz = 1.0 / z
    ru = fx * x * iz - (pix[:, 0] - u)
    rv = fy * y * iz - (pix[:, 1] - v)
    a0, a2 = fx * iz, -fx * x * iz * iz
    b1, b2 = fy * iz, -fy * y * iz * iz
    zero = np.zeros_like(x)
    Ju = np.stack([a2 * y, a0 * z - a2 * x, -a0 * y, a0, zero, a2], axis=1)
    Jv = np.stack([-b1 * z + b2 * y, -b2 * x, b1 * x, zero, b1, b2], axis=1)
    return Ju, Jv, ru, rv


def weighted_system(R, t, X, pix, sigma, fx, fy, u, v, pixel_sigma):
    """H = sum J^T S^-1 J, g = sum J^T S^-1 r, cost = sum r^T S^-1 r over all the given points."""
    Ju, Jv, ru, rv = _jacobians(R, t, X, pix, fx, fy, u, v)
    w00, w01, w11 = weights(R, t, X, sigma, fx, fy, pixel_sigma)
    Wu = w00[:, None] * Ju + w01[:, None] * Jv
    Wv = w01[:, None] * Ju + w11[:, None] * Jv
    H = Wu.T @ Ju + Wv.T @ Jv
    g = Wu.T @ ru + Wv.T @ rv
    cost = float((w00 * ru * ru + 2.0 * w01 * ru * rv + w11 * rv * rv).sum())
    return H, g, cost


def refine_weighted(R, t, X, pix, sigma, fx, fy, u, v, thr, iters, pixel_sigma=1.0):
    """pnp_ref.refine with every inlier's residual weighed by S_i^-1, S_i evaluated at the current pose and held fixed
    for the iteration (also in the candidate's cost)."""
    for _ in range(iters):
        e2, Z = P.project_error2(R, t, X, pix, fx, fy, u, v)
        inl = (Z > 0.0) & (e2 < thr * thr)
        if inl.sum() < 3:
            break
        H, g, cost = weighted_system(R, t, X[inl], pix[inl], sigma[inl], fx, fy, u, v, pixel_sigma)
        try:
            L = np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            break
        d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
        dR = P.rodrigues(d[:3])
        R2, t2 = dR @ R, dR @ t + d[3:]
        Xn = X[inl] @ R2.T + t2
        if not (Xn[:, 2] > 0.0).all():
            break
        w00, w01, w11 = weights(R, t, X[inl], sigma[inl], fx, fy, pixel_sigma)
        ru = fx * Xn[:, 0] / Xn[:, 2] - (pix[inl, 0] - u)
        rv = fy * Xn[:, 1] / Xn[:, 2] - (pix[inl, 1] - v)
        cost2 = float((w00 * ru * ru + 2.0 * w01 * ru * rv + w11 * rv * rv).sum())
        if not cost2 < cost:
            break
        R, t = R2, t2
    return R, t


def covariance(R, t, X, pix, sigma, fx, fy, u, v, thr, pixel_sigma=1.0):
    """(Sigma [6,6] -- NaN with fewer than 3 inliers or H not positive definite --, weighted cost, 2 * inliers - 6,
    inliers) at pose (R, t) over its inliers."""
    inl = P.inliers(R, t, X, pix, fx, fy, u, v, thr)
    n = int(inl.sum())
    Sg = np.full((6, 6), np.nan)
    if n == 0:
        return Sg, 0.0, -6.0, 0
    H, _, cost = weighted_system(R, t, X[inl], pix[inl], sigma[inl], fx, fy, u, v, pixel_sigma)
    if n >= 3:
        try:
            Li = np.linalg.inv(np.linalg.cholesky(H))
            Sg = Li.T @ Li
        except np.linalg.LinAlgError:
            pass
    return Sg, cost, 2.0 * n - 6.0, n


def ransac_unc(records, weighted, t0=0, hypotheses_n=256, seed=0, fx=525.0, fy=525.0, u=320.0, v=240.0,
               min_confidence=20.0, inlier_px=10.0, cell_stride=8, min_points=16, refine_iters=10, pixel_sigma=1.0,
               hyps=None):
    """What kfn_pnp_ransac_unc returns: (poses [B,4,4], cov [B,6,6], quality [B,2], info [B,4]).  `hyps` (a list, filled
    on the first call and reused on the next) saves pnp_ref.hypotheses when both modes are solved on the same frames."""
    B = records.shape[0]
    poses = np.full((B, 4, 4), np.nan)
    cov = np.full((B, 6, 6), np.nan)
    quality = np.full((B, 2), np.nan)
    info = np.zeros((B, 4), np.int64)
    for b in range(B):
        if hyps is not None and len(hyps) > b:
            hp, counts, X, pix = hyps[b]
        else:
            _, hp, counts, X, pix = P.hypotheses(records[b], t0 + b, hypotheses_n, seed, fx, fy, u, v, min_confidence,
                                                 inlier_px, cell_stride, min_points)
            if hyps is not None:
                hyps.append((hp, counts, X, pix))
        n = X.shape[0]
        info[b] = (P.TOO_FEW, n, 0, -1)
        if n < max(min_points, 4):
            continue
        best = int(np.argmax(counts))
        if counts[best] < 0:
            info[b] = (P.NO_HYPOTHESIS, n, 0, -1)
            continue
        sigma = candidate_sigma(records[b], min_confidence)
        M = hp[best].reshape(3, 4)
        if weighted:
            R, t = refine_weighted(M[:, :3], M[:, 3], X, pix, sigma, fx, fy, u, v, inlier_px, refine_iters, pixel_sigma)
        else:
            R, t = P.refine(M[:, :3], M[:, 3], X, pix, fx, fy, u, v, inlier_px, refine_iters)
        poses[b] = P.cam_to_world(R, t)
        cov[b], quality[b, 0], quality[b, 1], ni = covariance(R, t, X, pix, sigma, fx, fy, u, v, inlier_px, pixel_sigma)
        info[b] = (P.OK, n, ni, best)
    return poses, cov, quality, info


def world_to_camera(T):
    """(R, t) of a camera-to-world 4x4."""
    T = np.asarray(T, np.float64)
    R = T[:3, :3].T
    return R, -R @ T[:3, 3]


def log_so3(M):
    c = ((M[0, 0] + M[1, 1] + M[2, 2]) - 1.0) / 2.0
    k = np.array([(M[2, 1] - M[1, 2]) / 2.0, (M[0, 2] - M[2, 0]) / 2.0, (M[1, 0] - M[0, 1]) / 2.0])
    s = math.sqrt(k @ k)
    return k if s < 1e-12 else math.atan2(s, c) / s * k


def body_error(est, gt):
    """(dtheta, drho) [6] with gt ~ est [exp(dtheta) | drho]: camera-to-world 4x4 poses."""
    est = np.asarray(est, np.float64)
    gt = np.asarray(gt, np.float64)
    return np.concatenate([log_so3(est[:3, :3].T @ gt[:3, :3]), est[:3, :3].T @ (gt[:3, 3] - est[:3, 3])])


def mahalanobis2(est, cov, gt):
    """Squared Mahalanobis distance of the true pose error under cov, per frame (NaN where est or cov is)."""
    out = np.full(len(est), np.nan)
    for b in range(len(est)):
        if np.isfinite(est[b]).all() and np.isfinite(cov[b]).all():
            e = body_error(est[b], gt[b])
            out[b] = float(e @ np.linalg.solve(np.asarray(cov[b], np.float64), e))
    return out


def synthetic_frames_sigma(seed, B, h, w, outliers=0.0, sigma_lo=0.005, sigma_hi=0.04, fx=525.0, fy=525.0, u=320.0, v=240.0,
                           cell_stride=8):
    """(records [B,h,w,4] float32, camera-to-world ground truth [B,4,4]): random poses; every cell has its own sigma,
    log-uniform in sigma_lo..sigma_hi (m), isotropic Gaussian noise of that sigma on its scene coordinates and
    confidence 1 / sigma; a share `outliers` of the cells replaced by points uniform in +-5 m (their confidence stays)."""
    rng = np.random.default_rng(seed)
    recs, gts = [], []
    for _ in range(B):
        R, t = P.random_pose(rng)
        rec = P.synthetic_records(rng, h, w, R, t, fx, fy, u, v, cell_stride)
        sigma = np.exp(rng.uniform(math.log(sigma_lo), math.log(sigma_hi), size=(h, w)))
        rec[..., :3] += (rng.normal(size=(h, w, 3)) * sigma[..., None]).astype(np.float32)
        rec[..., 3] = (1.0 / sigma).astype(np.float32)
        out = rng.random((h, w)) < outliers
        rec[..., :3][out] = rng.uniform(-5, 5, size=(int(out.sum()), 3)).astype(np.float32)
        recs.append(rec)
        gts.append(P.cam_to_world(R, t))
    return np.stack(recs), np.stack(gts)


def permutation_spread(R, t, X, pix, sigma, fx, fy, u, v, thr, iters, pixel_sigma=1.0, perms=5, seed=0):
    """d_perm: the largest change of (an entry of the camera-to-world pose, a normalised entry of Sigma, the relative cost)
    of refine_weighted + covariance when the candidates are listed in another order."""
    def run(Xp, pp, sp):
        Rr, tr = refine_weighted(R, t, Xp, pp, sp, fx, fy, u, v, thr, iters, pixel_sigma)
        Sg, cost, _, _ = covariance(Rr, tr, Xp, pp, sp, fx, fy, u, v, thr, pixel_sigma)
        return P.cam_to_world(Rr, tr), Sg, cost
    T0, S0, c0 = run(X, pix, sigma)
    n0 = np.sqrt(np.outer(np.diag(S0), np.diag(S0)))
    rng = np.random.default_rng(seed)
    dp = dc = 0.0
    for _ in range(perms):
        p = rng.permutation(X.shape[0])
        T1, S1, c1 = run(X[p], pix[p], sigma[p])
        dp = max(dp, float(np.abs(T1 - T0).max()))
        dc = max(dc, float((np.abs(S1 - S0) / n0).max()), abs(c1 - c0) / max(c0, 1e-300))
    return dp, dc


def rounding_spread(R, t, X, pix, sigma, fx, fy, u, v, thr, pixel_sigma=1.0):
    """d_round: the largest change of a normalised entry of Sigma and of the relative cost when the pose (as the
    camera-to-world 4x4 the device writes) is rounded to fp32 and back."""
    S0, c0, _, n0 = covariance(R, t, X, pix, sigma, fx, fy, u, v, thr, pixel_sigma)
    R1, t1 = world_to_camera(P.cam_to_world(R, t).astype(np.float32).astype(np.float64))
    S1, c1, _, n1 = covariance(R1, t1, X, pix, sigma, fx, fy, u, v, thr, pixel_sigma)
    if n0 != n1:
        return np.inf
    nrm = np.sqrt(np.outer(np.diag(S0), np.diag(S0)))
    return max(float((np.abs(S1 - S0) / nrm).max()), abs(c1 - c0) / max(c0, 1e-300))


# ---- the pose filter ------------------------------------------------------------------------------------------------

def pose_filter(poses, cov, rot_sigma=0.02, trans_sigma=0.02, gate=22.46, max_rejects=3, solve='cholesky'):
    """kfn_pose_filter on one sequence: poses [T,4,4], cov [T,6,6] (as the device reads them: fp32 values) ->
    (poses [T,4,4], cov [T,6,6], flags [T], nis [T]) in fp64.  The descriptor's floats are rounded to fp32 as the
    descriptor holds them.  solve = 'cholesky' factors S once as the device does, 'lu' uses numpy.linalg.solve."""
    poses = np.asarray(poses, np.float32).astype(np.float64)
    cov = np.asarray(cov, np.float32).astype(np.float64)
    T = poses.shape[0]
    qr = float(np.float32(rot_sigma)) ** 2
    qt = float(np.float32(trans_sigma)) ** 2
    gate = float(np.float32(gate))
    Q = np.diag([qr] * 3 + [qt] * 3)
    out_p = np.full((T, 4, 4), np.nan)
    out_c = np.full((T, 6, 6), np.nan)
    flags = np.zeros(T, np.int64)
    nis = np.full(T, np.nan)
    have, rejects = False, 0
    R = p = Pm = None
    for k in range(T):
        Z, Sz = poses[k], cov[k]
        valid = bool(np.isfinite(Z[:3]).all() and np.isfinite(Sz).all())
        init = False
        if not have:
            flag, init = (INIT, True) if valid else (NONE, False)
        else:
            Pm = Pm + Q
            flag = MISSING
            if valid:
                y = np.concatenate([log_so3(R.T @ Z[:3, :3]), R.T @ (Z[:3, 3] - p)])
                S = Pm + Sz
                try:
                    L = np.linalg.cholesky(S)
                except np.linalg.LinAlgError:
                    L = None
                if L is not None:
                    if solve == 'cholesky':
                        uu = np.linalg.solve(L, y)
                        nis[k] = float(uu @ uu)
                        K = np.linalg.solve(L.T, np.linalg.solve(L, Pm)).T
                    else:
                        nis[k] = float(y @ np.linalg.solve(S, y))
                        K = np.linalg.solve(S, Pm).T
                    if nis[k] > gate:
                        rejects += 1
                        flag = REJECTED
                        if rejects >= max_rejects:
                            flag, init = INIT, True
                    else:
                        d = K @ y
                        p = p + R @ d[3:]
                        R = R @ P.rodrigues(d[:3])
                        A = np.eye(6) - K
                        Pm = A @ Pm @ A.T + K @ Sz @ K.T
                        Pm = np.triu(Pm) + np.triu(Pm, 1).T            # the device mirrors the upper triangle
                        flag, rejects = UPDATED, 0
        if init:
            R, p, Pm = Z[:3, :3].copy(), Z[:3, 3].copy(), Sz.copy()
            have, rejects = True, 0
        if have:
            out_p[k] = np.eye(4)
            out_p[k, :3, :3], out_p[k, :3, 3] = R, p
            out_c[k] = Pm
        flags[k] = flag
    return out_p, out_c, flags, nis


def synthetic_trajectory(seed, T=200, missing=0.1, wrong=0.05, lead_missing=0, step_rot=0.01, step_trans=0.01,
                         meas_rot=0.004, meas_trans=0.025):
    """A random-walk camera trajectory and its measurements: (gt [T,4,4], measured poses [T,4,4] float32 -- NaN where
    missing --, cov [T,6,6] float32, kind [T]: 0 good, 1 missing, 2 wrong).  A good measurement is the truth perturbed in
    its body frame by a draw from its own covariance (a random SPD matrix of about meas_rot rad / meas_trans m per axis);
    a wrong one is off by 0.5-1 m and 0.2-0.5 rad and claims an ordinary covariance.  The frame after a wrong one is good,
    so no planted run forces a re-initialisation; the first `lead_missing` frames are missing."""
    rng = np.random.default_rng(seed)
    R, t = P.random_pose(rng)
    C = P.cam_to_world(R, t)
    gt = np.zeros((T, 4, 4))
    for k in range(T):
        d = np.concatenate([rng.normal(scale=step_rot, size=3), rng.normal(scale=step_trans, size=3)])
        C = C.copy()
        C[:3, 3] = C[:3, 3] + C[:3, :3] @ d[3:]
        C[:3, :3] = C[:3, :3] @ P.rodrigues(d[:3])
        gt[k] = C
    kind = np.zeros(T, np.int64)
    r = rng.random(T)
    kind[r < missing] = 1
    kind[(r >= missing) & (r < missing + wrong)] = 2
    kind[:lead_missing] = 1
    if lead_missing < T:
        kind[lead_missing] = 0
    for k in range(1, T):
        if kind[k - 1] == 2:
            kind[k] = 0
    meas = np.full((T, 4, 4), np.nan, np.float32)
    cov = np.zeros((T, 6, 6), np.float32)
    scale = np.array([meas_rot] * 3 + [meas_trans] * 3)
    for k in range(T):
        A = (np.eye(6) + 0.3 * rng.normal(size=(6, 6))) * scale[:, None]
        Sz = (A @ A.T).astype(np.float32)
        Sz = np.triu(Sz) + np.triu(Sz, 1).T
        cov[k] = Sz
        e = np.linalg.cholesky(Sz.astype(np.float64)) @ rng.normal(size=6)
        if kind[k] == 2:
            dirs = rng.normal(size=(2, 3))
            dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
            e = np.concatenate([dirs[0] * rng.uniform(0.2, 0.5), dirs[1] * rng.uniform(0.5, 1.0)])
        if kind[k] != 1:
            M = gt[k].copy()
            M[:3, 3] = M[:3, 3] + M[:3, :3] @ e[3:]
            M[:3, :3] = M[:3, :3] @ P.rodrigues(e[:3])
            meas[k] = M
    return gt, meas, cov, kind
