"""numpy fp64 restatement of kfn_kabsch_ransac (kfnet_amd/csrc/kfn_kabsch.hip, DESIGN.md 5c "Poses with depth").

Test infrastructure only: the product path never imports it.  The candidate rule, the counter-based sampling (pnp_ref's
hash, three distinct draws), the validity rule of a hypothesis, selection, the rounds of the closed-form refinement, the
covariance and the quality are the device's; the closed form itself is stated twice -- Horn's quaternion form with
numpy.linalg.eigh (what the device solves by Jacobi rotations) and the SVD form -- so that the reference's own
sensitivity to the algorithm, d_alg, can be measured.  The device scores in fp32, this module in fp64.

Pose convention: (R, t) maps camera to world, x = R p + t; it is the 4x4 the device returns.  Sigma is in the coordinates
(omega, tau) of the left perturbation of the world-to-camera pose (R^T, -R^T t), as pnp_unc_ref's.
"""
import math

import numpy as np

import pnp_ref as P

OK, TOO_FEW, NO_HYPOTHESIS = P.OK, P.TOO_FEW, P.NO_HYPOTHESIS
MIN_CROSS = 1e-6        # |(p1 - p0) x (p2 - p0)| below this (m^2): no hypothesis
MIN_GAP = 1e-9          # the two largest eigenvalues of Horn's matrix this close (share of the largest magnitude): degenerate
# (MIN_GAP is the project's addition to the area rule: the refinement's "degenerate set" needs a definition, and the one closed
# form serves hypotheses too.  Device and reference share it, so these tests pin the rule, not its absence from a hypothesis.)


def f32(x):
    """A descriptor's float as the device reads it."""
    return float(np.float32(x))


def draw_sample(seed, frame, hyp, n):
    """Three distinct candidate indices in draw order, or None after pnp_ref.MAX_DRAWS draws."""
    picked = []
    for draw in range(P.MAX_DRAWS):
        k = (P.sample_hash(seed, frame, hyp, draw) * n) >> 32
        if k not in picked:
            picked.append(k)
            if len(picked) == 3:
                return picked
    return None


def candidate_mask(rec, cam, min_confidence=20.0):
    rec = np.asarray(rec, dtype=np.float32)
    cam = np.asarray(cam, dtype=np.float32)
    return ((rec[..., 3] > np.float32(min_confidence)) & np.isfinite(rec[..., :3]).all(axis=-1)
            & (cam[..., 3] == np.float32(1.0)) & np.isfinite(cam[..., :3]).all(axis=-1))


def candidates(rec, cam, min_confidence=20.0):
    """rec [h,w,>=4], cam [h,w,>=4] -> (camera points [n,3], scene points [n,3], sigma^2 [n]) in raster order, fp64."""
    keep = candidate_mask(rec, cam, min_confidence)
    c = np.asarray(rec, np.float32)[..., 3][keep].astype(np.float64)
    with np.errstate(divide='ignore'):
        sig2 = 1.0 / (c * c)
    return (np.asarray(cam, np.float32)[..., :3][keep].astype(np.float64),
            np.asarray(rec, np.float32)[..., :3][keep].astype(np.float64), sig2)


# ---- the closed form ------------------------------------------------------------------------------------------------

def moments(Pc, X, w):
    """(sum w, weighted means of p and x, S = sum w (p - pbar)(x - xbar)^T)."""
    W = float(w.sum())
    pb = (w[:, None] * Pc).sum(0) / W
    xb = (w[:, None] * X).sum(0) / W
    S = (w[:, None] * (Pc - pb)).T @ (X - xb)
    return W, pb, xb, S


def quaternion_matrix(q):
    q0, qx, qy, qz = q
    return np.array([[q0 * q0 + qx * qx - qy * qy - qz * qz, 2.0 * (qx * qy - q0 * qz), 2.0 * (qx * qz + q0 * qy)],
                     [2.0 * (qx * qy + q0 * qz), q0 * q0 + qy * qy - qx * qx - qz * qz, 2.0 * (qy * qz - q0 * qx)],
                     [2.0 * (qx * qz - q0 * qy), 2.0 * (qy * qz + q0 * qx), q0 * q0 + qz * qz - qx * qx - qy * qy]])


def horn_matrix(S):
    return np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                     [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                     [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], S[1, 1] - S[0, 0] - S[2, 2], S[1, 2] + S[2, 1]],
                     [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], S[2, 2] - S[0, 0] - S[1, 1]]])


def kabsch_horn(Pc, X, w=None):
    """The (R, t) minimising sum w |R p + t - x|^2, det R = +1: the eigenvector of the largest eigenvalue of Horn's 4x4 as a
    unit quaternion.  None when the weight is not positive or the rotation is not determined (MIN_GAP)."""
    w = np.ones(len(Pc)) if w is None else w
    if not w.sum() > 0.0:
        return None
    W, pb, xb, S = moments(Pc, X, w)
    ev, V = np.linalg.eigh(horn_matrix(S))           # ascending
    if not ev[3] - ev[2] > MIN_GAP * np.abs(ev).max():
        return None
    R = quaternion_matrix(V[:, 3] / math.sqrt(V[:, 3] @ V[:, 3]))
    return R, xb - R @ pb


def kabsch_svd(Pc, X, w=None):
    """The same minimiser by the SVD of S (Kabsch; the sign of the smallest singular direction fixed so that det R = +1).
    In its terms Horn's eigenvalues are s1 + s2 + d s3, s1 - s2 - d s3, ..: the gap is 2 (s2 + d s3)."""
    w = np.ones(len(Pc)) if w is None else w
    if not w.sum() > 0.0:
        return None
    W, pb, xb, S = moments(Pc, X, w)
    U, s, Vt = np.linalg.svd(S)                      # S = sum p' x'^T = U s Vt; R = V diag(1, 1, d) U^T
    d = 1.0 if np.linalg.det(Vt.T @ U.T) > 0.0 else -1.0
    if not 2.0 * (s[1] + d * s[2]) > MIN_GAP * (s[0] + s[1] + s[2]):
        return None
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, xb - R @ pb


def jacobi_eigh4(A, sweeps=10):
    """The device's eigen-solver, restated: cyclic Jacobi on a symmetric 4x4 -> (eigenvalues, eigenvectors as columns)."""
    A = np.array(A, np.float64)
    V = np.eye(4)
    for _ in range(sweeps):
        for p in range(3):
            for q in range(p + 1, 4):
                apq = float(A[p, q])
                if apq == 0.0:
                    continue
                theta = float(A[q, q] - A[p, p]) / (2.0 * apq)       # (Python floats: theta^2 may overflow to inf, tt = 0)
                tt = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(tt * tt + 1.0)
                s = tt * c
                J = np.eye(4)
                J[p, p], J[p, q], J[q, p], J[q, q] = c, s, -s, c
                A = J.T @ A @ J
                V = V @ J
    return np.diag(A).copy(), V


def cross_norm(T):
    """|(p1 - p0) x (p2 - p0)| of a triangle [3,3]."""
    c = np.cross(T[1] - T[0], T[2] - T[0])
    return math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])


def dist2(R, t, Pc, X):
    d = Pc @ R.T + t - X
    return (d * d).sum(-1)


def inliers(R, t, Pc, X, thr):
    return dist2(R, t, Pc, X) < thr * thr


def hypothesis(Pc, X, sample, form=kabsch_horn):
    """(R, t) of the three pairs, or None: a degenerate triangle on either side, or an undetermined rotation."""
    s = list(sample)
    if cross_norm(Pc[s]) < MIN_CROSS or cross_norm(X[s]) < MIN_CROSS:
        return None
    return form(Pc[s], X[s])


def pose12(R, t):
    return np.concatenate([R, t[:, None]], axis=1).ravel()


def widen(hyp):
    """A device hypothesis [12] = [R | t] in fp32 -> (R, t) in fp64, as kabsch_refine_kernel reads it."""
    M = np.asarray(hyp, np.float32).astype(np.float64).reshape(3, 4)
    return M[:, :3].copy(), M[:, 3].copy()


def hypotheses(rec, cam, frame, H, seed=0, min_confidence=20.0, inlier_m=0.10, min_points=16, form=kabsch_horn):
    """What kfn_kabsch_hypotheses returns for one frame: samples [H,3] (-1 = none), poses [H,12] = [R | t] rounded to fp32
    (NaN = invalid), inlier counts [H] of the rounded pose (-1 = invalid); then the candidates."""
    Pc, X, sig2 = candidates(rec, cam, min_confidence)
    n = X.shape[0]
    thr = f32(inlier_m)
    samples = -np.ones((H, 3), np.int64)
    poses = np.full((H, 12), np.nan)
    counts = -np.ones(H, np.int64)
    if n < max(min_points, 3):
        return samples, poses, counts, (Pc, X, sig2)
    for k in range(H):
        s = draw_sample(seed, frame, k, n)
        if s is None:
            continue
        samples[k] = s
        hyp = hypothesis(Pc, X, s, form)
        if hyp is None:
            continue
        poses[k] = pose12(*hyp).astype(np.float32).astype(np.float64)
        counts[k] = int(inliers(*widen(poses[k]), Pc, X, thr).sum())
    return samples, poses, counts, (Pc, X, sig2)


def refine(R, t, Pc, X, w, thr, iters, form=kabsch_horn):
    """Up to `iters` rounds: the inliers of the current pose, then the weighted closed form over them.  The inlier set of
    the round before ends the loop (it would give the same pose); fewer than 3 inliers or a degenerate set keeps the pose."""
    prev = None
    for _ in range(iters):
        inl = inliers(R, t, Pc, X, thr)
        if prev is not None and np.array_equal(inl, prev):
            break
        prev = inl
        if inl.sum() < 3:
            break
        sol = form(Pc[inl], X[inl], w[inl])
        if sol is None:
            break
        R, t = sol
    return R, t


def covariance(R, t, Pc, X, sig2, thr, point_sigma=0.01):
    """(Sigma [6,6] -- NaN with fewer than 3 inliers or H not positive definite --, weighted cost, 3 * inliers - 6, inliers)
    at pose (R, t) over its inliers: H = sum w J^T J, J = [-[q]x | I], q = R^T (x - t), w = 1 / (sigma^2 + point_sigma^2)."""
    d2 = dist2(R, t, Pc, X)
    inl = d2 < thr * thr
    n = int(inl.sum())
    Sg = np.full((6, 6), np.nan)
    w = 1.0 / (sig2[inl] + f32(point_sigma) ** 2)
    q = (X[inl] - t) @ R
    J = np.zeros((n, 3, 6))
    J[:, 0, 1], J[:, 0, 2] = q[:, 2], -q[:, 1]
    J[:, 1, 0], J[:, 1, 2] = -q[:, 2], q[:, 0]
    J[:, 2, 0], J[:, 2, 1] = q[:, 1], -q[:, 0]
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
    H = np.einsum('n,nri,nrk->ik', w, J, J)
    cost = float((w * d2[inl]).sum())
    if n >= 3:
        try:
            Li = np.linalg.inv(np.linalg.cholesky(H))
            Sg = Li.T @ Li
            Sg = np.triu(Sg) + np.triu(Sg, 1).T          # the device mirrors the upper triangle
        except np.linalg.LinAlgError:
            pass
    return Sg, cost, 3.0 * n - 6.0, n


def refine_weights(sig2, weighted, point_sigma=0.01):
    return 1.0 / (sig2 + f32(point_sigma) ** 2) if weighted else np.ones_like(sig2)


def cam_to_world(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def first_max(counts):
    return P.first_max(counts)


def ransac(records, cams, weighted=False, t0=0, hypotheses_n=256, seed=0, min_confidence=20.0, inlier_m=0.10, min_points=16,
           refine_iters=10, point_sigma=0.01, hyps=None, form=kabsch_horn):
    """What kfn_kabsch_ransac returns: (poses [B,4,4], cov [B,6,6], quality [B,2], info [B,4]).  `hyps` (a list, filled on
    the first call and reused on the next) saves the hypotheses when both modes are solved on the same frames."""
    B = records.shape[0]
    poses = np.full((B, 4, 4), np.nan)
    cov = np.full((B, 6, 6), np.nan)
    quality = np.full((B, 2), np.nan)
    info = np.zeros((B, 4), np.int64)
    thr = f32(inlier_m)
    for b in range(B):
        if hyps is not None and len(hyps) > b:
            hp, counts, (Pc, X, sig2) = hyps[b]
        else:
            _, hp, counts, (Pc, X, sig2) = hypotheses(records[b], cams[b], t0 + b, hypotheses_n, seed, min_confidence,
                                                      inlier_m, min_points, form)
            if hyps is not None:
                hyps.append((hp, counts, (Pc, X, sig2)))
        n = X.shape[0]
        info[b] = (TOO_FEW, n, 0, -1)
        if n < max(min_points, 3):
            continue
        best = first_max(counts)
        if best < 0:
            info[b] = (NO_HYPOTHESIS, n, 0, -1)
            continue
        R, t = refine(*widen(hp[best]), Pc, X, refine_weights(sig2, weighted, point_sigma), thr, refine_iters, form)
        poses[b] = cam_to_world(R, t)
        cov[b], quality[b, 0], quality[b, 1], ni = covariance(R, t, Pc, X, sig2, thr, point_sigma)
        info[b] = (OK, n, ni, best)
    return poses, cov, quality, info


# ---- helpers of the tests: one stage of the device at a time against fp64 ------------------------------------------------

def threshold_margin(R, t, Pc, X, thr):
    """Smallest relative distance |dist / thr - 1| of a candidate from the inlier threshold."""
    return float(np.abs(np.sqrt(dist2(R, t, Pc, X)) / thr - 1.0).min())


def score_brackets(hyps, Pc, X, thr, delta=1e-3, chunk=64):
    """hyps [H,12] fp32 -> (lo [H], hi [H]): lo counts the candidates that are inliers of the widened pose beyond doubt, hi
    adds the undecided ones (a distance within a relative delta of thr)."""
    hyps = np.asarray(hyps, np.float32).astype(np.float64).reshape(-1, 3, 4)
    H = hyps.shape[0]
    lo = np.zeros(H, np.int64)
    hi = np.zeros(H, np.int64)
    for k0 in range(0, H, chunk):
        M = hyps[k0:k0 + chunk]
        d = np.einsum('hrc,nc->hnr', M[:, :, :3], Pc) + M[:, None, :, 3] - X[None]
        dist = np.sqrt((d * d).sum(-1))
        undecided = np.abs(dist - thr) <= delta * thr
        inl = (dist < thr) & ~undecided
        lo[k0:k0 + chunk] = inl.sum(1)
        hi[k0:k0 + chunk] = inl.sum(1) + undecided.sum(1)
    return lo, hi


def algorithm_spread(Pc, X, sample):
    """d_alg of one hypothesis: the largest change of an entry of [R | t] between the SVD form and the eigh form."""
    a, b = hypothesis(Pc, X, sample, kabsch_svd), hypothesis(Pc, X, sample, kabsch_horn)
    if a is None or b is None:
        return np.inf if (a is None) != (b is None) else 0.0
    return float(np.abs(pose12(*a) - pose12(*b)).max())


def permutation_spread(R, t, Pc, X, sig2, weighted, thr, iters, point_sigma=0.01, perms=5, seed=0):
    """d_perm: the largest change of (an entry of the camera-to-world pose, a normalised entry of Sigma or the relative cost)
    of refine + covariance when the candidates are listed in another order."""
    def run(Pp, Xp, sp):
        Rr, tr = refine(R, t, Pp, Xp, refine_weights(sp, weighted, point_sigma), thr, iters)
        Sg, cost, _, _ = covariance(Rr, tr, Pp, Xp, sp, thr, point_sigma)
        return cam_to_world(Rr, tr), Sg, cost
    T0, S0, c0 = run(Pc, X, sig2)
    n0 = np.sqrt(np.outer(np.diag(S0), np.diag(S0)))
    rng = np.random.default_rng(seed)
    dp = dc = 0.0
    for _ in range(perms):
        p = rng.permutation(X.shape[0])
        T1, S1, c1 = run(Pc[p], X[p], sig2[p])
        dp = max(dp, float(np.abs(T1 - T0).max()))
        dc = max(dc, float((np.abs(S1 - S0) / n0).max()), abs(c1 - c0) / max(c0, 1e-300))
    return dp, dc


def rounding_spread(R, t, Pc, X, sig2, thr, point_sigma=0.01):
    """d_round, as pnp_unc_ref's: the largest change of a normalised entry of Sigma and of the relative cost when the pose
    (the camera-to-world 4x4 the device writes) is rounded to fp32 and back."""
    S0, c0, _, n0 = covariance(R, t, Pc, X, sig2, thr, point_sigma)
    T = cam_to_world(R, t).astype(np.float32).astype(np.float64)
    S1, c1, _, n1 = covariance(T[:3, :3], T[:3, 3], Pc, X, sig2, thr, point_sigma)
    if n0 != n1:
        return np.inf
    nrm = np.sqrt(np.outer(np.diag(S0), np.diag(S0)))
    return max(float((np.abs(S1 - S0) / nrm).max()), abs(c1 - c0) / max(c0, 1e-300))


def synthetic_frames_depth(seed, B, h, w, outliers=0.0, sigma_lo=0.005, sigma_hi=0.04, depth_noise=0.005, point_noise=0.0,
                           fx=525.0, fy=525.0, u=320.0, v=240.0, cell_stride=8):
    """(records [B,h,w,4], cam_points [B,h,w,4], camera-to-world ground truth [B,4,4]).  The records are
    pnp_unc_ref.synthetic_frames_sigma's for the same arguments, draw for draw (tested), so PnP and Kabsch can be compared
    on the same frames.  The camera points come from a generator of their own (seed + 1): the true camera point of every
    cell, moved along its viewing ray by N(0, depth_noise) in depth and by an isotropic N(0, point_noise); mask 1."""
    rng = np.random.default_rng(seed)
    rng_d = np.random.default_rng(seed + 1)
    recs, cams, gts = [], [], []
    for _ in range(B):
        R, t = P.random_pose(rng)
        rec = P.synthetic_records(rng, h, w, R, t, fx, fy, u, v, cell_stride)
        true_cam = rec[..., :3].astype(np.float64) @ R.T + t
        sigma = np.exp(rng.uniform(math.log(sigma_lo), math.log(sigma_hi), size=(h, w)))
        rec[..., :3] += (rng.normal(size=(h, w, 3)) * sigma[..., None]).astype(np.float32)
        rec[..., 3] = (1.0 / sigma).astype(np.float32)
        out = rng.random((h, w)) < outliers
        rec[..., :3][out] = rng.uniform(-5, 5, size=(int(out.sum()), 3)).astype(np.float32)
        z = true_cam[..., 2:3]
        cam = np.ones((h, w, 4), np.float32)
        pts = true_cam
        if depth_noise:
            pts = pts / z * (z + rng_d.normal(scale=depth_noise, size=z.shape))
        if point_noise:
            pts = pts + rng_d.normal(scale=point_noise, size=pts.shape)
        cam[..., :3] = pts
        recs.append(rec)
        cams.append(cam)
        gts.append(P.cam_to_world(R, t))
    return np.stack(recs), np.stack(cams), np.stack(gts)


# ---- the RGB-D frame sets that tests/test_gpu_kabsch.py solves and tests/test_kabsch_host.py measures on the CPU --------

def synthetic_frames_rgbd(seed, B, h, w, outliers=0.0, sigma_lo=0.005, sigma_hi=0.04, depth_noise=0.005, camera=None,
                          noise=True):
    """(records [B,h,w,4] float32, depth maps [B,8h,8w] uint16 in millimetres, camera-to-world ground truth [B,4,4]).
    Records as synthetic_frames_depth's (noise=False: exact scene points, confidence 100); the depth map holds, at the
    depth pixel that colour pixel (8c, 8r) reads under `camera` (a labels.DepthCamera; registration included), the cell's
    true depth plus N(0, depth_noise) rounded to the millimetre, and 0 (outside the validity window) everywhere else."""
    import labels_ref as L
    from kfnet_amd.labels import DepthCamera
    cam = DepthCamera() if camera is None else camera
    rng = np.random.default_rng(seed)
    rng_d = np.random.default_rng(seed + 1)
    H, W = 8 * h, 8 * w
    _, _, xd, yd, ok_x, ok_y = L.depth_pixels(cam, H, W, 8, np.float32)
    assert ok_x.all() and ok_y.all()
    xd, yd = xd.astype(np.int64), yd.astype(np.int64)
    recs, gts = [], []
    depth = np.zeros((B, H, W), np.uint16)
    for b in range(B):
        R, t = P.random_pose(rng)
        rec = P.synthetic_records(rng, h, w, R, t, cam.fx, cam.fy, cam.u, cam.v, 8)
        z = (rec[..., :3].astype(np.float64) @ R.T + t)[..., 2]
        if noise:
            sigma = np.exp(rng.uniform(math.log(sigma_lo), math.log(sigma_hi), size=(h, w)))
            rec[..., :3] += (rng.normal(size=(h, w, 3)) * sigma[..., None]).astype(np.float32)
            rec[..., 3] = (1.0 / sigma).astype(np.float32)
        out = rng.random((h, w)) < outliers
        rec[..., :3][out] = rng.uniform(-5, 5, size=(int(out.sum()), 3)).astype(np.float32)
        if depth_noise:
            z = z + rng_d.normal(scale=depth_noise, size=z.shape)
        depth[b][yd[:, None], xd[None, :]] = np.clip(np.rint(z * 1000.0), 1, 65534).astype(np.uint16)
        recs.append(rec)
        gts.append(P.cam_to_world(R, t))
    return np.stack(recs), depth, np.stack(gts)


def cam_points32(depth, camera=None):
    """kfn_depth_labels at stride 8 under the identity pose, restated in float32 (labels_ref.labels32)."""
    import labels_ref as L
    from kfnet_amd.labels import DepthCamera
    cam = DepthCamera() if camera is None else camera
    return L.labels32(depth, np.tile(np.eye(4), (depth.shape[0], 1, 1)), cam, 8)


def _registered():
    from kfnet_amd.labels import DepthCamera
    return DepthCamera(depth_fx=500., depth_fy=500., depth_u=318., depth_v=240.)    # every cell's depth pixel inside 120x160


def _wide(a, ld):
    """[...,4] -> [...,ld] with NaN in the extra channels, which must not be read."""
    out = np.full(a.shape[:-1] + (ld,), np.nan, np.float32)
    out[..., :4] = a
    return out


def stage_set(name):
    """The named frame set of the stage tests: dict(records, depth, camera, ld, ldp, kw = solver options)."""
    kw = dict(hypotheses=256, min_points=16, seed=0, min_confidence=20., inlier_m=0.10, point_sigma=0.01)
    cam, ld, ldp = None, 4, 4
    if name == '9x13':
        recs, depth, _ = synthetic_frames_rgbd(801, 8, 9, 13, 0.5)
    elif name == '15x20':
        recs, depth, _ = synthetic_frames_rgbd(802, 4, 15, 20, 0.3)
        ld, ldp = 7, 5
    elif name == '37x53':
        recs, depth, _ = synthetic_frames_rgbd(803, 3, 37, 53, 0.4)
    elif name == '15x20_registered':
        cam = _registered()
        recs, depth, _ = synthetic_frames_rgbd(804, 4, 15, 20, 0.3, camera=cam)
    else:
        raise KeyError(name)
    return dict(records=recs, depth=depth, camera=cam, ld=ld, ldp=ldp, kw=kw)


STAGE_SETS = ('9x13', '15x20', '37x53', '15x20_registered')
SMALL_AREA = 1e-4          # hypotheses whose camera or scene triangle has |cross| below this (m^2) are compared by flag only
