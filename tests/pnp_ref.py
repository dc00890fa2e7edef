"""numpy fp64 restatement of kfn_pnp_ransac (kfnet_amd/csrc/kfn_pnp.hip, DESIGN.md "Camera poses").

Test infrastructure only: the product path never imports it.  Same candidate rule, same counter-based sampling (so the
samples match the device bit for bit), the same Grunert P3P with a Ferrari quartic, the same selection and the same
Gauss-Newton refinement; the device scores its hypotheses in fp32, this module in fp64.

Pose convention: (R, t) maps world to camera, Xc = R X + t; the returned 4x4 is camera-to-world [R^T | -R^T t].
"""
import math

import numpy as np

M32 = 0xFFFFFFFF
OK, TOO_FEW, NO_HYPOTHESIS = 0, 1, 2
MAX_DRAWS = 16


def lowbias32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def sample_hash(seed, frame, hyp, draw):
    return lowbias32((seed & M32) ^ ((frame * 0x9E3779B1) & M32) ^ ((hyp * 0x85EBCA77) & M32)
                     ^ ((draw * 0xC2B2AE3D) & M32))


def draw_sample(seed, frame, hyp, n):
    """Four distinct candidate indices in draw order, or None after MAX_DRAWS draws."""
    picked = []
    for draw in range(MAX_DRAWS):
        k = (sample_hash(seed, frame, hyp, draw) * n) >> 32
        if k not in picked:
            picked.append(k)
            if len(picked) == 4:
                return picked
    return None


def candidates(rec, min_confidence=20.0, cell_stride=8):
    """rec [h,w,>=4] -> (points [n,3] fp64, pixels [n,2] = (8c, 8r)) in raster order."""
    rec = np.asarray(rec, dtype=np.float32)
    h, w = rec.shape[:2]
    xyz = rec[..., :3]
    keep = (rec[..., 3] > np.float32(min_confidence)) & np.isfinite(xyz).all(axis=-1)
    rr, cc = np.nonzero(keep)
    pix = np.stack([cc * cell_stride, rr * cell_stride], axis=1).astype(np.float64)
    return xyz[keep].astype(np.float64), pix


# ---- P3P: Grunert's quartic (Haralick et al., IJCV 1994), Ferrari's solution ---------------------------------------

def _cubic_largest_root(a, b, c):
    """Largest real root of m^3 + a m^2 + b m + c (Cardano / trigonometric form, two Newton steps)."""
    P = b - a * a / 3.0
    Q = 2.0 * a * a * a / 27.0 - a * b / 3.0 + c
    D = Q * Q / 4.0 + P * P * P / 27.0
    if D >= 0.0:
        sd = math.sqrt(D)
        z = np.cbrt(-Q / 2.0 + sd) + np.cbrt(-Q / 2.0 - sd)
    else:
        k = 3.0 * Q / (2.0 * P) * math.sqrt(-3.0 / P)
        k = min(1.0, max(-1.0, k))
        z = 2.0 * math.sqrt(-P / 3.0) * math.cos(math.acos(k) / 3.0)
    m = float(z) - a / 3.0
    for _ in range(2):
        f = ((m + a) * m + b) * m + c
        df = (3.0 * m + 2.0 * a) * m + b
        if df != 0.0:
            m -= f / df
    return m


def _quadratic(B, C, out):
    d = B * B - 4.0 * C
    if d < 0.0:
        if d < -1e-10 * max(1.0, B * B):
            return
        d = 0.0
    s = math.sqrt(d)
    out.append((-B + s) / 2.0)
    out.append((-B - s) / 2.0)


def solve_quartic(A4, A3, A2, A1, A0):
    """Real roots (up to 4, possibly repeated) of A4 x^4 + ... + A0, each polished by two Newton steps."""
    if abs(A4) < 1e-14 * max(abs(A3), abs(A2), abs(A1), abs(A0), 1e-300):
        return []
    b, c, d, e = A3 / A4, A2 / A4, A1 / A4, A0 / A4
    p = c - 3.0 * b * b / 8.0
    q = d - b * c / 2.0 + b * b * b / 8.0
    r = e - b * d / 4.0 + b * b * c / 16.0 - 3.0 * b * b * b * b / 256.0
    m = _cubic_largest_root(p, p * p / 4.0 - r, -q * q / 8.0)
    ys = []
    if m > 1e-12:
        s = math.sqrt(2.0 * m)
        _quadratic(-s, p / 2.0 + m + q / (2.0 * s), ys)
        _quadratic(s, p / 2.0 + m - q / (2.0 * s), ys)
    else:                       # q ~ 0: biquadratic y^4 + p y^2 + r
        zs = []
        _quadratic(p, r, zs)
        for z in zs:
            if z >= 0.0:
                ys.append(math.sqrt(z))
                ys.append(-math.sqrt(z))
    out = []
    for y in ys:
        x = y - b / 4.0
        for _ in range(2):
            f = (((x + b) * x + c) * x + d) * x + e
            df = ((4.0 * x + 3.0 * b) * x + 2.0 * c) * x + d
            if df != 0.0:
                x -= f / df
        out.append(x)
    return out


def bearing(pix, fx, fy, u, v):
    f = np.array([(pix[0] - u) / fx, (pix[1] - v) / fy, 1.0])
    return f / math.sqrt(f @ f)


def _frame(p1, p2, p3):
    e1 = p2 - p1
    e1 = e1 / math.sqrt(e1 @ e1)
    e3 = np.cross(p2 - p1, p3 - p1)
    e3 = e3 / math.sqrt(e3 @ e3)
    return np.stack([e1, np.cross(e3, e1), e3], axis=1)     # columns


def p3p(P, F):
    """P [3,3] world points, F [3,3] unit bearings -> list of (R, t) with R P_i + t = s_i F_i, s_i > 0."""
    P = np.asarray(P, np.float64)
    F = np.asarray(F, np.float64)
    a2 = float((P[1] - P[2]) @ (P[1] - P[2]))
    b2 = float((P[0] - P[2]) @ (P[0] - P[2]))
    c2 = float((P[0] - P[1]) @ (P[0] - P[1]))
    if b2 <= 0.0:
        return []
    ca, cb, cg = float(F[1] @ F[2]), float(F[0] @ F[2]), float(F[0] @ F[1])
    K1 = (a2 - c2) / b2
    K2 = (a2 + c2) / b2
    A4 = (K1 - 1.0) ** 2 - 4.0 * c2 / b2 * ca * ca
    A3 = 4.0 * (K1 * (1.0 - K1) * cb - (1.0 - K2) * ca * cg + 2.0 * c2 / b2 * ca * ca * cb)
    A2 = 2.0 * (K1 * K1 - 1.0 + 2.0 * K1 * K1 * cb * cb + 2.0 * (b2 - c2) / b2 * ca * ca
                - 4.0 * K2 * ca * cb * cg + 2.0 * (b2 - a2) / b2 * cg * cg)
    A1 = 4.0 * (-K1 * (1.0 + K1) * cb + 2.0 * a2 / b2 * cg * cg * cb - (1.0 - K2) * ca * cg)
    A0 = (1.0 + K1) ** 2 - 4.0 * a2 / b2 * cg * cg
    sols = []
    for v in solve_quartic(A4, A3, A2, A1, A0):
        den = 2.0 * (cg - v * ca)
        if v <= 0.0 or abs(den) < 1e-12:
            continue
        uu = ((K1 - 1.0) * v * v - 2.0 * K1 * cb * v + 1.0 + K1) / den
        q = 1.0 + v * v - 2.0 * v * cb
        if uu <= 0.0 or q <= 0.0:
            continue
        s1 = math.sqrt(b2 / q)
        C = np.stack([s1 * F[0], uu * s1 * F[1], v * s1 * F[2]])
        R = _frame(C[0], C[1], C[2]) @ _frame(P[0], P[1], P[2]).T
        t = C[0] - R @ P[0]
        sols.append((R, t))
    return sols


def project_error2(R, t, X, pix, fx, fy, u, v):
    """Squared pixel error and camera-frame Z of points X [n,3]."""
    Xc = X @ R.T + t
    Z = Xc[:, 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        ex = fx * Xc[:, 0] / Z - (pix[:, 0] - u)
        ey = fy * Xc[:, 1] / Z - (pix[:, 1] - v)
    return ex * ex + ey * ey, Z


def hypothesis(X, pix, sample, fx, fy, u, v):
    """(R, t) from the P3P solutions of sample[0:3] that puts sample[3] in front of the camera with the smallest
    pixel error (first such on ties), or None."""
    F = np.stack([bearing(pix[k], fx, fy, u, v) for k in sample[:3]])
    best, best_e = None, np.inf
    for R, t in p3p(X[sample[:3]], F):
        e2, Z = project_error2(R, t, X[sample[3:4]], pix[sample[3:4]], fx, fy, u, v)
        if Z[0] > 0.0 and e2[0] < best_e:
            best, best_e = (R, t), e2[0]
    return best


def rodrigues(w):
    th = math.sqrt(w @ w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1.0 - math.cos(th)) / (th * th) * (K @ K)


def _gn_system(R, t, X, pix, fx, fy, u, v):
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
    H = Ju.T @ Ju + Jv.T @ Jv
    g = Ju.T @ ru + Jv.T @ rv
    return H, g, float(ru @ ru + rv @ rv)


def refine(R, t, X, pix, fx, fy, u, v, thr, iters):
    """Gauss-Newton on the pixel error over the inliers of the current pose; a step is kept only if it lowers the
    cost over that inlier set."""
    for _ in range(iters):
        e2, Z = project_error2(R, t, X, pix, fx, fy, u, v)
        inl = (Z > 0.0) & (e2 < thr * thr)
        if inl.sum() < 3:
            break
        H, g, cost = _gn_system(R, t, X[inl], pix[inl], fx, fy, u, v)
        try:
            L = np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            break
        d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
        dR = rodrigues(d[:3])
        R2, t2 = dR @ R, dR @ t + d[3:]
        e2n, Zn = project_error2(R2, t2, X[inl], pix[inl], fx, fy, u, v)
        cost2 = float(e2n.sum()) if (Zn > 0.0).all() else np.inf
        if not cost2 < cost:
            break
        R, t = R2, t2
    return R, t


def inliers(R, t, X, pix, fx, fy, u, v, thr):
    e2, Z = project_error2(R, t, X, pix, fx, fy, u, v)
    return (Z > 0.0) & (e2 < thr * thr)


def cam_to_world(R, t):
    T = np.eye(4)
    T[:3, :3] = R.T
    T[:3, 3] = -R.T @ t
    return T


def hypotheses(rec, frame, H, seed=0, fx=525.0, fy=525.0, u=320.0, v=240.0, min_confidence=20.0, inlier_px=10.0,
               cell_stride=8, min_points=16):
    """What kfn_pnp_hypotheses returns for one frame: samples [H,4] (-1 = none), poses [H,12] = [R | t] (NaN = invalid),
    inlier counts [H] (-1 = invalid)."""
    X, pix = candidates(rec, min_confidence, cell_stride)
    n = X.shape[0]
    samples = -np.ones((H, 4), np.int64)
    poses = np.full((H, 12), np.nan)
    counts = -np.ones(H, np.int64)
    if n < max(min_points, 4):
        return samples, poses, counts, X, pix
    for k in range(H):
        s = draw_sample(seed, frame, k, n)
        if s is None:
            continue
        samples[k] = s
        hyp = hypothesis(X, pix, s, fx, fy, u, v)
        if hyp is None:
            continue
        R, t = hyp
        poses[k] = np.concatenate([R, t[:, None]], axis=1).ravel()
        counts[k] = int(inliers(R, t, X, pix, fx, fy, u, v, inlier_px).sum())
    return samples, poses, counts, X, pix


def ransac(records, t0=0, hypotheses_n=256, seed=0, fx=525.0, fy=525.0, u=320.0, v=240.0, min_confidence=20.0,
           inlier_px=10.0, cell_stride=8, min_points=16, refine_iters=10):
    """records [B,h,w,4] -> (poses [B,4,4] camera-to-world, NaN on failure; info [B,4] = (status, candidates,
    final inliers, best hypothesis))."""
    B = records.shape[0]
    poses = np.full((B, 4, 4), np.nan)
    info = np.zeros((B, 4), np.int64)
    for b in range(B):
        samples, hp, counts, X, pix = hypotheses(records[b], t0 + b, hypotheses_n, seed, fx, fy, u, v, min_confidence,
                                                 inlier_px, cell_stride, min_points)
        n = X.shape[0]
        info[b] = (TOO_FEW, n, 0, -1)
        if n < max(min_points, 4):
            continue
        best = int(np.argmax(counts))            # first maximum: ties go to the lowest index
        if counts[best] < 0:
            info[b] = (NO_HYPOTHESIS, n, 0, -1)
            continue
        M = hp[best].reshape(3, 4)
        R, t = refine(M[:, :3], M[:, 3], X, pix, fx, fy, u, v, inlier_px, refine_iters)
        poses[b] = cam_to_world(R, t)
        info[b] = (OK, n, int(inliers(R, t, X, pix, fx, fy, u, v, inlier_px).sum()), best)
    return poses, info


def random_pose(rng):
    """A random world-to-camera (R, t): uniform rotation, camera centre within 2 m of the origin."""
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    c = rng.uniform(-2.0, 2.0, size=3)
    return R, -R @ c


def synthetic_records(rng, h, w, R, t, fx=525.0, fy=525.0, u=320.0, v=240.0, cell_stride=8, confidence=100.0):
    """[h,w,4] float32 records whose scene coordinates project exactly onto pixel (8c, 8r) from pose (R, t), at depths
    uniform in 0.5..5 m, with confidence channel `confidence`."""
    rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    z = rng.uniform(0.5, 5.0, size=(h, w))
    Xc = np.stack([(cc * cell_stride - u) / fx * z, (rr * cell_stride - v) / fy * z, z], axis=-1)
    Xw = (Xc - t) @ R                       # R^T (Xc - t)
    rec = np.empty((h, w, 4), np.float32)
    rec[..., :3] = Xw
    rec[..., 3] = confidence
    return rec


# ---- helpers of tests/test_gpu_pnp_stages.py: one stage of the device at a time against fp64 ----------------------------

def synthetic_frames(seed, B, h, w, outliers=0.0, noise=0.0, fx=525.0, fy=525.0, u=320.0, v=240.0, cell_stride=8):
    """(records [B,h,w,4] float32, camera-to-world ground truth [B,4,4]): random poses, Gaussian `noise` (m) on every
    scene coordinate, a share `outliers` of the cells replaced by points uniform in +-5 m."""
    rng = np.random.default_rng(seed)
    recs, gts = [], []
    for _ in range(B):
        R, t = random_pose(rng)
        rec = synthetic_records(rng, h, w, R, t, fx, fy, u, v, cell_stride)
        if noise:
            rec[..., :3] += rng.normal(scale=noise, size=rec[..., :3].shape).astype(np.float32)
        out = rng.random((h, w)) < outliers
        rec[..., :3][out] = rng.uniform(-5, 5, size=(int(out.sum()), 3)).astype(np.float32)
        recs.append(rec)
        gts.append(cam_to_world(R, t))
    return np.stack(recs), np.stack(gts)


def first_max(counts):
    """The selection rule: index of the first maximum of the counts, -1 if no hypothesis is valid."""
    k = int(np.argmax(counts))
    return k if counts[k] >= 0 else -1


def widen(hyp):
    """A device hypothesis [12] = [R | t] in fp32 -> (R, t) in fp64, as pnp_refine_kernel reads it."""
    M = np.asarray(hyp, np.float32).astype(np.float64).reshape(3, 4)
    return M[:, :3].copy(), M[:, 3].copy()


def threshold_margin(R, t, X, pix, fx, fy, u, v, thr):
    """Smallest relative distance |err / thr - 1| of a candidate in front of the camera from the inlier threshold."""
    e2, Z = project_error2(R, t, X, pix, fx, fy, u, v)
    front = Z > 0.0
    if not front.any():
        return np.inf
    return float(np.abs(np.sqrt(e2[front]) / thr - 1.0).min())


def score_brackets(hyps, X, pix, fx, fy, u, v, thr, delta=1e-3, zmin=1e-3, chunk=64):
    """hyps [H,12] fp32 -> (lo [H], hi [H]): lo counts the candidates that are inliers of the widened pose beyond doubt,
    hi adds the undecided ones (|Zc| < zmin, or a pixel error within a relative delta of thr)."""
    hyps = np.asarray(hyps, np.float32).astype(np.float64).reshape(-1, 3, 4)
    H = hyps.shape[0]
    lo = np.zeros(H, np.int64)
    hi = np.zeros(H, np.int64)
    dx, dy = pix[:, 0] - u, pix[:, 1] - v
    for k0 in range(0, H, chunk):
        M = hyps[k0:k0 + chunk]
        Xc = np.einsum('hrc,nc->hnr', M[:, :, :3], X) + M[:, None, :, 3]
        Z = Xc[..., 2]
        with np.errstate(divide='ignore', invalid='ignore'):
            err = np.sqrt((fx * Xc[..., 0] / Z - dx) ** 2 + (fy * Xc[..., 1] / Z - dy) ** 2)
        undecided = (np.abs(Z) < zmin) | (np.abs(err - thr) <= delta * thr)
        inl = (Z > 0.0) & (err < thr) & ~undecided
        lo[k0:k0 + chunk] = inl.sum(1)
        hi[k0:k0 + chunk] = inl.sum(1) + undecided.sum(1)
    return lo, hi


def refine_permutation_spread(R, t, X, pix, fx, fy, u, v, thr, iters, perms=5, seed=0):
    """d_perm: the largest change of an entry of cam_to_world(refine(...)) when the candidates are listed in another
    order (other summation order; at convergence possibly another last accept/reject decision)."""
    base = cam_to_world(*refine(R, t, X, pix, fx, fy, u, v, thr, iters))
    rng = np.random.default_rng(seed)
    d = 0.0
    for _ in range(perms):
        p = rng.permutation(X.shape[0])
        T = cam_to_world(*refine(R, t, X[p], pix[p], fx, fy, u, v, thr, iters))
        d = max(d, float(np.abs(T - base).max()))
    return d
