"""numpy restatement of kfn_pnp_ransac_guided's sampling (DESIGN.md 5c "Guided sampling"), on top of pnp_ref.

Test infrastructure only: the product path never imports it.  Candidates, the hash, the 16-draw limit, P3P, scoring,
selection and refinement are pnp_ref's; this module replaces the index of a draw: the candidates carry integer weights
made from their confidence in float32, and a draw picks the first candidate whose cumulative weight exceeds
floor(hash * total / 2**32).  All integers here are exact (uint64 arrays whose sums stay below 2**48, Python ints for the
product), so the device must reproduce `cumulative` and every sample bit for bit.
"""
import numpy as np

import pnp_ref as P

UNIFORM, CONFIDENCE, CONFIDENCE_SQ = 0, 1, 2
MAX_CAP = 4096.0


def candidate_confidence(rec, min_confidence=20.0):
    """record[3] of the candidates as float32, in pnp_ref.candidates' (raster) order."""
    rec = np.asarray(rec, dtype=np.float32)
    keep = (rec[..., 3] > np.float32(min_confidence)) & np.isfinite(rec[..., :3]).all(axis=-1)
    return rec[..., 3][keep]


def weights(conf, mode, min_confidence=20.0, confidence_cap=1000.0):
    """conf [n] (candidates' confidences, each > min_confidence) -> w [n] uint64: q = int(floor((min(c, cap) - minc) * 16))
    + 1 with every operation in float32, w = q (mode 1) or q * q (mode 2)."""
    if mode not in (CONFIDENCE, CONFIDENCE_SQ):
        raise ValueError('mode must be 1 or 2')
    minc, cap = np.float32(min_confidence), np.float32(confidence_cap)
    if not (0.0 <= minc < cap <= MAX_CAP and np.isfinite(cap)):
        raise ValueError('need 0 <= min_confidence < confidence_cap <= 4096')
    c = np.asarray(conf, dtype=np.float32)
    d = (np.minimum(c, cap) - minc).astype(np.float32)
    q = np.floor((d * np.float32(16.0)).astype(np.float32)).astype(np.int64) + 1
    assert (q >= 1).all()
    q = q.astype(np.uint64)
    return q if mode == CONFIDENCE else q * q


def cumulative(w):
    """cum[i] = w[0] + .. + w[i] in uint64."""
    return np.cumsum(np.asarray(w, dtype=np.uint64), dtype=np.uint64)


def draw_target(hsh, total):
    """floor(hsh * total / 2**32), the exact integer."""
    return (int(hsh) * int(total)) >> 32


def draw_sample_guided(seed, frame, hyp, cum):
    """pnp_ref.draw_sample with the guided index: four distinct candidate indices in draw order, or None."""
    total = int(cum[-1])
    picked = []
    for draw in range(P.MAX_DRAWS):
        target = draw_target(P.sample_hash(seed, frame, hyp, draw), total)
        k = int(np.searchsorted(cum, np.uint64(target), side='right'))      # first i with cum[i] > target
        if k not in picked:
            picked.append(k)
            if len(picked) == 4:
                return picked
    return None


def hypotheses_guided(rec, frame, H, mode, confidence_cap=1000.0, seed=0, fx=525.0, fy=525.0, u=320.0, v=240.0,
                      min_confidence=20.0, inlier_px=10.0, cell_stride=8, min_points=16, score=True):
    """pnp_ref.hypotheses with guided draws: (samples [H,4], poses [H,12], counts [H], X, pix), and the frame's
    cumulative weights as a sixth value.  score=False leaves the counts of valid hypotheses at 0."""
    X, pix = P.candidates(rec, min_confidence, cell_stride)
    n = X.shape[0]
    cum = cumulative(weights(candidate_confidence(rec, min_confidence), mode, min_confidence, confidence_cap))
    samples = -np.ones((H, 4), np.int64)
    poses = np.full((H, 12), np.nan)
    counts = -np.ones(H, np.int64)
    if n < max(min_points, 4):
        return samples, poses, counts, X, pix, cum
    for k in range(H):
        s = draw_sample_guided(seed, frame, k, cum)
        if s is None:
            continue
        samples[k] = s
        hyp = P.hypothesis(X, pix, s, fx, fy, u, v)
        if hyp is None:
            continue
        R, t = hyp
        poses[k] = np.concatenate([R, t[:, None]], axis=1).ravel()
        counts[k] = int(P.inliers(R, t, X, pix, fx, fy, u, v, inlier_px).sum()) if score else 0
    return samples, poses, counts, X, pix, cum


def ransac_guided(records, mode, confidence_cap=1000.0, t0=0, hypotheses_n=256, seed=0, fx=525.0, fy=525.0, u=320.0,
                  v=240.0, min_confidence=20.0, inlier_px=10.0, cell_stride=8, min_points=16, refine_iters=10):
    """pnp_ref.ransac with guided draws: (poses [B,4,4], info [B,4])."""
    B = records.shape[0]
    poses = np.full((B, 4, 4), np.nan)
    info = np.zeros((B, 4), np.int64)
    for b in range(B):
        _, hp, counts, X, pix, _ = hypotheses_guided(records[b], t0 + b, hypotheses_n, mode, confidence_cap, seed, fx, fy,
                                                     u, v, min_confidence, inlier_px, cell_stride, min_points)
        n = X.shape[0]
        info[b] = (P.TOO_FEW, n, 0, -1)
        if n < max(min_points, 4):
            continue
        best = int(np.argmax(counts))
        if counts[best] < 0:
            info[b] = (P.NO_HYPOTHESIS, n, 0, -1)
            continue
        M = hp[best].reshape(3, 4)
        R, t = P.refine(M[:, :3], M[:, 3], X, pix, fx, fy, u, v, inlier_px, refine_iters)
        poses[b] = P.cam_to_world(R, t)
        info[b] = (P.OK, n, int(P.inliers(R, t, X, pix, fx, fy, u, v, inlier_px).sum()), best)
    return poses, info


def synthetic_frames_confidence(seed, B, h, w, outliers, fx=525.0, fy=525.0, u=320.0, v=240.0, cell_stride=8):
    """(records [B,h,w,4] float32, camera-to-world ground truth [B,4,4]).  Every cell has sigma log-uniform in 0.5-2 cm
    and Gaussian noise of that sigma on its scene coordinate; a share `outliers` of the cells is replaced by points uniform
    in +-5 m with sigma redrawn log-uniform in 1-4.5 cm.  Confidence = 1/sigma as float32: 50..200 on inliers, 22.2..100
    on outliers -- above the default threshold 20 everywhere, and overlapping: informative, not a label."""
    rng = np.random.default_rng(seed)
    recs, gts = [], []
    for _ in range(B):
        R, t = P.random_pose(rng)
        rec = P.synthetic_records(rng, h, w, R, t, fx, fy, u, v, cell_stride)
        sigma = np.exp(rng.uniform(np.log(0.005), np.log(0.02), size=(h, w)))
        rec[..., :3] += (rng.normal(size=(h, w, 3)) * sigma[..., None]).astype(np.float32)
        out = rng.random((h, w)) < outliers
        k = int(out.sum())
        rec[..., :3][out] = rng.uniform(-5, 5, size=(k, 3)).astype(np.float32)
        sigma[out] = np.exp(rng.uniform(np.log(0.01), np.log(0.045), size=k))
        rec[..., 3] = (1.0 / sigma).astype(np.float32)
        assert (rec[..., 3] > np.float32(20.0)).all()
        recs.append(rec)
        gts.append(P.cam_to_world(R, t))
    return np.stack(recs), np.stack(gts)


def within_5cm_5deg(poses, gts):
    """Frames whose camera-to-world pose is within 5 cm and 5 degrees of the truth (a NaN pose is outside)."""
    poses, gts = np.asarray(poses, np.float64), np.asarray(gts, np.float64)
    M = np.einsum('bji,bjk->bik', poses[:, :3, :3], gts[:, :3, :3])
    cos = np.clip((np.trace(M, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)
    with np.errstate(invalid='ignore'):
        rot = np.degrees(np.arccos(cos))
        trans = np.linalg.norm(poses[:, :3, 3] - gts[:, :3, 3], axis=1)
        return np.isfinite(rot) & np.isfinite(trans) & (rot < 5.0) & (trans < 0.05)
