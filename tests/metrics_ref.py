"""Reference of kfn_eval_metrics (kfnet_amd/csrc/kfn_metrics.hip), test infrastructure only: the kernel's contract restated
in fp64 from the fp32 inputs -- what include/kfnet_hip.h promises for `stats` and `dist_maps`, which is KFNet.
CoordLossWithUncertainty(downsample=True) x 3 (KFNet/KFNet.py:192-232 as wired by KFNet/train.py:252-257), get_NIS_measurement and
dist_error (KFNet/eval.py:10-29) on grid-sized labels.  Pinned on the CPU against oracle/kfnet_metrics_oracle.py and its
hand-computed values (tests/test_metrics.py) before any GPU sees it.

Every THRESHOLD is the fp32 constant the reference's graph holds, widened to fp64 -- never the unrounded double:
    THR2     float32(0.05 * 0.05)   the Python-double product rounded once (KFNet.py:227), bits 0x3B23D70A
    MIN_UNC  float32(1e-5)          tf.maximum(uncertainty, self.min_uncertainty) (KFNet.py:212)
    NIS_LO / NIS_HI  float32(0.0157), float32(2.706)   numpy compares the fp32 NIS array with these as fp32 (eval.py:13-14)
The second half of the file builds the inputs of tests/test_gpu_metrics.py and states the conditions they must satisfy."""
import numpy as np

THR2 = float(np.float32(0.05 * 0.05))
MIN_UNC = float(np.float32(1e-5))
NIS_LO = float(np.float32(0.0157))
NIS_HI = float(np.float32(2.706))
LOSS_CAP = -2.0
ROLES = ('meas', 'temp', 'kf')


def _f64(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, 'the reference starts from the fp32 values the kernel reads'
    return a.astype(np.float64)


def transformed(x, M):
    """ApplyTransform (KFNet/util.py:12-40) of [...,3] fp64 coordinates with the 3x4 M, or x itself for None."""
    if M is None:
        return x
    M = _f64(np.asarray(M, np.float32).reshape(3, 4))
    return x @ M[:, :3].T + M[:, 3]


def loss_terms(c, sigma, g):
    """One prediction against one label map.  c [HW,3] transformed coordinates, sigma [HW], g [HW,4] = (gt xyz, mask), all fp64.
    Returns a dict of [HW] arrays: m = (mask == 1), d2, u = max(sigma, MIN_UNC), a = 3 log u, q = d2 / (2 u^2), l = a + q (before
    the cap), term = m * min(l, -2), bad = max(m * d2 - THR2, 0) != 0."""
    m = (g[:, 3] == 1.0).astype(np.float64)
    e = c - g[:, :3]
    d2 = (e * e).sum(-1)
    u = np.maximum(sigma, MIN_UNC)
    a = 3.0 * np.log(u)
    q = d2 / (2.0 * u * u)
    l = a + q
    return dict(m=m, e=e, d2=d2, u=u, a=a, q=q, l=l, term=m * np.minimum(l, LOSS_CAP),
                bad=(np.maximum(m * d2 - THR2, 0.0) != 0.0).astype(np.float64))


def eval_metrics(meas, temp, kf, rec, nis, labels, pair, reset, M=None, with_terms=False):
    """meas / temp / kf / rec [T,HW,4] fp32, nis [T,HW,3] fp32, labels [L,HW,4] fp32 (grid-sized), pair [T,2] label rows (a, b),
    reset [T], M 3x4 or None.  Returns (stats [T,9] fp64, dist [T,3,HW] fp64 in cm): the nine reduced entries of kfn_eval_metrics
    -- [0..2] loss sums over BOTH labels of the pair, [3..5] inaccurate counts, [6] sum(mask_a) + sum(mask_b) + 1, [7] NIS
    values > 0, [8] of those inside (NIS_LO, NIS_HI) -- and the distance maps against label b (the measurement in place of the
    prediction on a reset step; the emitted record untransformed).  with_terms: also the per-pixel quantities the error bounds
    of the GPU test are computed from, terms[t][role] = (loss_terms vs a, loss_terms vs b)."""
    preds = [_f64(meas), _f64(temp), _f64(kf)]
    rec, nis, labels = _f64(rec), _f64(nis), _f64(labels)
    pair = np.asarray(pair).reshape(-1, 2)
    T, HW = preds[0].shape[:2]
    stats = np.zeros((T, 9))
    dist = np.zeros((T, 3, HW))
    terms = []
    for t in range(T):
        ga, gb = labels[pair[t, 0]], labels[pair[t, 1]]
        coords = [transformed(p[t, :, :3], M) for p in preds]
        per_role = {}
        for r in range(3):
            both = [loss_terms(coords[r], preds[r][t, :, 3], g) for g in (ga, gb)]
            stats[t, r] = both[0]['term'].sum() + both[1]['term'].sum()
            stats[t, 3 + r] = both[0]['bad'].sum() + both[1]['bad'].sum()
            per_role[ROLES[r]] = both
        terms.append(per_role)
        stats[t, 6] = (ga[:, 3] == 1.0).sum() + (gb[:, 3] == 1.0).sum() + 1.0
        stats[t, 7] = (nis[t] > 0.0).sum()
        stats[t, 8] = ((nis[t] > NIS_LO) & (nis[t] < NIS_HI)).sum()       # both imply > 0
        second = [coords[0], coords[0] if reset[t] else coords[1], rec[t, :, :3]]
        for k in range(3):
            dist[t, k] = np.sqrt(((second[k] - gb[:, :3]) ** 2).sum(-1)) * gb[:, 3] * 100.0
    return (stats, dist, terms) if with_terms else (stats, dist)


def log_fields(stats, dist):
    """The fields of eval.py's log line from one frame's stats [9] and dist [3,HW], as kfnet_amd/KFNet/metrics.py forms them."""
    out = {}
    for k, r in enumerate(('m', 't', 'kf')):
        out['l_' + r] = stats[k] / stats[6]
        out['a_' + r] = (stats[6] - stats[3 + k]) / stats[6]
        pos = dist[k][dist[k] > 0]
        out['d_' + r] = float(np.median(pos)) if pos.size else float('nan')
    out['nis'] = stats[8] / stats[7] if stats[7] > 0 else 0.0
    return out


# ---- the inputs of tests/test_gpu_metrics.py ------------------------------------------------------------------------------------
T_FRAMES, L_ROWS = 5, 7
PAIRS = np.array([(1, 0), (1, 2), (6, 6), (3, 5), (0, 4)], np.int32)       # a > b, adjacent, a == b, non-adjacent rows
RESET = np.array([1, 0, 0, 1, 0], np.uint8)
HW_CASES = (1, 63, 64, 65, 255, 256, 257, 391, 4800, 8160)
NIS_ALL_POSITIVE, NIS_NONE_POSITIVE = 2, 4                                  # frames
MASK_VALUES = np.array([0.0, 1.0, 0.5, 2.0], np.float32)                   # the losses use == 1, the maps the raw value
MIN_CLASS = 10                                                             # pixels per class and frame at HW >= 255
THR_MARGIN = 1e-6


def nis_edge_values():
    lo, hi = np.float32(0.0157), np.float32(2.706)
    return np.array([0.0, lo, np.nextafter(lo, np.float32(1)), hi, np.nextafter(hi, np.float32(0))], np.float32)


def make_case(HW, with_transform, seed=0):
    """Seeded inputs that populate every branch of the kernel (dict of arrays; M is 3x4 fp32 or None)."""
    rng = np.random.default_rng([20, HW, int(with_transform), seed])
    T, L = T_FRAMES, L_ROWS
    labels = rng.normal(size=(L, HW, 4)).astype(np.float32)
    labels[..., 3] = rng.choice(MASK_VALUES, p=[0.15, 0.55, 0.15, 0.15], size=(L, HW))
    M = None
    if with_transform:
        M = np.concatenate([np.eye(3) + 0.2 * rng.normal(size=(3, 3)), rng.normal(size=(3, 1))], axis=1).astype(np.float32)
    M64 = None if M is None else M.astype(np.float64)

    def near(target):
        """target + an offset of length in [0, 0.04] u [0.06, 0.5] m, random direction (fp64)."""
        n = target.shape[:-1]
        length = np.where(rng.uniform(size=n) < 0.5, rng.uniform(0.0, 0.04, size=n), rng.uniform(0.06, 0.5, size=n))
        v = rng.normal(size=n + (3,))
        return target + v / np.linalg.norm(v, axis=-1, keepdims=True) * length[..., None]

    def sigma():
        """1e-7 ... 1: half of the pixels log-uniform over the whole range (the 1e-5 floor is active on 2/7 of those), half
        in 0.02 ... 0.6, where 3 log u + d2 / (2 u^2) falls on either side of -2."""
        wide = 10.0 ** rng.uniform(-7.0, 0.0, size=(T, HW))
        mid = 10.0 ** rng.uniform(np.log10(0.02), np.log10(0.6), size=(T, HW))
        return np.where(rng.uniform(size=(T, HW)) < 0.5, wide, mid)

    gt_b = labels[PAIRS[:, 1], :, :3].astype(np.float64)                       # [T,HW,3], the frame the step is about
    out = dict(labels=labels, pair=PAIRS.copy(), reset=RESET.copy(), M=M)
    for name in ROLES:
        want = near(gt_b)                                                     # in the labels' frame
        raw = want if M is None else (want - M64[:, 3]) @ np.linalg.inv(M64[:, :3]).T
        out[name] = np.concatenate([raw, sigma()[..., None]], axis=-1).astype(np.float32)
    out['rec'] = np.concatenate([near(gt_b), 1.0 / sigma()[..., None]], axis=-1).astype(np.float32)    # emitted: (T.x, 1/sigma)
    nis = np.exp(rng.normal(-1.0, 2.5, size=(T, HW, 3))).astype(np.float32)      # positives on both sides of the band
    special = np.concatenate([nis_edge_values(), -np.exp(rng.normal(size=3)).astype(np.float32)])
    pick = rng.uniform(size=nis.shape) < 0.45
    nis = np.where(pick, rng.choice(special, size=nis.shape), nis).astype(np.float32)
    nis[NIS_ALL_POSITIVE] = np.where(nis[NIS_ALL_POSITIVE] > 0, nis[NIS_ALL_POSITIVE], np.float32(0.5))
    nis[NIS_NONE_POSITIVE] = np.where(nis[NIS_NONE_POSITIVE] > 0, -nis[NIS_NONE_POSITIVE], nis[NIS_NONE_POSITIVE])
    out['nis'] = nis
    return out


def check_case(case, terms):
    """The conditions on the inputs, asserted on the host before any launch (and on a machine without a GPU by
    tests/test_metrics.py): all finite; no masked pixel within THR_MARGIN of the squared threshold in fp64, so that the
    reference alone decides every count; at HW >= 255 every class holds at least MIN_CLASS pixels per frame."""
    T, HW = case['meas'].shape[:2]
    for k in ROLES + ('rec', 'nis', 'labels'):
        assert np.isfinite(case[k]).all(), k
    for t in range(T):
        for role in ROLES:
            for lt in terms[t][role]:
                assert not np.any((lt['m'] == 1.0) & (np.abs(lt['d2'] - THR2) < THR_MARGIN)), (t, role)
    nis = case['nis']
    assert (nis[NIS_ALL_POSITIVE] > 0).all() and not (nis[NIS_NONE_POSITIVE] > 0).any()
    if HW < 255:
        return
    edges = nis_edge_values()
    for t in range(T):
        classes = {}
        for j, row in enumerate(case['pair'][t]):
            for v in MASK_VALUES:
                classes['label %d mask %g' % (j, v)] = case['labels'][row, :, 3] == v
        for role in ROLES:
            s = case[role][t, :, 3]
            classes[role + ' sigma below the floor'] = s < np.float32(1e-5)
            classes[role + ' sigma above the floor'] = s > np.float32(1e-5)
            masked = [lt['m'] == 1.0 for lt in terms[t][role]]
            l = [lt['l'] for lt in terms[t][role]]
            classes[role + ' masked, capped'] = np.concatenate([masked[0] & (l[0] > LOSS_CAP), masked[1] & (l[1] > LOSS_CAP)])
            classes[role + ' masked, below the cap'] = np.concatenate([masked[0] & (l[0] < LOSS_CAP), masked[1] & (l[1] < LOSS_CAP)])
            b = terms[t][role][1]
            classes[role + ' masked, within 5 cm'] = masked[1] & (b['d2'] < THR2)
            classes[role + ' masked, beyond 5 cm'] = masked[1] & (b['d2'] > THR2)
        if t == NIS_NONE_POSITIVE:
            classes['nis zero'] = nis[t] == 0
            classes['nis negative'] = nis[t] < 0
        else:
            for e in edges[1:]:
                classes['nis == %.9g' % e] = nis[t] == e
            classes['nis inside the band'] = (nis[t] > edges[2]) & (nis[t] < edges[4])
            classes['nis below the band'] = (nis[t] > 0) & (nis[t] < edges[1])
            classes['nis above the band'] = nis[t] > edges[3]
            if t != NIS_ALL_POSITIVE:
                classes['nis zero'] = nis[t] == 0
                classes['nis negative'] = nis[t] < 0
        for name, sel in classes.items():
            assert int(np.count_nonzero(sel)) >= MIN_CLASS, (HW, t, name, int(np.count_nonzero(sel)))
