"""kfn_pnp_ransac one stage at a time against the fp64 restatement tests/pnp_ref.py (DESIGN.md "Camera poses").

tests/test_gpu_pnp.py pins the draws and the P3P poses; everything after them it checks against ground truth only, with
tolerances the unrefined hypothesis already meets.  Here every later stage is compared with pnp_ref, and each stage's
reference starts from the device's own output of the stage before: the probe's fp32 [R|t] widened to double, exactly
as pnp_refine_kernel reads it, and the probe's integer counts (kfn_pnp_ransac and kfn_pnp_hypotheses share
launch_hyp_and_score, so these are the counts ransac selects from).  A legitimate fp32/fp64 difference in one stage
then cannot cause a mismatch in the next.

  selection   info[:,3] is the first index of the maximum of the probe's counts, info[:,1] the candidate count: exact.
  refinement  pose against pnp_ref.refine from the selected fp32 hypothesis: per entry 2**-23 * max(1, |ref|) (the fp32
              rounding of the output) + 10 * D_PERM (the reference's own sensitivity to the order of its sums);
              info[:,2] equals the reference's final inlier count.
  scoring     for every valid hypothesis, #decided inliers <= count <= #decided inliers + #undecided, a candidate
              being undecided if |Zc| < 1e-3 m or its pixel error is within a relative DELTA of inlier_px.

Out of scope: frames whose selected hypothesis has fewer than 16 inliers.  With near-singular normal equations the
device's Cholesky and LAPACK may disagree on positive definiteness; every refinement check asserts >= 16 first.

All inputs are deterministic from fixed seeds.  The conditions that keep a check from being vacuous (ties present, an
empty band at the threshold, mean bracket width below 1, reference movement above 1e-3, both kinds of sample row at
n = 4) are asserted, so a later change of seeds cannot quietly empty a test."""
import numpy as np
import pytest

import pnp_ref as P
from kfnet_amd import _lib
from kfnet_amd.KFNet import pnp

pytestmark = pytest.mark.gpu

# Largest change of the reference's camera-to-world pose over five permutations of its candidate list, measured on the
# CPU from pnp_ref.hypotheses' selected pose (rounded to fp32) on every frame set and variant below, refine_iters 1, 3,
# 10 and 100: 0 to 3.6e-15 at refine_iters 1 and 3; up to 7.92e-9 (9x13, frame 1) at 10 and 100, where the loop has
# converged and the last accept/reject decision depends on the last bits of the two costs.
D_PERM = 7.92e-9
# Scoring: ex = fx*Xc - (x-u)*Zc carries a few fp32 ulps of fx*|Xc|, about 3e-4 px*m for fx = 525 in 5 m scenes, and is
# compared against thr*Zc >= 5 px*m (Zc >= 0.5 m): about 1e-4 relative.  DELTA keeps a tenfold margin over that.
DELTA = 1e-3
BAND = 1e-6          # no candidate's final error within this relative distance of inlier_px (asserted)

DEFAULTS = dict(fx=525., fy=525., u=320., v=240., hypotheses=256, min_points=16, seed=0, min_confidence=20.,
                inlier_px=10., cell_stride=8)
CONFIG5 = dict(fx=1050. * 540 / 1080, fy=1050. * 540 / 1080, u=480., v=270.)


def _kw(**kw):
    full = dict(DEFAULTS)
    full.update(kw)
    return full


def _cam(kw):
    return kw['fx'], kw['fy'], kw['u'], kw['v']


def _frames(seed, B, h, w, outliers, noise, kw):
    return P.synthetic_frames(seed, B, h, w, outliers, noise, kw['fx'], kw['fy'], kw['u'], kw['v'], kw['cell_stride'])[0]


class Probe(object):
    """The device's hypotheses and counts of one batch, with the reference's candidate lists."""

    def __init__(self, recs, kw, t0=0):
        self.recs, self.kw, self.t0 = recs, kw, t0
        self.h, self.w = recs.shape[1:3]
        self.samples, self.hp, self.counts = pnp.PnPSolver(self.h, self.w, **kw).hypotheses_probe(recs, t0=t0)
        self.cands = [P.candidates(r, kw['min_confidence'], kw['cell_stride']) for r in recs]

    def solve(self, refine_iters):
        return pnp.PnPSolver(self.h, self.w, refine_iters=refine_iters, **self.kw).solve(self.recs, t0=self.t0)


_PROBES = {}


def _probe(key, make):
    if key not in _PROBES:
        _PROBES[key] = Probe(*make())
    return _PROBES[key]


# ---- the three rules ----------------------------------------------------------------------------------------------------

def check_selection(pr, info):
    """Rule 1.  Returns the selected index of every frame."""
    best = []
    for b in range(pr.recs.shape[0]):
        n = pr.cands[b][0].shape[0]
        k = P.first_max(pr.counts[b]) if n >= pr.kw['min_points'] else -1
        status = _lib.PNP_TOO_FEW_POINTS if n < pr.kw['min_points'] else (_lib.PNP_OK if k >= 0 else _lib.PNP_NO_HYPOTHESIS)
        assert (info[b, 0], info[b, 1], info[b, 3]) == (status, n, k), (b, info[b], status, n, k)
        best.append(k)
    return best


def check_refinement(pr, poses, info, refine_iters):
    """Rule 2.  Returns how far the reference moved every frame's pose from its starting hypothesis."""
    kw = pr.kw
    cam, thr = _cam(kw), kw['inlier_px']
    moved = []
    for b in range(pr.recs.shape[0]):
        X, pix = pr.cands[b]
        k = P.first_max(pr.counts[b])
        assert info[b, 3] == k and pr.counts[b, k] >= 16, (b, info[b], k, pr.counts[b, k])
        R0, t0 = P.widen(pr.hp[b, k])
        R, t = P.refine(R0, t0, X, pix, *cam, thr, refine_iters)
        ref = P.cam_to_world(R, t)
        got = poses[b].astype(np.float64)
        margin = P.threshold_margin(R, t, X, pix, *cam, thr)
        inl = int(P.inliers(R, t, X, pix, *cam, thr).sum())
        moved.append(float(np.abs(ref - P.cam_to_world(R0, t0)).max()))
        print('frame %d: iters %d, max |device - ref| %.3g, ref moved %.3g, threshold margin %.3g, inliers %d / %d'
              % (b, refine_iters, np.abs(got - ref).max(), moved[-1], margin, info[b, 2], inl))
        assert margin > BAND, (b, margin)
        if refine_iters == 0:
            # no arithmetic on the rotation: the transpose of the probe's fp32 R, bit for bit
            assert np.array_equal(poses[b, :3, :3].view(np.uint32), pr.hp[b, k].reshape(3, 4)[:, :3].T.view(np.uint32)), b
            bound = 2.0 ** -23 * (np.abs(R0) * np.abs(t0)[:, None]).sum(0)     # |r0 t0| + |r1 t1| + |r2 t2| per column
            assert (np.abs(got[:3, 3] - ref[:3, 3]) <= bound).all(), (b, got[:3, 3], ref[:3, 3], bound)
            assert np.array_equal(got[3], [0., 0., 0., 1.])
        else:
            tol = 2.0 ** -23 * np.maximum(1.0, np.abs(ref)) + 10 * D_PERM
            assert (np.abs(got - ref) <= tol).all(), (b, refine_iters, np.abs(got - ref).max(), got, ref)
        assert info[b, 2] == inl, (b, info[b], inl)
    return moved


def check_scoring(pr):
    """Rule 3.  Returns the bracket widths of all valid hypotheses."""
    kw = pr.kw
    widths = []
    for b in range(pr.recs.shape[0]):
        X, pix = pr.cands[b]
        valid = pr.counts[b] >= 0
        assert (np.isfinite(pr.hp[b]).all(1) == valid).all(), b
        if not valid.any():
            continue
        lo, hi = P.score_brackets(pr.hp[b][valid], X, pix, *_cam(kw), kw['inlier_px'], DELTA, 1e-3)
        c = pr.counts[b][valid]
        bad = (c < lo) | (c > hi)
        assert not bad.any(), (b, np.nonzero(valid)[0][bad], c[bad], lo[bad], hi[bad])
        widths.append(hi - lo)
    return np.concatenate(widths) if widths else np.zeros(0)


def check_stages(pr, refine_iters=10, narrow=True):
    """Rules 1-3 on one batch; the scoring bracket must stay narrow (mean below 1 point) to mean anything."""
    poses, info = pr.solve(refine_iters)
    check_selection(pr, info)
    moved = check_refinement(pr, poses, info, refine_iters)
    widths = check_scoring(pr)
    print('bracket width: mean %.3f, max %d over %d hypotheses' % (widths.mean(), widths.max(), widths.size))
    assert widths.size and (widths.mean() < 1.0 or not narrow), widths.mean()
    return moved


# ---- 1. selection -------------------------------------------------------------------------------------------------------

def _tie_grids():
    kw = _kw(min_points=16)
    noisy = _frames(101, 8, 4, 5, 0.3, 0.02, kw)                       # n = 20
    clean = _frames(102, 8, 5, 7, 0.0, 0.0, kw)                        # every valid hypothesis ties at n
    for b in range(8):
        clean[b].reshape(-1, 4)[:3 + 2 * b, 3] = 1.0                   # n = 32, 30, .. 18: list index != cell index
    mixed = _frames(103, 8, 6, 7, 0.3, 0.02, kw)                       # n = 42
    return [('4x5', noisy), ('5x7', clean), ('6x7', mixed)]


def test_selection_is_the_first_maximum_of_the_device_counts():
    """Ties are the normal case on small grids; the tie-break goes through a per-lane strided scan, a wave butterfly and
    a four-wave merge.  Hypothesis counts on both sides of every one of those boundaries."""
    real_tie = winner_past_256 = cross_wave = 0
    for H in (1, 63, 64, 65, 255, 256, 257, 1024):
        for name, recs in _tie_grids():
            pr = Probe(recs, _kw(hypotheses=H, min_points=16), t0=3)
            _, info = pr.solve(10)
            best = check_selection(pr, info)
            for b, k in enumerate(best):
                if name == '5x7' and k >= 0:
                    n = pr.cands[b][0].shape[0]
                    valid = pr.counts[b] >= 0
                    assert (pr.counts[b][valid] == n).all(), (b, pr.counts[b])
                if k < 0:
                    continue
                tied = np.nonzero(pr.counts[b] == pr.counts[b, k])[0]
                real_tie += tied.size >= 2
                winner_past_256 += k >= 256
                cross_wave += bool(((tied % 256) // 64 != (k % 256) // 64).any())
    print('ties %d, winners >= 256: %d, ties across waves %d' % (real_tie, winner_past_256, cross_wave))
    assert real_tie >= 1 and winner_past_256 >= 1 and cross_wave >= 1, (real_tie, winner_past_256, cross_wave)


# ---- 2. refinement ------------------------------------------------------------------------------------------------------

FRAME_SETS = {
    '15x20': lambda: (_frames(201, 4, 15, 20, 0.3, 0.02, _kw()), _kw()),
    '30x40': lambda: (_frames(202, 4, 30, 40, 0.4, 0.015, _kw()), _kw()),
    '60x80': lambda: (_frames(203, 4, 60, 80, 0.5, 0.01, _kw()), _kw()),
    '68x120': lambda: (_frames(204, 4, 68, 120, 0.3, 0.01, _kw(**CONFIG5)), _kw(**CONFIG5)),
}


@pytest.mark.parametrize('refine_iters', [0, 1, 3, 10, 100])
@pytest.mark.parametrize('frames', sorted(FRAME_SETS))
def test_refinement_matches_fp64_gauss_newton(frames, refine_iters):
    """A Gauss-Newton loop that never accepts a step, has a wrong Jacobian column or a wrong Cholesky solve still meets
    the ground-truth tolerances of test_gpu_pnp.py: they are the size of the movement itself.  At refine_iters = 100 the
    accept rule ends the loop (the step-rejected branch); at 0 the pose is the hypothesis, transposed."""
    pr = _probe(frames, FRAME_SETS[frames])
    poses, info = pr.solve(refine_iters)
    assert (info[:, 0] == _lib.PNP_OK).all(), info
    moved = check_refinement(pr, poses, info, refine_iters)
    if refine_iters >= 3:
        assert min(moved) > 1e-3, moved           # else agreeing with the reference proves nothing


# ---- 3. scoring ---------------------------------------------------------------------------------------------------------

def test_scoring_is_bracketed_for_every_hypothesis():
    """The 0.5 % n of test_gpu_pnp.py is 24 points at 60x80; the bracket here is 3 points at most and about 0.1 on
    average (asserted below 1)."""
    kw = _kw(hypotheses=1024)
    pr = Probe(_frames(301, 2, 60, 80, 0.5, 0.01, kw), kw, t0=11)
    widths = check_scoring(pr)
    print('bracket width: mean %.3f, max %d over %d hypotheses' % (widths.mean(), widths.max(), widths.size))
    assert widths.size > 0.5 * 2 * 1024 and widths.mean() < 1.0, (widths.size, widths.mean())


# ---- 4. short candidate lists -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 5, 16])
def test_short_candidate_lists(n):
    """With few candidates the 16-draw limit bites: at n = 4 some hypotheses never draw 4 distinct indices."""
    kw = _kw(min_points=4)
    recs = _frames(401, 4, 6, 7, 0.0, 0.0, kw)
    rng = np.random.default_rng(402)
    for b in range(4):
        conf = np.ones(42, np.float32)
        conf[rng.permutation(42)[:n]] = 100.0
        recs[b, ..., 3] = conf.reshape(6, 7)
    pr = Probe(recs, kw, t0=0)
    none = 0
    for b in range(4):
        rs, _, rc, X, _ = P.hypotheses(recs[b], b, 256, min_points=4)
        assert X.shape[0] == n
        assert np.array_equal(pr.samples[b], rs), b                 # the -1 rows included
        assert ((pr.counts[b] >= 0) == (rc >= 0)).mean() >= 0.99, b
        assert (pr.counts[b][(rs < 0).any(1)] == -1).all(), b
        none += int((rs < 0).any(1).sum())
    if n == 4:
        assert 0 < none < 4 * 256, none                             # both kinds of row
    _, info = pr.solve(10)
    check_selection(pr, info)


# ---- 5. KFN_PNP_NO_HYPOTHESIS ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', ['one_point', 'one_line'])
def test_no_hypothesis_status_without_touching_neighbours(shape):
    """42 confident cells that all carry the same scene point, or points of one line: no P3P sample has a solution."""
    kw = _kw()
    recs = _frames(501, 3, 30, 40, 0.3, 0.01, kw)
    recs[1, ..., 3] = 1.0
    recs[1, 7, :, 3][:40] = 100.0
    recs[1, 8, :2, 3] = 100.0
    cells = recs[1].reshape(-1, 4)
    conf = cells[:, 3] > 20.0
    assert conf.sum() == 42
    if shape == 'one_point':
        cells[conf, :3] = (0.25, -0.5, 2.0)
    else:
        cells[conf, :3] = np.stack([0.125 * np.arange(42), np.zeros(42), np.full(42, 2.0)], 1)
    with np.errstate(all='ignore'):
        _, ref_info = P.ransac(recs[1:2], t0=1)
    assert tuple(ref_info[0]) == (P.NO_HYPOTHESIS, 42, 0, -1)
    solver = pnp.PnPSolver(30, 40, **kw)
    poses, info = solver.solve(recs)
    assert tuple(info[1]) == (_lib.PNP_NO_HYPOTHESIS, 42, 0, -1), info[1]
    assert np.isnan(poses[1]).all()
    for b in (0, 2):
        pb, ib = solver.solve(recs[b:b + 1], t0=b)
        assert ib[0, 0] == _lib.PNP_OK
        assert np.array_equal(pb[0].view(np.uint32), poses[b].view(np.uint32)) and np.array_equal(ib[0], info[b]), b


# ---- 6. strides, pitch and the grid limits ------------------------------------------------------------------------------

def _ld7():
    kw = _kw()
    recs = _frames(601, 3, 30, 40, 0.4, 0.01, kw)
    wide = np.full(recs.shape[:3] + (7,), np.nan, np.float32)      # the extra channels must not be read
    wide[..., :4] = recs
    return wide, kw


def _strided(cs):
    kw = _kw(cell_stride=cs, u=20. * cs, v=15. * cs)
    return _frames(602 + cs, 3, 30, 40, 0.4, 0.01, kw), kw


def _skewed():
    kw = _kw(fx=500., fy=560., u=300.5, v=250.25)
    return _frames(603, 3, 30, 40, 0.4, 0.01, kw), kw


def _grid(h, w, seed):
    kw = _kw()
    return _frames(seed, 3, h, w, 0.3, 0.01, kw), kw


def _limit(outliers, noise):
    kw = _kw(hypotheses=64, u=1024., v=512.)                       # 32 768 cells: the uint16 list fills 64 KiB of LDS
    return _frames(606, 1, 128, 256, outliers, noise, kw), kw


VARIANTS = {
    'ld7': _ld7,
    'cell_stride4': lambda: _strided(4),
    'cell_stride16': lambda: _strided(16),
    'fx_ne_fy': _skewed,
    'grid9x13': lambda: _grid(9, 13, 604),             # h*w a multiple of neither TILE = 128 nor 256
    'grid37x53': lambda: _grid(37, 53, 605),
    'grid128x256': lambda: _limit(0.3, 0.01),
    'grid128x256_clean': lambda: _limit(0.0, 0.0),
}


@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_strides_pitch_and_grid_limits(variant):
    """The width of the scoring bracket grows with the number of candidates: about 2e-4 of uniformly spread points have
    |Zc| < 1e-3 m, and noisy near points sit at the threshold.  On 32 768 cells with 30 % outliers and 1 cm noise it is
    11.6 points on average (CPU measurement), so there the bracket alone would let a lost cell pass.  The largest grid
    therefore runs twice: with outliers and noise, where refinement has something to do, and with neither, where
    every candidate is a decided inlier of every valid hypothesis, the bracket closes and all 32 768 must be counted."""
    recs, kw = VARIANTS[variant]()
    moved = check_stages(Probe(recs, kw, t0=5), narrow=variant != 'grid128x256')
    if variant != 'grid128x256_clean':
        assert min(moved) > 1e-3, moved
