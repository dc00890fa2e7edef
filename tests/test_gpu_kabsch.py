"""kfn_kabsch_ransac one stage at a time against the fp64 restatement tests/kabsch_ref.py (DESIGN.md 5c "Poses with depth").

As tests/test_gpu_pnp_stages.py does for PnP, each stage's reference starts from the device's own output of the stage
before: the camera points are the device's (kfn_depth_labels at stride 8 under the identity pose), the hypotheses are the
probe's fp32 [R|t] widened to double as kabsch_refine_kernel reads them, the counts are the probe's integers.

  samples      exact.
  validity     exact; no sampled triangle within a relative 1e-6 of the degeneracy threshold (asserted).
  hypotheses   per entry |device - ref| <= 2**-23 max(1, |ref|) + 10 d_alg, d_alg the reference's own change between its SVD
               form and its eigh form on the same sample; triangles below kabsch_ref.SMALL_AREA are compared by flag only and
               are at most 5 % of the valid ones (asserted here and, for the reference's hypotheses, on the CPU).
  scoring      #decided inliers <= count <= #decided + #undecided under the widened fp32 pose, undecided = a distance within a
               relative DELTA of inlier_m; the mean bracket width stays below 1 point.  DELTA: a component of R p + t - x
               carries a few fp32 ulps of coordinates up to 8 m, about 2e-6 m; against inlier_m >= 0.01 m that is 2e-4
               relative; DELTA is five times that.
  selection    exact: the first maximum of the probe's counts.
  refinement   per pose entry 2**-23 max(1, |ref|) + 10 d_perm, d_perm the reference's largest change over five
               permutations of its candidate list, measured here on every frame; covariance and cost per entry in units of
               sqrt(Sigma_ii Sigma_jj) (the cost relative to itself): 2**-23 + 10 (d_perm + d_round), d_round the reference's
               change when its final pose is rounded to fp32 and back; final inlier counts equal, with no candidate within a
               relative BAND of inlier_m (asserted); the reference must have moved the pose by more than 1e-3.
All inputs are deterministic from fixed seeds."""
import numpy as np
import pytest

import kabsch_ref as K
from kfnet_amd import _lib
from kfnet_amd.KFNet import kabsch

pytestmark = pytest.mark.gpu

DELTA = 1e-3
BAND = 1e-6
T0 = 5


class Probe(object):
    """One frame set on the device: the camera points, the hypotheses and counts, and the reference's candidate lists."""

    def __init__(self, records, depth, camera=None, ld=4, ldp=4, kw=None, t0=T0, cams=None):
        self.kw, self.t0, self.camera = dict(kw), t0, camera
        self.h, self.w = records.shape[1:3]
        if cams is None:
            cams = self.solver().cam_points(depth).cpu().numpy()
            assert np.array_equal(cams[..., 3] == 1.0, K.cam_points32(depth, camera)[..., 3] == 1.0)
        self.cams4, self.recs4 = cams, records
        self.recs = records if ld == 4 else K._wide(records, ld)
        self.cams = cams if ldp == 4 else K._wide(cams, ldp)
        self.samples, self.hp, self.counts = self.solver().hypotheses_probe(self.recs, self.cams, t0=t0)
        self.cands = [K.candidates(r, c, self.kw['min_confidence']) for r, c in zip(records, cams)]

    def solver(self, **more):
        kw = dict(self.kw)
        kw.update(more)
        return kabsch.KabschSolver(self.h, self.w, self.camera, **kw)

    def solve_unc(self, refine_iters, weighted):
        return self.solver(refine_iters=refine_iters, weighted=weighted).solve_unc(self.recs, self.cams, t0=self.t0)


_PROBES = {}


def _probe(name):
    if name not in _PROBES:
        s = K.stage_set(name)
        _PROBES[name] = Probe(s['records'], s['depth'], s['camera'], s['ld'], s['ldp'], s['kw'])
    return _PROBES[name]


# ---- the rules --------------------------------------------------------------------------------------------------------------

def check_samples_and_flags(pr):
    """Samples exact, validity flags exact, no triangle at the threshold.  Returns (valid, compared, small) counts."""
    valid = small = 0
    for b in range(pr.recs.shape[0]):
        Pc, X, _ = pr.cands[b]
        n = X.shape[0]
        for k in range(pr.kw['hypotheses']):
            s = K.draw_sample(pr.kw['seed'], pr.t0 + b, k, n) if n >= pr.kw['min_points'] else None
            assert list(pr.samples[b, k]) == (s if s is not None else [-1, -1, -1]), (b, k, pr.samples[b, k], s)
            if s is None:
                assert pr.counts[b, k] == -1 and np.isnan(pr.hp[b, k]).all(), (b, k)
                continue
            areas = (K.cross_norm(Pc[s]), K.cross_norm(X[s]))
            assert min(abs(a / K.MIN_CROSS - 1.0) for a in areas) > 1e-6, (b, k, areas)
            ref = K.hypothesis(Pc, X, s)
            assert (pr.counts[b, k] >= 0) == (ref is not None) == bool(np.isfinite(pr.hp[b, k]).all()), (b, k, areas)
            if ref is None:
                continue
            valid += 1
            if min(areas) < K.SMALL_AREA:
                small += 1
                continue
            d_alg = K.algorithm_spread(Pc, X, s)
            got, want = pr.hp[b, k].astype(np.float64), K.pose12(*ref)
            tol = 2.0 ** -23 * np.maximum(1.0, np.abs(want)) + 10 * d_alg
            assert (np.abs(got - want) <= tol).all(), (b, k, np.abs(got - want).max(), d_alg, areas)
    return valid, small


def check_scoring(pr):
    widths = []
    thr = K.f32(pr.kw['inlier_m'])
    for b in range(pr.recs.shape[0]):
        Pc, X, _ = pr.cands[b]
        valid = pr.counts[b] >= 0
        if not valid.any():
            continue
        lo, hi = K.score_brackets(pr.hp[b][valid], Pc, X, thr, DELTA)
        c = pr.counts[b][valid]
        bad = (c < lo) | (c > hi)
        assert not bad.any(), (b, np.nonzero(valid)[0][bad], c[bad], lo[bad], hi[bad])
        widths.append(hi - lo)
    return np.concatenate(widths) if widths else np.zeros(0)


def check_selection(pr, info):
    best = []
    for b in range(pr.recs.shape[0]):
        n = pr.cands[b][1].shape[0]
        k = K.first_max(pr.counts[b]) if n >= pr.kw['min_points'] else -1
        status = _lib.PNP_TOO_FEW_POINTS if n < pr.kw['min_points'] else (_lib.PNP_OK if k >= 0 else _lib.PNP_NO_HYPOTHESIS)
        assert (info[b, 0], info[b, 1], info[b, 3]) == (status, n, k), (b, info[b], status, n, k)
        best.append(k)
    return best


def check_refinement(pr, out, refine_iters, weighted):
    """Pose, covariance, cost, degrees of freedom and inlier count of every frame against the reference started from the
    device's selected fp32 hypothesis.  Returns how far the reference moved each pose."""
    poses, cov, quality, info = out
    ps, thr = pr.kw['point_sigma'], K.f32(pr.kw['inlier_m'])
    moved = []
    assert np.array_equal(cov.view(np.uint32), np.swapaxes(cov, 1, 2).copy().view(np.uint32))        # symmetric bit for bit
    for b in range(pr.recs.shape[0]):
        Pc, X, sig2 = pr.cands[b]
        k = K.first_max(pr.counts[b])
        assert info[b, 0] == _lib.PNP_OK and info[b, 3] == k and pr.counts[b, k] >= 16, (b, info[b], k)
        R0, t0 = K.widen(pr.hp[b, k])
        w = K.refine_weights(sig2, weighted, ps)
        R, t = K.refine(R0, t0, Pc, X, w, thr, refine_iters)
        ref = K.cam_to_world(R, t)
        Sg, cost, dof, inl = K.covariance(R, t, Pc, X, sig2, thr, ps)
        d_perm, d_perm_cov = K.permutation_spread(R0, t0, Pc, X, sig2, weighted, thr, refine_iters, ps)
        d_round = K.rounding_spread(R, t, Pc, X, sig2, thr, ps)
        margin = K.threshold_margin(R, t, Pc, X, thr)
        got = poses[b].astype(np.float64)
        moved.append(float(np.abs(ref - K.cam_to_world(R0, t0)).max()))
        nrm = np.sqrt(np.outer(np.diag(Sg), np.diag(Sg)))
        dc = float((np.abs(cov[b].astype(np.float64) - Sg) / nrm).max())
        dq = abs(float(quality[b, 0]) - cost) / cost
        print('frame %d: iters %d weighted %d, max |device - ref| %.3g, moved %.3g, margin %.3g, inliers %d / %d, d_perm %.3g '
              '%.3g, d_round %.3g, cov %.3g, cost %.3g' % (b, refine_iters, weighted, np.abs(got - ref).max(), moved[-1], margin,
                                                          info[b, 2], inl, d_perm, d_perm_cov, d_round, dc, dq))
        assert margin > BAND, (b, margin)
        if refine_iters == 0:
            assert np.array_equal(poses[b, :3].view(np.uint32), pr.hp[b, k].reshape(3, 4).view(np.uint32)), b      # a copy
            assert np.array_equal(got[3], [0., 0., 0., 1.])
        else:
            tol = 2.0 ** -23 * np.maximum(1.0, np.abs(ref)) + 10 * d_perm
            assert (np.abs(got - ref) <= tol).all(), (b, refine_iters, np.abs(got - ref).max())
        assert info[b, 2] == inl and quality[b, 1] == dof == 3 * inl - 6, (b, info[b], inl, quality[b])
        tol = 2.0 ** -23 + 10 * (d_perm_cov + d_round)
        assert np.isfinite(d_round) and dc <= tol and dq <= tol, (b, dc, dq, tol)
    return moved


# ---- 1. samples, flags, hypothesis poses, scoring -------------------------------------------------------------------------

@pytest.mark.parametrize('name', K.STAGE_SETS)
def test_samples_flags_and_hypotheses(name):
    pr = _probe(name)
    valid, small = check_samples_and_flags(pr)
    print('%s: %d valid hypotheses, %d below the small-triangle limit' % (name, valid, small))
    assert valid > 0.5 * pr.counts.size and small <= 0.05 * valid, (valid, small)


@pytest.mark.parametrize('name', K.STAGE_SETS)
def test_scoring_is_bracketed_for_every_hypothesis(name):
    pr = _probe(name)
    widths = check_scoring(pr)
    print('bracket width: mean %.4f, max %d over %d hypotheses' % (widths.mean(), widths.max(), widths.size))
    assert widths.size > 0.5 * pr.counts.size and widths.mean() < 1.0, (widths.size, widths.mean())


def test_limit_grid_counts_every_cell():
    """128 x 256 = 32 768 cells, the uint16 list's limit, without noise or outliers: every cell is a decided inlier of every
    valid hypothesis, so the bracket closes and all 32 768 must be counted."""
    kw = dict(hypotheses=64, min_points=16, seed=0, min_confidence=20., inlier_m=0.10, point_sigma=0.01)
    recs, depth, _ = K.synthetic_frames_rgbd(806, 1, 128, 256, 0.0, depth_noise=0.0, noise=False)
    pr = Probe(recs, depth, kw=kw)
    assert pr.cands[0][1].shape[0] == 32768
    valid, _ = check_samples_and_flags(pr)
    widths = check_scoring(pr)
    assert valid > 32 and widths.max() == 0 and (pr.counts[0][pr.counts[0] >= 0] == 32768).all(), (valid, widths.max())
    poses, cov, quality, info = pr.solve_unc(10, True)
    assert tuple(info[0, :3]) == (_lib.PNP_OK, 32768, 32768) and info[0, 3] == K.first_max(pr.counts[0])
    assert np.isfinite(cov).all() and quality[0, 1] == 3 * 32768 - 6


# ---- 2. selection ---------------------------------------------------------------------------------------------------------

def tie_grids():
    """Small grids on which equal counts are the normal case; the tight inlier_m of the last one spreads the counts, so that
    the first maximum also falls late in the list."""
    kw = dict(min_points=16, seed=0, min_confidence=20., inlier_m=0.10, point_sigma=0.01)
    out = []
    recs, depth, _ = K.synthetic_frames_rgbd(811, 8, 4, 5, 0.3)                                # n = 20
    out.append(('4x5', recs, depth, kw))
    recs, depth, _ = K.synthetic_frames_rgbd(812, 8, 5, 7, 0.0, depth_noise=0.0, noise=False)   # every valid hypothesis ties
    for b in range(8):
        recs[b].reshape(-1, 4)[:3 + 2 * b, 3] = 1.0                                             # list index != cell index
    out.append(('5x7', recs, depth, kw))
    recs, depth, _ = K.synthetic_frames_rgbd(813, 8, 6, 7, 0.3)                                # n = 42
    out.append(('6x7', recs, depth, dict(kw, inlier_m=0.03)))
    return out


def test_selection_is_the_first_maximum_of_the_device_counts():
    real_tie = winner_past_256 = cross_wave = 0
    for name, recs, depth, kw in tie_grids():
        cams = None
        for H in (1, 63, 64, 65, 255, 256, 257, 1024):
            pr = Probe(recs, depth, kw=dict(kw, hypotheses=H), t0=3, cams=cams)
            cams = pr.cams4
            _, _, _, info = pr.solve_unc(10, False)
            best = check_selection(pr, info)
            assert np.array_equal(kabsch.select_probe(pr.counts), np.array(best)), (name, H)
            for b, k in enumerate(best):
                if name == '5x7' and k >= 0:
                    n = pr.cands[b][1].shape[0]
                    assert (pr.counts[b][pr.counts[b] >= 0] == n).all(), (b, pr.counts[b])
                if k < 0:
                    continue
                tied = np.nonzero(pr.counts[b] == pr.counts[b, k])[0]
                real_tie += tied.size >= 2
                winner_past_256 += k >= 256
                cross_wave += bool(((tied % 256) // 64 != (k % 256) // 64).any())
    print('ties %d, winners >= 256: %d, ties across waves %d' % (real_tie, winner_past_256, cross_wave))
    assert real_tie >= 1 and winner_past_256 >= 1 and cross_wave >= 1, (real_tie, winner_past_256, cross_wave)


def test_selection_probe_on_planted_counts():
    """The rule alone: maxima planted on both sides of every lane, wave and 256-block boundary, with ties behind them."""
    rng = np.random.default_rng(821)
    for H in (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 1023, 1024):
        rows = [np.full(H, -1, np.int32)]
        for first in sorted({0, H - 1, H // 2, min(63, H - 1), min(64, H - 1), min(255, H - 1), min(256, H - 1), min(767, H - 1)}):
            c = rng.integers(-1, 40, size=H).astype(np.int32)
            c[first] = 50
            c[first + 1:][rng.random(H - first - 1) < 0.3] = 50          # ties behind the first maximum
            rows.append(c)
        counts = np.stack(rows)
        want = np.array([K.first_max(c) for c in counts])
        assert want[0] == -1 and np.array_equal(kabsch.select_probe(counts), want), H


# ---- 3. refinement, covariance, quality ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('refine_iters', [0, 1, 3, 10])
@pytest.mark.parametrize('name', K.STAGE_SETS)
def test_refinement_and_covariance_match_the_fp64_closed_form(name, refine_iters, weighted):
    pr = _probe(name)
    out = pr.solve_unc(refine_iters, weighted)
    check_selection(pr, out[3])
    moved = check_refinement(pr, out, refine_iters, weighted)
    if refine_iters >= 1:
        assert min(moved) > 1e-3, moved           # else agreeing with the reference proves nothing
    poses, info = pr.solver(refine_iters=refine_iters, weighted=weighted).solve(pr.recs, pr.cams, t0=pr.t0)
    assert np.array_equal(poses.view(np.uint32), out[0].view(np.uint32)) and np.array_equal(info, out[3])    # cov = NULL


def test_depth_maps_and_camera_points_give_the_same_bits():
    s = K.stage_set('15x20_registered')
    pr = _probe('15x20_registered')
    a = pr.solve_unc(10, True)
    b = pr.solver(refine_iters=10, weighted=True).solve_unc(s['records'], s['depth'], t0=pr.t0)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    d = pr.solver(refine_iters=10, weighted=True).solve_unc(s['records'], pr.cams.astype(np.float64), t0=pr.t0)   # rounded once
    for x, y in zip(a, d):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    with pytest.raises(ValueError):
        pr.solver().solve(s['records'], pr.cams.astype(np.int32), t0=pr.t0)
    import torch
    c = pr.solver(refine_iters=10, weighted=True).solve_unc(torch.from_numpy(s['records']).cuda(),
                                                             torch.from_numpy(s['depth'].view(np.int16)).cuda(), t0=pr.t0)
    for x, y in zip(a, c):
        assert torch.is_tensor(y) and np.array_equal(x.view(np.uint32), y.cpu().numpy().view(np.uint32))


# ---- 4. edges ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [3, 4, 16])
def test_short_candidate_lists(n):
    """With few candidates the 16-draw limit bites: at n = 3 some hypotheses never draw 3 distinct indices.  The candidates
    are thinned three ways: by confidence, by a raw depth outside the validity window (0 and 65535) and by a NaN record."""
    kw = dict(hypotheses=256, min_points=3, seed=0, min_confidence=20., inlier_m=0.10, point_sigma=0.01)
    recs, depth, _ = K.synthetic_frames_rgbd(831, 4, 6, 7, 0.0)
    rng = np.random.default_rng(832)
    for b in range(4):
        order = rng.permutation(42)
        drop = order[n:]
        cells = recs[b].reshape(-1, 4)
        cells[drop[0::3], 3] = 1.0
        cells[drop[1::3], 0] = np.nan
        rr, cc = np.divmod(drop[2::3], 7)
        depth[b][8 * rr, 8 * cc] = np.where(np.arange(rr.size) % 2 == 0, 0, 65535)
    pr = Probe(recs, depth, kw=kw, t0=0)
    for b in range(4):
        assert pr.cands[b][1].shape[0] == n
    check_samples_and_flags(pr)
    none = int((pr.samples < 0).any(-1).sum())
    if n == 3:
        assert 0 < none < 4 * 256, none                             # both kinds of row
    check_scoring(pr)
    _, _, _, info = pr.solve_unc(10, True)
    check_selection(pr, info)
    assert (info[:, 1] == n).all() and (info[:, 2] <= n).all()


def test_too_few_points_status():
    kw = dict(hypotheses=64, min_points=16, seed=0, min_confidence=20., inlier_m=0.10, point_sigma=0.01)
    recs, depth, _ = K.synthetic_frames_rgbd(841, 3, 6, 7, 0.0)
    recs[1].reshape(-1, 4)[15:, 3] = 1.0                            # 15 candidates
    pr = Probe(recs, depth, kw=kw, t0=0)
    poses, cov, quality, info = pr.solve_unc(10, False)
    assert tuple(info[1]) == (_lib.PNP_TOO_FEW_POINTS, 15, 0, -1), info[1]
    assert np.isnan(poses[1]).all() and np.isnan(cov[1]).all() and np.isnan(quality[1]).all()
    assert (pr.samples[1] == -1).all() and (pr.counts[1] == -1).all()
    assert (info[[0, 2], 0] == _lib.PNP_OK).all() and np.isfinite(poses[[0, 2]]).all()


def test_no_hypothesis_status_without_touching_neighbours():
    """42 confident cells whose scene points lie on one line: every sampled scene triangle is degenerate."""
    kw = dict(hypotheses=256, min_points=16, seed=0, min_confidence=20., inlier_m=0.10, point_sigma=0.01)
    recs, depth, _ = K.synthetic_frames_rgbd(851, 3, 15, 20, 0.3)
    recs[1, ..., 3] = 1.0
    recs[1, 7, :, 3] = 100.0
    recs[1, 8, :, 3] = 100.0
    recs[1, 9, :2, 3] = 100.0
    cells = recs[1].reshape(-1, 4)
    conf = cells[:, 3] > 20.0
    assert conf.sum() == 42
    cells[conf, :3] = np.stack([0.125 * np.arange(42), np.zeros(42), np.full(42, 2.0)], 1)
    pr = Probe(recs, depth, kw=kw, t0=0)
    ref = K.ransac(recs[1:2], pr.cams4[1:2], t0=1)
    assert tuple(ref[3][0]) == (K.NO_HYPOTHESIS, 42, 0, -1)
    poses, cov, quality, info = pr.solve_unc(10, True)
    assert tuple(info[1]) == (_lib.PNP_NO_HYPOTHESIS, 42, 0, -1), info[1]
    assert np.isnan(poses[1]).all() and np.isnan(cov[1]).all() and np.isnan(quality[1]).all()
    solver = pr.solver(refine_iters=10, weighted=True)
    for b in (0, 2):
        pb, cb, qb, ib = solver.solve_unc(recs[b:b + 1], pr.cams4[b:b + 1], t0=b)
        assert ib[0, 0] == _lib.PNP_OK
        for x, y in ((pb[0], poses[b]), (cb[0], cov[b]), (qb[0], quality[b])):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), b
        assert np.array_equal(ib[0], info[b]), b


def test_a_frame_alone_equals_its_pose_in_a_batch_and_launches_repeat():
    pr = _probe('9x13')
    first = pr.solve_unc(10, True)
    again = pr.solve_unc(10, True)
    for x, y in zip(first, again):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    solver = pr.solver(refine_iters=10, weighted=True)
    for b in (0, 3, 7):
        alone = solver.solve_unc(pr.recs[b:b + 1], pr.cams[b:b + 1], t0=pr.t0 + b)
        for x, y in zip(alone, first):
            assert np.array_equal(x[0].view(np.uint32), y[b].view(np.uint32)), b
    probe_again = pr.solver().hypotheses_probe(pr.recs, pr.cams, t0=pr.t0)
    for x, y in zip(probe_again, (pr.samples, pr.hp, pr.counts)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


# ---- 5. the program, 64x96 ----------------------------------------------------------------------------------------------------

def test_command_line_solves_rendered_frames_as_the_solver_does(tmp_path, capsys):
    """Frames of synth.synthetic_scene rendered at 64x96 with their depth maps: the scene coordinates of every eighth pixel
    as coord_<i>.npy (confidence 100 where the renderer hit the model), the depth maps as 16-bit PNGs.  KFNet.pnp
    --depth_list writes the poses and covariances that KabschSolver.solve_unc returns for the same arrays, bit for bit, and
    they are the cameras the frames were rendered from: the records are exact and the depth is rounded to the millimetre,
    so a camera point is off by at most 0.5 mm x |ray| / z < 1 mm; 5 mm and 0.5 degrees leave room for lever arms of 0.1 m."""
    from kfnet_amd import render, synth
    from kfnet_amd.KFNet import pnp
    from kfnet_amd.labels import DepthCamera
    cam = DepthCamera(80., 80., 48., 32.)
    vertices, colors, triangles = synth.synthetic_scene(3, cells=8)
    gt = synth.synthetic_trajectory(5, 3)
    labels, depth, _, _ = render.Renderer(vertices, triangles, colors, image_size=(64, 96), batch=5, stride=1,
                                          camera=cam).render(gt)
    recs = labels.cpu().numpy()[:, ::8, ::8].copy()
    depth = depth.cpu().numpy()
    recs[..., 3] *= 100.0
    assert recs.shape == (5, 8, 12, 4) and ((recs[..., 3] == 100.0).sum((1, 2)) >= 48).all()
    coords, depths, poses = [], [], []
    for i in range(5):
        coords.append(str(tmp_path / ('coord_%d.npy' % i)))
        depths.append(str(tmp_path / ('frame-%06d.depth.png' % i)))
        poses.append(str(tmp_path / ('frame-%06d.pose.txt' % i)))
        np.save(coords[-1], recs[i])
        render.write_png(depths[-1], depth[i])
        pnp.write_pose(poses[-1], gt[i])
    for name, paths in (('coord_list.txt', coords), ('depth_list.txt', depths), ('pose_list.txt', poses)):
        (tmp_path / name).write_text('\n'.join(paths) + '\n')
    out = tmp_path / 'out'
    flags = ['--focal_x', '80', '--focal_y', '80', '--u', '48', '--v', '32', '--hypotheses', '64', '--batch', '3']
    assert pnp.main([str(tmp_path / 'coord_list.txt'), str(out), '--depth_list', str(tmp_path / 'depth_list.txt'), '--gt',
                     str(tmp_path / 'pose_list.txt'), '--weighted', '--covariance'] + flags) == 0
    text = capsys.readouterr().out
    assert '5 poses written' in text and '(0 frames without a pose)' in text and 'median rotation error' in text
    solver = kabsch.KabschSolver(8, 12, cam, hypotheses=64, weighted=True)
    want = pnp.solve_unc_in_batches(solver, recs, 3, depth=depth)
    got = np.stack([pnp.read_pose(str(out / ('pose_%d.txt' % i))) for i in range(5)])
    got_cov = np.stack([pnp.read_covariance(str(out / ('pose_cov_%d.txt' % i))) for i in range(5)])
    assert (want[3][:, 0] == _lib.PNP_OK).all()
    assert np.array_equal(got.astype(np.float32).view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got_cov.astype(np.float32).view(np.uint32), want[1].view(np.uint32))
    rot, trans = pnp.pose_errors(got, gt)
    print('rotation errors (deg)', rot, 'translation errors (m)', trans)
    assert (rot < 0.5).all() and (trans < 0.005).all(), (rot, trans)
    # without --weighted / --covariance: solve's poses, no covariance files
    out2 = tmp_path / 'out2'
    assert pnp.main([str(tmp_path / 'coord_list.txt'), str(out2), '--depth_list', str(tmp_path / 'depth_list.txt')] + flags) == 0
    plain = pnp.solve_in_batches(kabsch.KabschSolver(8, 12, cam, hypotheses=64), recs, 3, depth=depth)
    got2 = np.stack([pnp.read_pose(str(out2 / ('pose_%d.txt' % i))) for i in range(5)])
    assert np.array_equal(got2.astype(np.float32).view(np.uint32), plain[0].view(np.uint32))
    assert not (out2 / 'pose_cov_0.txt').exists()


# ---- 6. the eval programs, 64x96: --pose_depth ------------------------------------------------------------------------------

def _env():
    import os
    e = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT'):
        e.pop(k, None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e['PYTHONPATH'] = root + os.pathsep + e.get('PYTHONPATH', '')
    e['KFN_DIST_BACKEND'] = 'gloo'
    return e, root


def _run(cmd):
    import subprocess
    import sys
    env, root = _env()
    r = subprocess.run([sys.executable] + cmd, cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def _same(one, two, names):
    for name in names:
        with open(str(one / name), 'rb') as a, open(str(two / name), 'rb') as b:
            assert a.read() == b.read(), name


def test_eval_pose_depth_equals_pnp_depth_list_and_the_sharded_run(tmp_path):
    """Rendered frames of synth.synthetic_scene with their depth maps through KFNet.eval --pose_depth --pose_weighted, then
    KFNet.pnp --depth_list on the written coord_<i>.npy: the same pose_<i>.txt and pose_cov_<i>.txt, byte for byte; a
    two-rank gloo run on this GPU writes the single process's files; --pose without the flag stays the PnP path.  The
    weights are random, so the records' confidences may leave no frame solvable: this test pins the programs' plumbing (flags,
    lists, files, ranks); that the poses are right, frame by frame and chunk by chunk, is the DepthPoseSolver test's."""
    import socket
    from kfnet_amd import render, synth
    T = 6
    vertices, colors, triangles = synth.synthetic_scene(3, cells=8)
    _, depth, frames, _ = render.Renderer(vertices, triangles, colors, image_size=(64, 96), batch=T, stride=1).render(
        synth.synthetic_trajectory(T, 3))
    depth, frames = depth.cpu().numpy(), frames.cpu().numpy()
    inp = tmp_path / 'in'
    inp.mkdir()
    images, depths = [], []
    for i in range(T):
        images.append(str(inp / ('frame-%06d.color.png' % i)))
        depths.append(str(inp / ('frame-%06d.depth.png' % i)))
        render.write_png(images[-1], frames[i])
        render.write_png(depths[-1], depth[i])
    (inp / 'image_list.txt').write_text('\n'.join(images) + '\n')
    (inp / 'depth_list.txt').write_text('\n'.join(depths) + '\n')
    np.savetxt(str(inp / 'transform.txt'), synth.synthetic_transform())
    small = ['--scene', 'chess', '--input_folder', str(inp), '--random_weights', '--height', '64', '--width', '96']
    one, two, three, four, five = (tmp_path / n for n in ('one', 'two', 'three', 'four', 'five'))
    for d in (one, two, three, four, five):
        d.mkdir()
    out = _run(['-m', 'kfnet_amd.KFNet.eval', '--output_folder', str(one), '--pose_depth', '--pose_weighted'] + small)
    import re
    solved = re.search(r'poses: (\d+) of (\d+) frames solved', out)
    assert solved and int(solved.group(2)) == T, out[-500:]
    print('random weights: %s of %d frames solved (solvable frames: the DepthPoseSolver test below)' % (solved.group(1), T))
    pose_files = ['pose_%d.txt' % i for i in range(T)] + ['pose_cov_%d.txt' % i for i in range(T)]
    coord_files = ['coord_%d.npy' % i for i in range(T)]
    (tmp_path / 'coord_list.txt').write_text('\n'.join(str(one / n) for n in coord_files) + '\n')
    _run(['-m', 'kfnet_amd.KFNet.pnp', str(tmp_path / 'coord_list.txt'), str(two), '--depth_list', str(inp / 'depth_list.txt'),
          '--weighted', '--covariance'])
    _same(one, two, pose_files)
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    _run(['-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1', '--master-port',
          str(port), '-m', 'kfnet_amd.KFNet.eval', '--output_folder', str(three), '--pose_depth', '--pose_weighted'] + small)
    _same(one, three, pose_files + coord_files)
    # without the flag: the PnP path, as KFNet.pnp without --depth_list solves the same records
    _run(['-m', 'kfnet_amd.KFNet.eval', '--output_folder', str(four), '--pose'] + small)
    _run(['-m', 'kfnet_amd.KFNet.pnp', str(tmp_path / 'coord_list.txt'), str(five)])
    _same(one, four, coord_files)
    _same(four, five, pose_files[:T])
    assert not (four / 'pose_cov_0.txt').exists()


# ---- 7. modes.DepthPoseSolver: every frame is solved with its own depth map ------------------------------------------------

def test_depth_pose_solver_solves_rendered_frames_chunked_at_t0_above_zero(tmp_path, capsys):
    """The eval test above runs random weights, whose confidences may leave no frame solvable; it pins the plumbing only.
    Here the one place that makes --pose_depth's poses (modes.solver_of -> DepthPoseSolver, write_poses, ChunkOutputs.add) gets
    records that can be solved -- the rendered scene coordinates of every eighth pixel with confidence 100 -- and the depth
    PNGs of the run: all T frames must come out OK, finite, equal to KabschSolver on the same arrays bit for bit, chunked
    and at t0 > 0, and at the rendering cameras (bound as in the command-line test).  A frame solved with another
    frame's depth map must not give these poses: the depth is read, and read for the right frame."""
    import os
    import types
    import torch
    from kfnet_amd import modes, render, synth
    from kfnet_amd.KFNet import pnp
    from kfnet_amd.labels import DepthCamera
    T = 7
    vertices, colors, triangles = synth.synthetic_scene(3, cells=8)
    gt = synth.synthetic_trajectory(T, 3)
    labels, depth, _, _ = render.Renderer(vertices, triangles, colors, image_size=(64, 96), batch=T, stride=1).render(gt)
    recs = labels.cpu().numpy()[:, ::8, ::8].copy()
    depth = depth.cpu().numpy()
    recs[..., 3] *= 100.0
    assert ((recs[..., 3] == 100.0).sum((1, 2)) >= 48).all()
    paths = [str(tmp_path / ('frame-%06d.depth.png' % i)) for i in range(T)]
    for p, d in zip(paths, depth):
        render.write_png(p, d)
    opts = modes.DepthPoseOptions(True, paths)
    solver = modes.solver_of(opts, 8, 12)
    assert isinstance(solver, modes.DepthPoseSolver) and solver.weighted
    ref = kabsch.KabschSolver(8, 12, DepthCamera(), weighted=True)
    want = pnp.solve_unc_in_batches(ref, recs, 3, depth=depth)
    assert (want[3][:, 0] == _lib.PNP_OK).all() and np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    rot, trans = pnp.pose_errors(want[0], gt)
    print('rotation errors (deg)', rot, 'translation errors (m)', trans)
    assert (rot < 0.5).all() and (trans < 0.005).all(), (rot, trans)
    for lo, n in ((0, 3), (3, 4), (6, 1)):                                    # chunks, two of them at t0 > 0
        got = solver.solve_unc(recs[lo:lo + n], t0=lo)
        for x, y in zip(got, want):
            assert np.array_equal(x.view(np.uint32), y[lo:lo + n].view(np.uint32)), lo
        plain = solver.solve(recs[lo:lo + n], t0=lo)
        assert np.array_equal(plain[0].view(np.uint32), want[0][lo:lo + n].view(np.uint32)) and (plain[1][:, 0] == 0).all()
    wrong = ref.solve_unc(recs[3:7], depth[0:4], t0=3)                        # the depth of frames 0..3 under frames 3..6
    assert not np.array_equal(wrong[0].view(np.uint32), want[0][3:7].view(np.uint32))
    with pytest.raises(ValueError):
        solver.solve(recs[5:7], t0=6)                                         # frame 7 has no depth map listed
    # write_poses (the single-process runs)
    out = tmp_path / 'out'
    out.mkdir()
    capsys.readouterr()
    poses, info = modes.write_poses(recs, str(out), batch=3, pose=opts)
    assert 'poses: %d of %d frames solved' % (T, T) in capsys.readouterr().out
    assert np.array_equal(poses.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(info, want[3])
    files = np.stack([pnp.read_pose(str(out / ('pose_%d.txt' % i))) for i in range(T)])
    covs = np.stack([pnp.read_covariance(str(out / ('pose_cov_%d.txt' % i))) for i in range(T)])
    assert np.array_equal(files.astype(np.float32).view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(covs.astype(np.float32).view(np.uint32), want[1].view(np.uint32))
    # ChunkOutputs.add (a sharded rank): its frames alone, the device records view, t0 = the global frame index
    out2 = tmp_path / 'out2'
    out2.mkdir()
    eng = types.SimpleNamespace(h=8, w=12, H=64, W=96, torch=torch)
    res = modes.ChunkOutputs(eng, T, str(out2), pose=opts).add(3, torch.from_numpy(recs[3:]).cuda())
    assert res['metrics'] is None and (res['info'][:, 0] == _lib.PNP_OK).all()
    assert np.array_equal(res['poses'].view(np.uint32), want[0][3:].view(np.uint32))
    assert sorted(os.listdir(str(out2))) == sorted(['pose_%d.txt' % i for i in range(3, T)] + ['pose_cov_%d.txt' % i for i in range(3, T)])
    for i in range(3, T):
        with open(str(out / ('pose_%d.txt' % i)), 'rb') as a, open(str(out2 / ('pose_%d.txt' % i)), 'rb') as b:
            assert a.read() == b.read(), i
