"""kfn_pnp_ransac_guided / kfn_pnp_hypotheses_guided on the device against tests/pnp_guided_ref.py (DESIGN.md 5c "Guided
sampling").

The cumulative weights, the candidate counts and every sample are integers and must equal the reference's.  Everything
behind the draws is the uniform path's launches, so it is checked by that path's rules, with the helpers and tolerances
of test_gpu_pnp_stages.py: valid hypotheses to 1e-4 (test_gpu_pnp.py), counts inside pnp_ref.score_brackets with a mean
width below one point, selection as the first maximum of the device's own counts, refinement within
2**-23 * max(1, |ref|) + 10 * d_perm of pnp_ref.refine started from the device's selected hypothesis.

Shapes: the smallest that reach each path of the scan and the search -- 4x4 (n = 16 = min_points), 9x13 (n < 256: one
partial chunk, totals above 2**32 with squared weights), 15x20 with ld = 7 and NaN in the extra channels (two chunks: a
carry), 37x53 with fx != fy and an off-centre principal point, and 128x256 (the limit) once."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pnp_guided_ref as G
import pnp_ref as P
import test_gpu_pnp_stages as S
import test_pnp_guided_host as HOST
from kfnet_amd import _lib
from kfnet_amd.KFNet import pnp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLING = {G.CONFIDENCE: 'confidence', G.CONFIDENCE_SQ: 'confidence2'}
MODES = sorted(SAMPLING)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _with_confidence(recs, seed, lo=25.0, hi=1000.0):
    """The frames with a confidence log-uniform in lo .. hi in every cell (float32)."""
    rng = np.random.default_rng(seed)
    recs = recs.copy()
    recs[..., 3] = np.exp(rng.uniform(np.log(lo), np.log(hi), size=recs.shape[:3])).astype(np.float32)
    return recs


class GuidedProbe(S.Probe):
    """test_gpu_pnp_stages.Probe of a guided solver (kw carries `sampling`), with the device's cum and n."""

    def __init__(self, recs, kw, t0=0):
        self.recs, self.kw, self.t0 = recs, kw, t0
        self.h, self.w = recs.shape[1:3]
        self.samples, self.hp, self.counts, self.cum, self.n = \
            pnp.PnPSolver(self.h, self.w, **kw).hypotheses_probe(recs, t0=t0, with_cdf=True)
        self.cands = [P.candidates(r[..., :4], kw['min_confidence'], kw['cell_stride']) for r in recs]


def _mode_of(kw):
    return {v: k for k, v in SAMPLING.items()}[kw['sampling']]


def check_draws(pr):
    """cum, n and samples against the reference's integers; valid hypotheses to 1e-4.  Returns (rows without a sample,
    hypotheses valid on both sides)."""
    kw = pr.kw
    H = kw['hypotheses']
    none = both_valid = 0
    for b in range(pr.recs.shape[0]):
        rs, rp, rc, X, _, cum = G.hypotheses_guided(
            pr.recs[b][..., :4], pr.t0 + b, H, _mode_of(kw), kw.get('confidence_cap', 1000.0), kw['seed'], kw['fx'], kw['fy'],
            kw['u'], kw['v'], kw['min_confidence'], kw['inlier_px'], kw['cell_stride'], kw['min_points'], score=False)
        n = X.shape[0]
        assert pr.n[b] == n == cum.size, (b, pr.n[b], n)
        assert np.array_equal(pr.cum[b, :n], cum), (b, np.nonzero(pr.cum[b, :n] != cum)[0][:5])
        assert not pr.cum[b, n:].any(), b                                # nothing written behind the n entries
        assert np.array_equal(pr.samples[b], rs), (b, np.nonzero((pr.samples[b] != rs).any(1))[0][:5])
        assert (pr.counts[b][(rs < 0).any(1)] == -1).all(), b
        both = (pr.counts[b] >= 0) & (rc >= 0)
        if n >= kw['min_points']:
            assert ((pr.counts[b] >= 0) == (rc >= 0)).mean() >= 0.99, b
        if both.any():
            assert np.abs(pr.hp[b][both] - rp[both]).max() < 1e-4, b
        none += int((rs < 0).any(1).sum())
        both_valid += int(both.sum())
    return none, both_valid


# ---- exact stages, hypotheses and counts ----------------------------------------------------------------------------------

def _kw(mode, **kw):
    return S._kw(sampling=SAMPLING[mode], **kw)


def _grid4x4(mode):
    kw = _kw(mode)
    recs = _with_confidence(S._frames(701, 4, 4, 4, 0.0, 0.0, kw), 702, 21.0, 400.0)
    recs[1] = HOST.exhaustion_frame()
    return recs, kw


def _grid9x13(mode):
    kw = _kw(mode)
    recs = _with_confidence(S._frames(703, 3, 9, 13, 0.2, 0.01, kw), 704)
    recs[0, ..., 3] = HOST.spread_9x13()[..., 3]                          # total 2.25 * 2^32 with squared weights
    recs[2, 4, 5, 3] = np.inf                                             # weighs as the cap
    recs[2, 4, 6, 3] = 20.0                                               # == threshold: no candidate
    recs[2, 0, 0, 1] = np.nan                                             # no candidate either
    return recs, kw


def _grid15x20_ld7(mode):
    kw = _kw(mode)
    recs = _with_confidence(S._frames(705, 4, 15, 20, 0.3, 0.01, kw), 706)
    recs[1, ..., 3][np.random.default_rng(707).random((15, 20)) < 0.2] = 10.0      # list index != cell index
    wide = np.full(recs.shape[:3] + (7,), np.nan, np.float32)            # the extra channels must not be read
    wide[..., :4] = recs
    return wide, kw


def _grid37x53(mode):
    kw = _kw(mode, fx=500., fy=560., u=210.5, v=140.25, confidence_cap=300.0)
    return _with_confidence(S._frames(708, 3, 37, 53, 0.3, 0.01, kw), 709), kw


GRIDS = {'4x4': _grid4x4, '9x13': _grid9x13, '15x20_ld7': _grid15x20_ld7, '37x53': _grid37x53}
_PROBES = {}


def _probe(grid, mode):
    if (grid, mode) not in _PROBES:
        recs, kw = GRIDS[grid](mode)
        _PROBES[grid, mode] = GuidedProbe(recs, kw, t0=5)
    return _PROBES[grid, mode]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('grid', sorted(GRIDS))
def test_cum_n_samples_hypotheses_and_counts(grid, mode):
    pr = _probe(grid, mode)
    none, both_valid = check_draws(pr)
    if grid == '4x4':
        # the exhaustion frame: some rows without a sample under weights, all under squared weights
        ex = (pr.samples[1] < 0).any(1).sum()
        assert (0 < ex < 256) if mode == G.CONFIDENCE else ex == 256, ex
    if grid == '9x13' and mode == G.CONFIDENCE_SQ:
        assert int(pr.cum[0, pr.n[0] - 1]) > 2 << 32
    assert both_valid > 0.3 * pr.counts.size or grid == '4x4', both_valid
    widths = S.check_scoring(pr)
    print('%s mode %d: %d rows without a sample, %d valid hypotheses, bracket width mean %.3f'
          % (grid, mode, none, both_valid, widths.mean()))
    assert widths.size and widths.mean() < 1.0, widths.mean()
    for iters in (0, 10):
        _, info = pr.solve(iters)
        S.check_selection(pr, info)


@pytest.mark.parametrize('grid', ['9x13', '15x20_ld7', '37x53'])
def test_refinement_behind_guided_draws(grid):
    pr = _probe(grid, G.CONFIDENCE)
    poses, info = pr.solve(10)
    assert (info[:, 0] == _lib.PNP_OK).all(), info
    S.check_refinement(pr, poses, info, 10)


def test_the_grid_limit():
    """128x256 once: 128 chunks of the scan, 15 steps of the search, a clean frame so that the scoring bracket closes."""
    kw = _kw(G.CONFIDENCE_SQ, hypotheses=64, u=1024., v=512.)
    recs = _with_confidence(S._frames(606, 1, 128, 256, 0.0, 0.0, kw), 710)
    pr = GuidedProbe(recs, kw, t0=5)
    check_draws(pr)
    widths = S.check_scoring(pr)
    assert widths.size and widths.mean() < 1.0, widths.mean()
    _, info = pr.solve(10)
    S.check_selection(pr, info)
    assert info[0, 1] == 32768


@pytest.mark.parametrize('mode', MODES)
def test_too_few_candidates_gives_status_and_nan_without_touching_neighbours(mode):
    kw = _kw(mode)
    recs = _with_confidence(S._frames(711, 3, 9, 13, 0.2, 0.01, kw), 712)
    bad = recs.copy()
    bad[1, ..., 3] = 1.0
    bad[1, 0, :10, 3] = 100.0                                  # 10 candidates < min_points 16
    solver = pnp.PnPSolver(9, 13, **kw)
    poses, info = solver.solve(bad)
    assert tuple(info[1]) == (_lib.PNP_TOO_FEW_POINTS, 10, 0, -1)
    assert np.isnan(poses[1]).all()
    samples, hp, counts, cum, n = solver.hypotheses_probe(bad, with_cdf=True)
    assert n[1] == 10 and (samples[1] == -1).all() and (counts[1] == -1).all() and np.isnan(hp[1]).all()
    ref_poses, ref_info = solver.solve(recs)
    for b in (0, 2):
        assert ref_info[b, 0] == _lib.PNP_OK
        assert np.array_equal(_bits(poses[b]), _bits(ref_poses[b])) and np.array_equal(info[b], ref_info[b]), b


# ---- identity with the uniform path ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', MODES)
def test_constant_confidence_gives_the_uniform_path_bit_for_bit(mode):
    for h, w, conf in ((15, 20, 100.0), (37, 53, 20.1)):
        kw = S._kw()
        recs = S._frames(720 + h, 4, h, w, 0.4, 0.01, kw)
        recs[..., 3] = np.float32(conf)
        uni = pnp.PnPSolver(h, w, **kw)
        gui = pnp.PnPSolver(h, w, sampling=SAMPLING[mode], **kw)
        pu, iu = uni.solve(recs, t0=3)
        pg, ig = gui.solve(recs, t0=3)
        assert (iu[:, 0] == _lib.PNP_OK).all()
        assert np.array_equal(_bits(pu), _bits(pg)) and np.array_equal(iu, ig), (h, w)
        su, gs = uni.hypotheses_probe(recs, t0=3), gui.hypotheses_probe(recs, t0=3)
        assert np.array_equal(su[0], gs[0]) and np.array_equal(_bits(su[1]), _bits(gs[1])) and np.array_equal(su[2], gs[2])
        for weighted in (False, True):
            uni_w = pnp.PnPSolver(h, w, weighted=weighted, pixel_sigma=0.7, **kw)
            gui_w = pnp.PnPSolver(h, w, weighted=weighted, pixel_sigma=0.7, sampling=SAMPLING[mode], **kw)
            a, b = uni_w.solve_unc(recs, t0=3), gui_w.solve_unc(recs, t0=3)
            for x, y in zip(a[:3], b[:3]):
                assert np.array_equal(_bits(x), _bits(y)), (h, w, weighted)
            assert np.array_equal(a[3], b[3]) and np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
            if not weighted:
                assert np.array_equal(_bits(a[0]), _bits(pu))


# ---- independence and repeatability --------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', MODES)
def test_frame_alone_equals_frame_in_batch_and_launches_repeat(mode):
    kw = _kw(mode)
    recs = _with_confidence(S._frames(730, 8, 15, 20, 0.4, 0.01, kw), 731)
    solver = pnp.PnPSolver(15, 20, weighted=True, **kw)
    p1, i1 = solver.solve(recs)
    p2, i2 = solver.solve(recs)
    assert np.array_equal(_bits(p1), _bits(p2)) and np.array_equal(i1, i2)
    u1, u2 = solver.solve_unc(recs), solver.solve_unc(recs)
    for x, y in zip(u1, u2):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    q1, q2 = solver.hypotheses_probe(recs, with_cdf=True), solver.hypotheses_probe(recs, with_cdf=True)
    for x, y in zip(q1, q2):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    for k in (0, 3, 7):
        pk, ik = solver.solve(recs[k:k + 1], t0=k)
        assert np.array_equal(_bits(pk[0]), _bits(p1[k])) and np.array_equal(ik[0], i1[k]), k
        uk = solver.solve_unc(recs[k:k + 1], t0=k)
        for x, y in zip(uk, u1):
            assert np.array_equal(x[0].view(np.uint32), y[k].view(np.uint32)), k


@pytest.mark.parametrize('cs', [4, 16])
def test_cell_strides(cs):
    kw = _kw(G.CONFIDENCE_SQ, cell_stride=cs, u=10. * cs, v=7.5 * cs)
    pr = GuidedProbe(_with_confidence(S._frames(740 + cs, 3, 15, 20, 0.3, 0.01, kw), 741), kw, t0=5)
    check_draws(pr)
    S.check_stages(pr)


# ---- end to end ------------------------------------------------------------------------------------------------------------

def _runner_up_reaches_the_winner(hp, counts, X, pix, kw):
    """Whether a device count anywhere inside its scoring bracket could make another hypothesis the first maximum."""
    valid = np.nonzero(counts >= 0)[0]
    best = P.first_max(counts)
    lo, hi = P.score_brackets(hp[valid].astype(np.float32), X, pix, *S._cam(kw), kw['inlier_px'], S.DELTA, 1e-3)
    lo_best = lo[np.nonzero(valid == best)[0][0]]
    for j, k in enumerate(valid):
        if k != best and (hi[j] > lo_best or (hi[j] == lo_best and k < best)):
            return True
    return False


@pytest.mark.parametrize('mode', MODES)
def test_end_to_end_on_the_70_percent_outlier_set(mode):
    """The 40 frames of test_pnp_guided_host.py.  The device must select the reference's best hypothesis; where it does
    not, it must have counted at least as many inliers for its own pick as for the reference's (fp32 against fp64 at the
    threshold breaking a near tie), on at most 2 frames -- and first the reference must show, on the CPU, that no more
    than 2 frames have a runner-up whose scoring bracket reaches the winner's.  Poses of agreeing frames: the refinement
    bound of test_gpu_pnp_stages.py from the device's selected hypothesis, with d_perm measured on these frames (frames
    whose selected hypothesis has fewer than 16 inliers are out of that rule's scope, as there)."""
    recs, gts, out = HOST.solved(0.7)
    kw = _kw(mode, hypotheses=64)
    cam, thr = S._cam(kw), kw['inlier_px']
    ref_poses, ref_info = out[mode]
    ref_best, at_risk = [], 0
    for b in range(40):
        _, hp, counts, X, pix, _ = G.hypotheses_guided(recs[b], b, 64, mode)
        ref_best.append(P.first_max(counts))
        assert ref_best[-1] == ref_info[b, 3]
        at_risk += _runner_up_reaches_the_winner(hp, counts, X, pix, kw)
    assert at_risk <= 2, at_risk
    pr = GuidedProbe(recs, kw, t0=0)
    poses, info = pr.solve(10)
    assert (info[:, 0] == _lib.PNP_OK).all()
    S.check_selection(pr, info)                                           # the device's own counts, exactly
    differ = [b for b in range(40) if info[b, 3] != ref_best[b]]
    for b in differ:
        assert pr.counts[b, info[b, 3]] >= pr.counts[b, ref_best[b]], (b, info[b], ref_best[b])
    assert len(differ) <= 2, differ
    checked = 0
    for b in range(40):
        if b in differ or pr.counts[b, info[b, 3]] < 16:
            continue
        X, pix = pr.cands[b]
        R0, t0 = P.widen(pr.hp[b, info[b, 3]])
        d_perm = P.refine_permutation_spread(R0, t0, X, pix, *cam, thr, 10)
        ref = P.cam_to_world(*P.refine(R0, t0, X, pix, *cam, thr, 10))
        tol = 2.0 ** -23 * np.maximum(1.0, np.abs(ref)) + 10 * max(d_perm, S.D_PERM)
        assert (np.abs(poses[b].astype(np.float64) - ref) <= tol).all(), (b, np.abs(poses[b] - ref).max(), d_perm)
        checked += 1
    ok_dev = int(G.within_5cm_5deg(poses, gts).sum())
    ok_ref = int(G.within_5cm_5deg(ref_poses, gts).sum())
    ok_uni = int(G.within_5cm_5deg(pnp.PnPSolver(15, 20, **S._kw(hypotheses=64)).solve(recs)[0], gts).sum())
    print('mode %d: frames within 5 cm / 5 deg of 40: device %d, reference %d (device, uniform sampling: %d); best hypothesis '
          'differs on %s; %d poses checked against the refinement bound; %d frames at risk of a tie-break'
          % (mode, ok_dev, ok_ref, ok_uni, differ, checked, at_risk))
    assert checked >= 30, checked


# ---- programs ----------------------------------------------------------------------------------------------------------

def _run(args):
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, timeout=600)


def test_cli_sampling_flag(tmp_path):
    recs, gts = G.synthetic_frames_confidence(HOST.SEED, 5, 15, 20, 0.7)
    paths = []
    for i in range(5):
        paths.append(str(tmp_path / ('coord_%d.npy' % i)))
        np.save(paths[-1], recs[i])
    (tmp_path / 'coords.txt').write_text('\n'.join(paths) + '\n')
    outs = {}
    for name, flags in (('none', []), ('uniform', ['--sampling', 'uniform']), ('guided', ['--sampling', 'confidence2'])):
        r = _run(['-m', 'kfnet_amd.KFNet.pnp', str(tmp_path / 'coords.txt'), str(tmp_path / name), '--hypotheses', '64',
                  '--batch', '2'] + flags)
        assert r.returncode == 0, r.stdout
        outs[name] = ([open(str(tmp_path / name / ('pose_%d.txt' % i))).read() for i in range(5)],
                      r.stdout.replace(str(tmp_path / name), 'OUT'))
        assert sorted(os.listdir(str(tmp_path / name))) == sorted('pose_%d.txt' % i for i in range(5))
    assert outs['none'] == outs['uniform']                                # files and printed lines
    want, _ = pnp.PnPSolver(15, 20, hypotheses=64, sampling='confidence2').solve(recs)
    for i in range(5):
        got = pnp.read_pose(str(tmp_path / 'guided' / ('pose_%d.txt' % i)))
        assert np.array_equal(got.astype(np.float32), want[i], equal_nan=True), i
    assert outs['guided'][0] != outs['none'][0]


def test_eval_pose_sampling_flag(tmp_path):
    r = _run(['-m', 'kfnet_amd.KFNet.eval', '--scene', 'chess', '--synthetic', '8', '--random_weights', '--pose',
              '--pose_sampling', 'confidence', '--output_folder', str(tmp_path)])
    assert r.returncode == 0, r.stdout
    assert 'poses:' in r.stdout
    for i in range(8):
        rec = np.load(str(tmp_path / ('coord_%d.npy' % i)))
        T = pnp.read_pose(str(tmp_path / ('pose_%d.txt' % i)))
        want, info = pnp.PnPSolver(rec.shape[0], rec.shape[1], sampling='confidence').solve(rec[None], t0=i)
        if info[0, 0] == _lib.PNP_OK:
            assert np.array_equal(T.astype(np.float32), want[0]), i
        else:
            assert np.isnan(T).all(), i
