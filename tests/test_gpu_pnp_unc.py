"""kfn_pnp_ransac_unc and kfn_pose_filter against the fp64 restatement tests/pnp_unc_ref.py (DESIGN.md 5c "Uncertainty").

As in tests/test_gpu_pnp_stages.py every reference starts from the device's own output of the stage before: the probe's
fp32 [R|t] of the selected hypothesis widened to double, exactly as the refinement kernels read it.

  unweighted   weighted = 0: poses and info are kfn_pnp_ransac's bits; every output repeats bit for bit.
  weighted     pose against pnp_unc_ref.refine_weighted: per entry 2**-23 * max(1, |ref|) (the fp32 rounding of the
               output) + 10 * D_PERM; info[:,2] equals the reference's inlier count.
  covariance   cov per entry in units of sqrt(Sigma_ii Sigma_jj), the cost relative to itself, against the reference at
               the reference's final pose: 2**-23 + 10 * (D_PERM_COV + D_ROUND); 2 * inliers - 6 exactly; symmetric to the
               last bit; NaN exactly where there is no pose.
  value        on the 200-frame sets of tests/test_pnp_unc_host.py solved on the device: weighting lowers both median
               errors, and the true error's mean squared Mahalanobis distance is a chi^2_6 mean within 4 standard errors.
  filter       flags exactly, poses / covariances / NIS within 2**-23 * max(1, |ref|) + 10 * D_SOLVE.

Conditions that keep a check from being vacuous are asserted (reference movement above 1e-3, >= 16 inliers of the
selected hypothesis, an empty band at the inlier threshold and at the NIS gate, every flag value present)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pnp_ref as P
import pnp_unc_ref as U
from kfnet_amd import _lib
from kfnet_amd.KFNet import pnp
from kfnet_amd.KFNet.pose_filter import PoseFilter

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The reference's own sensitivity, measured on the CPU on every frame of every set below, from pnp_ref.hypotheses' selected
# pose (rounded to fp32), refine_iters 0, 1, 3 and 10 (DESIGN.md 5c "Uncertainty"):
#   D_PERM       largest change of an entry of the weighted refinement's camera-to-world pose over five permutations of
#                the candidate list: 0 at refine_iters 0, up to 4.1e-14 at 1 and 3, up to 3.11e-9 (9x13, frame 7) at 10,
#                where the loop has converged and the last accept/reject decision hangs on the last bits of two costs
#   D_PERM_COV   the same for an entry of Sigma in units of sqrt(Sigma_ii Sigma_jj) and for the relative cost: up to
#                2.5e-13 before convergence, 4.86e-9 (the same frame) at refine_iters 10
#   D_ROUND      largest change of such an entry of Sigma / of the relative cost when the final pose of refine_iters 10
#                (what the covariance test runs) is rounded to fp32 and back: up to 7.55e-7 after the weighted
#                refinement, 3.22e-6 (9x13, frame 1) after the unweighted one, whose final pose is not the minimum of the
#                weighted cost, so that the cost changes to first order in the rounding
D_PERM = 3.11e-9
D_PERM_COV = 4.86e-9
D_ROUND = 3.22e-6
# The filter reference's own largest difference between solving with S by Cholesky (as the device) and by LU
# (numpy.linalg.solve), over every output of the three sequences below (poses, covariances, NIS); the flags agree.
D_SOLVE = 3.41e-13
BAND = 1e-6          # no candidate's final error within this relative distance of inlier_px, no NIS of the gate (asserted)

DEFAULTS = dict(fx=525., fy=525., u=320., v=240., hypotheses=256, min_points=16, seed=0, min_confidence=20.,
                inlier_px=10., cell_stride=8)
FILTER = dict(rot_sigma=0.02, trans_sigma=0.02, gate=22.46, max_rejects=3)


def _kw(**kw):
    full = dict(DEFAULTS)
    full.update(kw)
    return full


def _cam(kw):
    return kw['fx'], kw['fy'], kw['u'], kw['v']


def _set(seed, B, h, w, outliers, ld=4, **cam):
    kw = _kw(**cam)
    recs, gt = U.synthetic_frames_sigma(seed, B, h, w, outliers, fx=kw['fx'], fy=kw['fy'], u=kw['u'], v=kw['v'])
    if ld > 4:
        wide = np.full(recs.shape[:3] + (ld,), np.nan, np.float32)       # the extra channels must not be read
        wide[..., :4] = recs
        recs = wide
    return recs, gt, kw


FRAME_SETS = {
    '9x13': lambda: _set(9101, 8, 9, 13, 0.2),                                     # h*w below one pass of 256 threads
    '15x20_ld7': lambda: _set(9102, 4, 15, 20, 0.3, ld=7),
    '37x53_fx_ne_fy': lambda: _set(9103, 4, 37, 53, 0.3, fx=500., fy=560., u=300.5, v=250.25),   # 1961 cells: 8 passes
}


class Probe(object):
    """One frame set on the device: the probe's hypotheses and counts, and the reference's candidate lists."""

    def __init__(self, recs, gt, kw):
        self.recs, self.gt, self.kw = recs, gt, kw
        self.h, self.w = recs.shape[1:3]
        _, self.hp, self.counts = pnp.PnPSolver(self.h, self.w, **kw).hypotheses_probe(recs)
        self.cands = [P.candidates(r[..., :4], kw['min_confidence'], kw['cell_stride']) for r in recs]
        self.sigma = [U.candidate_sigma(r[..., :4], kw['min_confidence']) for r in recs]

    def solver(self, refine_iters, weighted):
        return pnp.PnPSolver(self.h, self.w, refine_iters=refine_iters, weighted=weighted, **self.kw)

    def start(self, b):
        k = P.first_max(self.counts[b])
        assert self.counts[b, k] >= 16, (b, k, self.counts[b, k])
        return (k,) + P.widen(self.hp[b, k])


_PROBES = {}


def _probe(name):
    if name not in _PROBES:
        _PROBES[name] = Probe(*FRAME_SETS[name]())
    return _PROBES[name]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ---- 1. weighted = 0 and repeatability ------------------------------------------------------------------------------------

@pytest.mark.parametrize('frames', sorted(FRAME_SETS))
def test_unweighted_is_kfn_pnp_ransac_bit_for_bit_and_both_modes_repeat(frames):
    pr = _probe(frames)
    for iters in (0, 3, 10):
        poses, info = pr.solver(iters, False).solve(pr.recs)
        p0, c0, q0, i0 = pr.solver(iters, False).solve_unc(pr.recs)
        assert (info[:, 0] == _lib.PNP_OK).all()
        assert np.array_equal(_bits(p0), _bits(poses)) and np.array_equal(i0, info), iters
    for weighted in (False, True):
        a = pr.solver(10, weighted).solve_unc(pr.recs)
        b = pr.solver(10, weighted).solve_unc(pr.recs)
        for x, y in zip(a, b):
            assert np.array_equal(_bits(x), _bits(y)), weighted
    # a frame's result does not depend on the batch it is solved in
    one = pr.solver(10, True).solve_unc(pr.recs[1:2], t0=1)
    for x, y in zip(a, one):
        assert np.array_equal(_bits(x[1:2]), _bits(y))


# ---- 2. the weighted pose -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('refine_iters', [0, 1, 3, 10])
@pytest.mark.parametrize('frames', sorted(FRAME_SETS))
def test_weighted_pose_matches_the_fp64_restatement(frames, refine_iters):
    pr = _probe(frames)
    kw = pr.kw
    cam, thr = _cam(kw), kw['inlier_px']
    poses, cov, quality, info = pr.solver(refine_iters, True).solve_unc(pr.recs)
    assert (info[:, 0] == _lib.PNP_OK).all(), info
    moved = []
    for b in range(pr.recs.shape[0]):
        X, pix = pr.cands[b]
        k, R0, t0 = pr.start(b)
        assert info[b, 3] == k and info[b, 1] == X.shape[0]
        R, t = U.refine_weighted(R0, t0, X, pix, pr.sigma[b], *cam, thr, refine_iters)
        ref = P.cam_to_world(R, t)
        got = poses[b].astype(np.float64)
        margin = P.threshold_margin(R, t, X, pix, *cam, thr)
        inl = int(P.inliers(R, t, X, pix, *cam, thr).sum())
        moved.append(float(np.abs(ref - P.cam_to_world(R0, t0)).max()))
        print('frame %d: iters %d, max |device - ref| %.3g, ref moved %.3g, threshold margin %.3g, inliers %d / %d'
              % (b, refine_iters, np.abs(got - ref).max(), moved[-1], margin, info[b, 2], inl))
        assert margin > BAND, (b, margin)
        tol = 2.0 ** -23 * np.maximum(1.0, np.abs(ref)) + 10 * D_PERM
        assert (np.abs(got - ref) <= tol).all(), (b, refine_iters, np.abs(got - ref).max(), got, ref)
        assert info[b, 2] == inl, (b, info[b], inl)
    if refine_iters >= 3:
        assert min(moved) > 1e-3, moved           # else agreeing with the reference proves nothing


# ---- 3. covariance and quality --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('frames', sorted(FRAME_SETS))
def test_covariance_and_quality_match_the_fp64_restatement(frames, weighted):
    pr = _probe(frames)
    kw = pr.kw
    cam, thr = _cam(kw), kw['inlier_px']
    poses, cov, quality, info = pr.solver(10, weighted).solve_unc(pr.recs)
    assert (info[:, 0] == _lib.PNP_OK).all() and np.isfinite(cov).all() and np.isfinite(quality).all()
    # Sigma = L^-T L^-1: the kernel computes the upper triangle and mirrors it, so symmetry is exact, not within an ulp
    assert np.array_equal(_bits(cov), _bits(np.swapaxes(cov, 1, 2)))
    tol = 2.0 ** -23 + 10 * (D_PERM_COV + D_ROUND)
    for b in range(pr.recs.shape[0]):
        X, pix = pr.cands[b]
        _, R0, t0 = pr.start(b)
        if weighted:
            R, t = U.refine_weighted(R0, t0, X, pix, pr.sigma[b], *cam, thr, 10)
        else:
            R, t = P.refine(R0, t0, X, pix, *cam, thr, 10)
        assert P.threshold_margin(R, t, X, pix, *cam, thr) > BAND
        Sg, cost, dof, n = U.covariance(R, t, X, pix, pr.sigma[b], *cam, thr)
        nrm = np.sqrt(np.outer(np.diag(Sg), np.diag(Sg)))
        err = np.abs(cov[b].astype(np.float64) - Sg) / nrm
        print('frame %d: weighted %d, max normalised |cov - ref| %.3g, cost %.6g vs %.6g, dof %g'
              % (b, weighted, err.max(), quality[b, 0], cost, dof))
        assert (err <= tol).all(), (b, err.max(), tol)
        assert abs(float(quality[b, 0]) - cost) <= tol * cost, (b, quality[b, 0], cost)
        assert quality[b, 1] == dof == 2 * info[b, 2] - 6 and info[b, 2] == n
        assert (np.diag(cov[b]) > 0).all()


def test_nan_exactly_where_there_is_no_pose_and_null_outputs():
    import ctypes as C
    import torch
    recs, _, kw = _set(9104, 4, 9, 13, 0.2)
    recs[1, ..., 3] = 5.0                          # below min_confidence: too few points
    recs[3, ..., :3] = (0.25, -0.5, 2.0)           # one scene point everywhere: no P3P solution
    solver = pnp.PnPSolver(9, 13, weighted=True, **kw)
    poses, cov, quality, info = solver.solve_unc(recs)
    assert list(info[:, 0]) == [_lib.PNP_OK, _lib.PNP_TOO_FEW_POINTS, _lib.PNP_OK, _lib.PNP_NO_HYPOTHESIS], info
    for b in range(4):
        ok = info[b, 0] == _lib.PNP_OK
        for x in (poses[b], cov[b], quality[b]):
            assert np.isfinite(x).all() if ok else np.isnan(x).all(), (b, x)
    # cov and quality may be null: the same poses and info
    lib = _lib.load()
    rec = torch.from_numpy(recs).cuda()
    d, q = solver.desc(4), _lib.PnPUncDesc(weighted=1, pixel_sigma=1.0)
    nb = C.c_size_t()
    _lib.check(lib.kfn_pnp_scratch_bytes(C.byref(d), C.byref(nb)))
    scratch = torch.empty(nb.value, dtype=torch.uint8, device='cuda')
    p2 = torch.empty((4, 4, 4), dtype=torch.float32, device='cuda')
    i2 = torch.empty((4, 4), dtype=torch.int32, device='cuda')
    _lib.check(lib.kfn_pnp_ransac_unc(C.byref(d), C.byref(q), rec.data_ptr(), p2.data_ptr(), None, None, i2.data_ptr(),
                                      scratch.data_ptr(), torch.cuda.current_stream().cuda_stream), 'kfn_pnp_ransac_unc')
    assert np.array_equal(_bits(p2.cpu().numpy()), _bits(poses)) and np.array_equal(i2.cpu().numpy(), info)


# ---- 4. value on the device -----------------------------------------------------------------------------------------------

def test_weighting_helps_and_the_covariance_is_calibrated_on_the_device():
    import test_pnp_unc_host as H
    recs, gt = U.synthetic_frames_sigma(7001, H.FRAMES, H.GRID[0], H.GRID[1], 0.2)
    med = {}
    for weighted in (False, True):
        solver = pnp.PnPSolver(H.GRID[0], H.GRID[1], hypotheses=H.HYPS, weighted=weighted)
        poses, _, _, info = pnp.solve_unc_in_batches(solver, recs)
        assert (info[:, 0] == _lib.PNP_OK).all()
        rot, trans = pnp.pose_errors(poses, gt)
        med[weighted] = (float(np.median(rot)), float(np.median(trans)))
    print('median rotation error %.4f -> %.4f deg, translation %.4f -> %.4f m'
          % (med[False][0], med[True][0], med[False][1], med[True][1]))
    assert med[True][0] < med[False][0] and med[True][1] < med[False][1], med
    recs, gt = U.synthetic_frames_sigma(7002, H.FRAMES, H.GRID[0], H.GRID[1], 0.0)
    solver = pnp.PnPSolver(H.GRID[0], H.GRID[1], hypotheses=H.HYPS, weighted=True)
    poses, cov, _, info = pnp.solve_unc_in_batches(solver, recs)
    assert (info[:, 0] == _lib.PNP_OK).all() and np.isfinite(cov).all()
    d2 = U.mahalanobis2(poses, cov, gt)
    print('mean squared Mahalanobis distance %.3f (accepted %.2f .. %.2f)' % (d2.mean(), H.CHI2_LO, H.CHI2_HI))
    assert H.CHI2_LO < d2.mean() < H.CHI2_HI, d2.mean()


# ---- 5. the pose filter ---------------------------------------------------------------------------------------------------

def filter_sequences():
    """(poses [3,64,4,4], cov [3,64,6,6]) float32: missing frames and wrong poses; a start on missing frames; a scene
    change that forces a re-initialisation (and a NaN covariance, which counts as missing)."""
    seqs = [U.synthetic_trajectory(9201, T=64, missing=0.1, wrong=0.08),
            U.synthetic_trajectory(9202, T=64, missing=0.1, wrong=0.05, lead_missing=4),
            U.synthetic_trajectory(9203, T=64, missing=0.05, wrong=0.0)]
    poses = np.stack([s[1] for s in seqs])
    cov = np.stack([s[2] for s in seqs])
    jump = np.eye(4)
    jump[:3, 3] = (0.6, -0.4, 0.5)
    poses[2, 30:] = (jump @ poses[2, 30:].astype(np.float64)).astype(np.float32)
    cov[2, 10, 2, 3] = np.nan
    return poses, cov


def test_pose_filter_matches_the_fp64_restatement():
    poses, cov = filter_sequences()
    out_p, out_c, flags, nis = PoseFilter(**FILTER).run(poses, cov)
    assert out_p.shape == poses.shape and out_c.shape == cov.shape and flags.shape == nis.shape == (3, 64)
    seen = set()
    for s in range(3):
        rp, rc, rf, rn = U.pose_filter(poses[s], cov[s], **FILTER)
        tested = np.isfinite(rn)
        assert (np.abs(rn[tested] / float(np.float32(FILTER['gate'])) - 1.0) > BAND).all()
        assert np.array_equal(flags[s], rf), (s, flags[s], rf)
        seen |= set(int(f) for f in rf)
        for got, ref, what in ((out_p[s], rp, 'poses'), (out_c[s], rc, 'cov'), (nis[s], rn, 'nis')):
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (s, what)
            m = np.isfinite(ref)
            err = np.abs(got.astype(np.float64)[m] - ref[m])
            tol = 2.0 ** -23 * np.maximum(1.0, np.abs(ref[m])) + 10 * D_SOLVE
            print('sequence %d %s: max |device - ref| %.3g' % (s, what, err.max()))
            assert (err <= tol).all(), (s, what, err.max())
        assert np.array_equal(_bits(out_c[s]), _bits(np.swapaxes(out_c[s], 1, 2)))
    assert seen == {U.UPDATED, U.MISSING, U.REJECTED, U.INIT, U.NONE}, seen
    assert flags[1, 0] == U.NONE and flags[2, 10] == U.MISSING and (flags[2, 30:33] == (U.REJECTED, U.REJECTED, U.INIT)).all()
    # [T,...] input is one sequence; a sequence does not depend on its neighbours
    one = PoseFilter(**FILTER).run(poses[1], cov[1])
    for x, y in zip(one, (out_p[1], out_c[1], flags[1], nis[1])):
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y))


# ---- 6. the command lines -------------------------------------------------------------------------------------------------

def _run(args):
    e = dict(os.environ)
    e['PYTHONPATH'] = ROOT + os.pathsep + e.get('PYTHONPATH', '')
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, timeout=300)


def test_pnp_command_line_writes_covariances_and_smoothed_poses(tmp_path):
    recs, gt = U.synthetic_frames_sigma(9301, 6, 15, 20, 0.2)
    coords, gts = [], []
    for i in range(6):
        coords.append(str(tmp_path / ('coord_%d.npy' % i)))
        np.save(coords[-1], recs[i])
        gts.append(str(tmp_path / ('gt_%d.txt' % i)))
        pnp.write_pose(gts[-1], gt[i])
    (tmp_path / 'coords.txt').write_text('\n'.join(coords) + '\n')
    (tmp_path / 'gt.txt').write_text('\n'.join(gts) + '\n')
    out = tmp_path / 'out'
    r = _run(['-m', 'kfnet_amd.KFNet.pnp', str(tmp_path / 'coords.txt'), str(out), '--gt', str(tmp_path / 'gt.txt'),
              '--weighted', '--covariance', '--smooth', '--sequence_length', '4', '--batch', '4'])
    assert r.returncode == 0, r.stdout
    assert r.stdout.count('median rotation error') == 2 and 'smoothed frame 5:' in r.stdout, r.stdout
    poses, cov, _, info = pnp.PnPSolver(15, 20, weighted=True).solve_unc(recs)
    assert (info[:, 0] == _lib.PNP_OK).all()
    filt = PoseFilter()
    smooth = np.concatenate([filt.run(poses[:4], cov[:4])[0], filt.run(poses[4:], cov[4:])[0]])
    for i in range(6):
        assert np.array_equal(pnp.read_pose(str(out / ('pose_%d.txt' % i))).astype(np.float32), poses[i]), i
        assert np.array_equal(pnp.read_covariance(str(out / ('pose_cov_%d.txt' % i))).astype(np.float32), cov[i]), i
        assert np.array_equal(pnp.read_pose(str(out / ('pose_smooth_%d.txt' % i))).astype(np.float32), smooth[i]), i


def test_eval_pose_weighted_writes_the_weighted_poses_and_covariances(tmp_path):
    r = _run(['-m', 'kfnet_amd.SCoordNet.eval', '--scene', 'chess', '--synthetic', '3', '--random_weights',
              '--pose_weighted', '--height', '64', '--width', '96', '--output_folder', str(tmp_path)])
    assert r.returncode == 0, r.stdout
    assert 'poses:' in r.stdout
    for i in range(3):
        rec = np.load(str(tmp_path / ('coord_%d.npy' % i)))
        assert rec.shape == (8, 12, 4)
        poses, cov, _, _ = pnp.PnPSolver(8, 12, weighted=True).solve_unc(rec[None], t0=i)
        assert np.array_equal(pnp.read_pose(str(tmp_path / ('pose_%d.txt' % i))).astype(np.float32), poses[0], equal_nan=True)
        assert np.array_equal(pnp.read_covariance(str(tmp_path / ('pose_cov_%d.txt' % i))).astype(np.float32), cov[0],
                              equal_nan=True)
