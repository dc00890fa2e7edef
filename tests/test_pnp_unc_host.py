"""CPU tests of the uncertainty-aware pose stage (no GPU): that the numpy restatement tests/pnp_unc_ref.py is worth
comparing a device against (weighting helps, the covariance is calibrated, the filter smooths and gates), the C surface
of kfn_pnp_ransac_unc and kfn_pose_filter with their argument checks, and the command lines' flag checks."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pnp_ref as P
import pnp_unc_ref as U
from kfnet_amd import _lib
from kfnet_amd.KFNet import pnp, pose_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the 200-frame sets of the issue: 9x13 grids, sigma log-uniform in 0.5-4 cm, 64 hypotheses
FRAMES, GRID, HYPS = 200, (9, 13), 64
CHI2_LO, CHI2_HI = 6.0 - 4.0 * np.sqrt(12.0 / FRAMES), 6.0 + 4.0 * np.sqrt(12.0 / FRAMES)   # 4 standard errors of a chi^2_6 mean

_CACHE = {}


def reference_solutions(outliers):
    """(ground truth, {weighted: (poses, cov, quality, info)}) of the 200-frame set, solved once per session."""
    if outliers not in _CACHE:
        recs, gt = U.synthetic_frames_sigma(7001 if outliers else 7002, FRAMES, GRID[0], GRID[1], outliers)
        hyps = []
        _CACHE[outliers] = (gt, {wt: U.ransac_unc(recs, wt, hypotheses_n=HYPS, hyps=hyps) for wt in (False, True)})
    return _CACHE[outliers]


def test_weighted_refinement_lowers_the_reference_pose_error():
    gt, sol = reference_solutions(0.2)
    err = {}
    for wt in (False, True):
        poses, _, _, info = sol[wt]
        assert (info[:, 0] == P.OK).all()
        err[wt] = pnp.pose_errors(poses, gt)
    med = {wt: (float(np.median(err[wt][0])), float(np.median(err[wt][1]))) for wt in err}
    better = float(np.mean(err[True][1] < err[False][1]))
    print('median rotation error %.4f -> %.4f deg, translation %.4f -> %.4f m (%.2fx), weighted better in %.1f %%'
          % (med[False][0], med[True][0], med[False][1], med[True][1], med[True][1] / med[False][1], 100 * better))
    assert med[True][0] < med[False][0] and med[True][1] < med[False][1], med
    assert better > 0.5, better


def test_reference_covariance_is_calibrated():
    gt, sol = reference_solutions(0.0)
    poses, cov, quality, info = sol[True]
    assert (info[:, 0] == P.OK).all() and np.isfinite(cov).all()
    d2 = U.mahalanobis2(poses, cov, gt)
    print('mean squared Mahalanobis distance %.3f (chi^2_6: 6; accepted %.2f .. %.2f)' % (d2.mean(), CHI2_LO, CHI2_HI))
    assert CHI2_LO < d2.mean() < CHI2_HI, d2.mean()
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))                  # built as L^-T L^-1: symmetric
    assert (quality[:, 1] == 2 * info[:, 2] - 6).all() and (quality[:, 0] > 0).all()


def test_covariance_is_the_inverse_of_a_numerical_hessian():
    """Sigma^-1 = sum J^T S^-1 J with J checked against central differences of the projection under the left
    perturbation: a wrong Jacobian column or weight would pass every self-consistency check above."""
    rng = np.random.default_rng(5)
    R, t = P.random_pose(rng)
    rec = P.synthetic_records(rng, 9, 13, R, t)
    X, pix = P.candidates(rec)
    sigma = np.exp(rng.uniform(np.log(0.005), np.log(0.04), X.shape[0]))
    cam = (525., 525., 320., 240.)
    Sg, cost, dof, n = U.covariance(R, t, X, pix, sigma, *cam, 10.0, 1.0)
    assert n == X.shape[0] and dof == 2 * n - 6 and cost < 1e-3           # exact records: float32 rounding only

    def project(d):
        dR = P.rodrigues(d[:3])
        Xc = X @ (dR @ R).T + (dR @ t + d[3:])
        return np.stack([525. * Xc[:, 0] / Xc[:, 2], 525. * Xc[:, 1] / Xc[:, 2]], 1)
    J = np.zeros((X.shape[0], 2, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = 1e-6
        J[:, :, k] = (project(d) - project(-d)) / 2e-6
    w00, w01, w11 = U.weights(R, t, X, sigma, 525., 525., 1.0)
    W = np.stack([np.stack([w00, w01], 1), np.stack([w01, w11], 1)], 1)
    H = np.einsum('nai,nab,nbj->ij', J, W, J)
    assert np.abs(Sg @ H - np.eye(6)).max() < 1e-5
    # S itself: sigma^2 A A^T + I against the propagated covariance of the point
    Xc = X @ R.T + t
    k = 3
    A = np.array([[525. / Xc[k, 2], 0, -525. * Xc[k, 0] / Xc[k, 2] ** 2], [0, 525. / Xc[k, 2], -525. * Xc[k, 1] / Xc[k, 2] ** 2]])
    assert np.allclose(np.linalg.inv(sigma[k] ** 2 * A @ A.T + np.eye(2)), W[k], rtol=1e-12)


def test_position_covariance_rotates_the_translation_block():
    rng = np.random.default_rng(6)
    R, t = P.random_pose(rng)
    T = P.cam_to_world(R, t)
    A = rng.normal(size=(6, 6))
    Sg = A @ A.T
    assert np.allclose(pose_filter.position_covariance(T, Sg), T[:3, :3] @ Sg[3:, 3:] @ T[:3, :3].T)
    assert pose_filter.position_covariance(np.stack([T, T]), np.stack([Sg, Sg])).shape == (2, 3, 3)


def test_reference_filter_smooths_gates_and_bridges():
    raw, smooth, good_total, good_rejected = [], [], 0, 0
    for seed in (8001, 8002, 8003):
        gt, meas, cov, kind = U.synthetic_trajectory(seed)
        out, _, flags, nis = U.pose_filter(meas, cov)
        good = kind == 0
        assert np.isin(flags[kind == 2], (U.REJECTED, U.INIT)).all(), (seed, flags[kind == 2])
        assert (flags[kind == 1] == U.MISSING).all() or kind[0] == 1
        assert np.isnan(nis[kind == 1]).all() and np.isfinite(nis[kind != 1][1:]).all()
        raw.append(np.linalg.norm(meas[good][:, :3, 3] - gt[good][:, :3, 3], axis=1))
        smooth.append(np.linalg.norm(out[good][:, :3, 3] - gt[good][:, :3, 3], axis=1))
        good_total += int(good.sum()) - 1
        good_rejected += int((flags[good][1:] != U.UPDATED).sum())
        bridged = np.linalg.norm(out[~good][:, :3, 3] - gt[~good][:, :3, 3], axis=1)
        print('seed %d: %d good, %d missing, %d wrong; worst bridged frame %.3f m' % (seed, good.sum(), (kind == 1).sum(),
                                                                                     (kind == 2).sum(), bridged.max()))
    raw, smooth = np.concatenate(raw), np.concatenate(smooth)
    print('median position error of the good frames %.4f -> %.4f m; %d of %d good measurements rejected'
          % (np.median(raw), np.median(smooth), good_rejected, good_total))
    assert np.median(smooth) < np.median(raw)
    assert good_rejected <= 0.02 * good_total, (good_rejected, good_total)


def test_reference_filter_flags_before_the_first_pose_and_at_a_reset():
    gt, meas, cov, kind = U.synthetic_trajectory(8004, T=40, missing=0.0, wrong=0.0, lead_missing=3)
    jump = np.eye(4)
    jump[:3, 3] = (0.6, -0.4, 0.5)
    meas[20:] = (jump @ meas[20:].astype(np.float64)).astype(np.float32)      # the scene moved: every later pose is "wrong"
    out, oc, flags, nis = U.pose_filter(meas, cov, max_rejects=3)
    assert list(flags[:4]) == [U.NONE] * 3 + [U.INIT] and np.isnan(out[:3]).all() and np.isnan(oc[:3]).all()
    assert (flags[4:20] == U.UPDATED).all()
    assert list(flags[20:24]) == [U.REJECTED, U.REJECTED, U.INIT, U.UPDATED], flags[20:24]
    assert np.isfinite(nis[20:23]).all() and (nis[20:23] > 22.46).all() and np.isnan(nis[:4]).all()
    assert np.array_equal(out[22], meas[22].astype(np.float64))


def _header():
    return open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()


def _struct_fields(hdr, name):
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for stmt in body.split(';'):
        stmt = stmt.strip()
        if stmt:
            typ, names = stmt.split(None, 1)
            fields += [(n.strip(), typ) for n in names.split(',')]
    return fields


def test_descriptors_match_the_header_and_the_abi_stays_13():
    hdr = _header()
    ctype = {'int32_t': C.c_int32, 'uint32_t': C.c_uint32, 'float': C.c_float}
    for name, cls in (('kfn_pnp_unc_desc', _lib.PnPUncDesc), ('kfn_pose_filter_desc', _lib.PoseFilterDesc)):
        fields = _struct_fields(hdr, name)
        assert [(n, ctype[t]) for n, t in fields] == list(cls._fields_), name
        assert fields[0][0] == 'struct_size' and cls().struct_size == C.sizeof(cls) == 4 * len(fields)
    assert len(_struct_fields(hdr, 'kfn_pnp_desc')) == len(_lib.PnPDesc._fields_) == 17        # no field added
    for i, name in enumerate(('UPDATED', 'MISSING', 'REJECTED', 'INIT', 'NONE')):
        assert re.search(r'#define KFN_POSE_%s (\d+)' % name, hdr).group(1) == str(i) == str(getattr(_lib, 'POSE_' + name))
    assert (U.UPDATED, U.MISSING, U.REJECTED, U.INIT, U.NONE) == (0, 1, 2, 3, 4)
    lib = _lib.load()
    assert lib.kfn_abi_version() == 13 == _lib.ABI_VERSION and '#define KFN_ABI_VERSION 13' in hdr
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ('kfn_pnp_ransac_unc', 'kfn_pose_filter'):
        assert re.search(r'\bint %s\(' % name, hdr) and name in _lib.SYMBOLS and hasattr(lib, name) and name in doc, name


def test_new_entry_points_validate_arguments_without_a_gpu():
    lib = _lib.load()
    dummy = C.c_void_p(16)          # never dereferenced: every call below fails its checks first
    d = pnp.PnPSolver(60, 80).desc(2)

    def unc(desc=d, q=None, null=None, **kw):
        q = q if q is not None else _lib.PnPUncDesc(weighted=1, pixel_sigma=1.0)
        for k, v in kw.items():
            setattr(q, k, v)
        args = [dummy] * 7
        if null is not None:
            args[null] = None
        return lib.kfn_pnp_ransac_unc(C.byref(desc) if desc is not None else None, C.byref(q) if q is not False else None,
                                      args[0], args[1], args[2], args[3], args[4], args[5], None)
    assert unc(desc=None) == -1
    assert unc(q=False) == -1 and b'null' in lib.kfn_last_error()
    for kw in (dict(struct_size=8), dict(struct_size=0), dict(struct_size=14), dict(pixel_sigma=0.0),
               dict(pixel_sigma=-1.0), dict(pixel_sigma=float('nan')), dict(weighted=2)):
        assert unc(**kw) == -1, kw
    assert unc(pixel_sigma=0.0) == -1 and b'pixel_sigma' in lib.kfn_last_error()
    bad = pnp.PnPSolver(60, 80).desc(2)
    bad.hypotheses = 0
    assert unc(desc=bad) == -1
    neg = pnp.PnPSolver(60, 80, min_confidence=-1.0).desc(2)
    assert unc(desc=neg) == -1 and b'min_confidence' in lib.kfn_last_error()
    for null in (0, 1, 4, 5):                     # records, poses, info, scratch; cov (2) and quality (3) may be null
        assert unc(null=null) == -1, null
    assert lib.kfn_pnp_ransac_unc(C.byref(d), C.byref(_lib.PnPUncDesc(pixel_sigma=1.0)), dummy, dummy, dummy, dummy, dummy,
                                  C.c_void_p(20), None) == -1 and b'aligned' in lib.kfn_last_error()
    with pytest.raises(ValueError):
        pnp.PnPSolver(60, 80, pixel_sigma=0.0)

    def filt(desc=None, null=None, **kw):
        q = pose_filter.PoseFilter().desc(2, 8)
        for k, v in kw.items():
            setattr(q, k, v)
        args = [dummy] * 6
        if null is not None:
            args[null] = None
        return lib.kfn_pose_filter(C.byref(q) if desc is None else desc, *args, None)
    assert lib.kfn_pose_filter(None, dummy, dummy, dummy, dummy, dummy, dummy, None) == -1
    for kw in (dict(struct_size=8), dict(struct_size=0), dict(S=0), dict(T=0), dict(S=-1), dict(S=-2, T=-3),
               dict(max_rejects=0), dict(max_rejects=-1), dict(gate=0.0), dict(rot_sigma=-0.1), dict(trans_sigma=float('nan'))):
        assert filt(**kw) == -1, kw
    assert filt(max_rejects=0) == -1 and b'max_rejects' in lib.kfn_last_error()
    for null in range(6):
        assert filt(null=null) == -1, null
    for kw in (dict(max_rejects=0), dict(gate=0.0), dict(rot_sigma=-1.0)):
        with pytest.raises(ValueError):
            pose_filter.PoseFilter(**kw)


def _run(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    e['PYTHONPATH'] = ROOT + os.pathsep + e.get('PYTHONPATH', '')
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, timeout=300)


def test_command_lines_refuse_bad_flag_combinations_before_a_device_is_touched(tmp_path):
    lst = tmp_path / 'list.txt'
    lst.write_text(str(tmp_path / 'missing_coord_0.npy') + '\n')      # never read: the flags are checked first
    out = tmp_path / 'out'
    for flags, word in ((['--pixel_sigma', '0'], '--pixel_sigma'),
                        (['--smooth', '--max_rejects', '0'], '--max_rejects'),
                        (['--smooth', '--gate', '0'], '--gate'),
                        (['--smooth', '--rot_sigma', '-1'], '--rot_sigma'),
                        (['--smooth', '--sequence_length', '-2'], '--sequence_length'),
                        (['--gate', '10'], '--smooth'),
                        (['--sequence_length', '5'], '--smooth')):
        r = _run(['-m', 'kfnet_amd.KFNet.pnp', str(lst), str(out)] + flags)
        assert r.returncode == 2 and word in r.stdout, (flags, r.stdout)
        assert not out.exists()
    r = _run(['-m', 'kfnet_amd.KFNet.pnp', '--help'])
    assert r.returncode == 0
    for flag in ('--weighted', '--pixel_sigma', '--covariance', '--smooth', '--rot_sigma', '--trans_sigma', '--gate',
                 '--max_rejects', '--sequence_length'):
        assert flag in r.stdout, flag
    for prog in ('kfnet_amd.KFNet.eval', 'kfnet_amd.SCoordNet.eval'):
        r = _run(['-m', prog, '--help'])
        assert r.returncode == 0 and '--pose_weighted' in r.stdout, prog
