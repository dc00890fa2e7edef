"""RANSAC-Kabsch without a device: the fp64 restatement tests/kabsch_ref.py on its own, the accuracy study against
pnp_ref on the same frames, the calibration of the covariance, the CPU-side measurements that tests/test_gpu_kabsch.py's
tolerances are built from, the command line's refusals and the new exports' argument checks (DESIGN.md 5c "Poses with
depth")."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kabsch_ref as K
import pnp_ref as P
import pnp_unc_ref as U
from kfnet_amd import _lib, build
from kfnet_amd.KFNet import kabsch, pnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = (K.kabsch_horn, K.kabsch_svd)

# the 200-frame sets of DESIGN.md 5c "What the reference shows": 9x13 grids, sigma log-uniform in 0.5-4 cm, 64 hypotheses
FRAMES, GRID, HYPS = 200, (9, 13), 64
CHI2_LO, CHI2_HI = 6.0 - 4.0 * np.sqrt(12.0 / FRAMES), 6.0 + 4.0 * np.sqrt(12.0 / FRAMES)


# ---- hand cases -----------------------------------------------------------------------------------------------------------

def test_reference_recovers_a_known_pose_from_noise_free_points():
    rng = np.random.default_rng(11)
    for n in (3, 4, 50):
        R, t = P.random_pose(rng)
        Pc = rng.uniform(-2, 2, (n, 3))
        X = Pc @ R.T + t
        w = rng.uniform(0.5, 2.0, n)
        for form in FORMS:
            for ww in (None, w):
                Rr, tr = form(Pc, X, ww)
                assert np.abs(Rr - R).max() < 1e-12 and np.abs(tr - t).max() < 1e-12, (form.__name__, n)
        ev, V = K.jacobi_eigh4(K.horn_matrix(K.moments(Pc, X, w)[3]))       # the device's eigen-solver, restated
        assert np.abs(np.sort(ev) - np.linalg.eigvalsh(K.horn_matrix(K.moments(Pc, X, w)[3]))).max() < 1e-12 * np.abs(ev).max()
        assert np.abs(K.quaternion_matrix(V[:, np.argmax(ev)]) - R).max() < 1e-12


def test_reflection_prone_planar_set_still_gives_a_proper_rotation():
    """Nearly planar camera points whose scene points are their mirror image: the best orthogonal map is a reflection with
    zero residual; the answer must be the best rotation, det +1, in both forms."""
    rng = np.random.default_rng(12)
    R, t = P.random_pose(rng)
    eps = 1e-3
    Pc = np.concatenate([rng.uniform(-1, 1, (12, 2)), eps * rng.uniform(-1, 1, (12, 1))], axis=1)
    X = (Pc * [1.0, 1.0, -1.0]) @ R.T + t
    sols = [form(Pc, X) for form in FORMS]
    for Rr, tr in sols:
        assert abs(np.linalg.det(Rr) - 1.0) < 1e-12 and np.abs(Rr @ Rr.T - np.eye(3)).max() < 1e-12
        assert np.sqrt(K.dist2(Rr, tr, Pc, X)).max() <= 2.0 * eps          # the mirror image is 2 eps away at most
        assert np.abs(Rr - R).max() < 2.0 * eps        # the planted rotation, tilted by at most the relief over unit arms
    assert np.abs(sols[0][0] - sols[1][0]).max() < 1e-9
    # exactly planar and exactly mirrored: rotation and reflection tie; still det +1
    Pc[:, 2] = 0.0
    for form in FORMS:
        Rr, _ = form(Pc, Pc @ R.T + t)
        assert abs(np.linalg.det(Rr) - 1.0) < 1e-12 and np.abs(Rr - R).max() < 1e-9


def test_collinear_triples_are_invalid():
    rng = np.random.default_rng(13)
    R, t = P.random_pose(rng)
    line = np.outer([0.0, 0.5, 2.0, -1.0, 3.0], [1.0, 2.0, -1.0]) + [0.3, 0.1, 2.0]
    free = rng.uniform(-2, 2, (5, 3))
    for form in FORMS:
        assert K.hypothesis(line, line @ R.T + t, [0, 1, 2], form) is None         # both triangles on a line
        assert K.hypothesis(line, free, [0, 1, 2], form) is None                   # the camera triangle alone
        assert K.hypothesis(free, line, [0, 1, 2], form) is None                   # the scene triangle alone
        assert K.hypothesis(free, free @ R.T + t, [0, 1, 2], form) is not None
        assert form(line, line @ R.T + t) is None                                  # five points of a line: the gap rule
        assert form(line[:2], (line @ R.T + t)[:2]) is None
    assert K.cross_norm(line[:3]) < K.MIN_CROSS < K.cross_norm(free[:3])


# ---- the sampler ----------------------------------------------------------------------------------------------------------

def test_samples_are_pnp_refs_first_three_distinct_draws():
    both = short = 0
    for seed, frame in ((0, 0), (7, 3), (0xFFFFFFFF, 1000)):
        for n in (3, 4, 5, 16, 117):
            for hyp in range(64):
                distinct = []
                for draw in range(P.MAX_DRAWS):
                    k = (P.sample_hash(seed, frame, hyp, draw) * n) >> 32
                    if k not in distinct:
                        distinct.append(k)
                s3, s4 = K.draw_sample(seed, frame, hyp, n), P.draw_sample(seed, frame, hyp, n)
                assert s3 == (distinct[:3] if len(distinct) >= 3 else None)
                if s4 is not None:
                    assert s3 == s4[:3]
                    both += 1
                else:
                    short += 1
    assert both and short


# ---- the accuracy study ---------------------------------------------------------------------------------------------------

def test_weighted_kabsch_is_no_worse_than_pnp_on_the_same_frames():
    """200 9x13 frames, sigma log-uniform 0.5-4 cm, noise drawn from sigma, 64 hypotheses, 5 mm depth noise; the reference
    alone.  Nothing here says anything about real maps."""
    for outliers in (0.2, 0.5):
        recs, cams, gt = K.synthetic_frames_depth(7001, FRAMES, GRID[0], GRID[1], outliers)
        same, same_gt = U.synthetic_frames_sigma(7001, FRAMES, GRID[0], GRID[1], outliers)
        assert np.array_equal(recs, same) and np.array_equal(gt, same_gt)          # pnp_ref sees the same frames
        med = {}
        hyps = []
        for wt in (False, True):
            poses, _, _, info = K.ransac(recs, cams, wt, hypotheses_n=HYPS, hyps=hyps)
            assert (info[:, 0] == K.OK).all()
            rot, trans = pnp.pose_errors(poses, gt)
            med['kabsch weighted' if wt else 'kabsch'] = (float(np.median(rot)), float(np.median(trans)))
            assert (trans < 0.05).all()
        with np.errstate(all='ignore'):
            poses, info = P.ransac(recs, hypotheses_n=HYPS)
        assert (info[:, 0] == P.OK).all()
        rot, trans = pnp.pose_errors(poses, gt)
        med['pnp_ref'] = (float(np.median(rot)), float(np.median(trans)))
        for name in ('kabsch', 'kabsch weighted', 'pnp_ref'):
            print('%2.0f %% outliers, %-15s median rotation error %.4f deg, median translation error %.4f cm'
                  % (100 * outliers, name, med[name][0], 100 * med[name][1]))
        assert med['kabsch weighted'][1] <= med['pnp_ref'][1], med


# ---- the covariance -------------------------------------------------------------------------------------------------------

def test_reference_covariance_is_calibrated():
    """No outliers; the camera points carry the noise the model states (isotropic, point_sigma = 1 cm), the records their
    own sigma; weighted refinement, the default inlier_m.  (With 5 mm of noise in depth alone the floor overstates the noise
    and the mean is about 3: the covariance is then conservative.)"""
    recs, cams, gt = K.synthetic_frames_depth(7002, FRAMES, GRID[0], GRID[1], 0.0, depth_noise=0.0, point_noise=0.01)
    poses, cov, quality, info = K.ransac(recs, cams, True, hypotheses_n=HYPS, point_sigma=0.01)
    assert (info[:, 0] == K.OK).all() and np.isfinite(cov).all()
    d2 = U.mahalanobis2(poses, cov, gt)
    print('mean squared Mahalanobis distance %.3f (chi^2_6: 6; accepted %.2f .. %.2f)' % (d2.mean(), CHI2_LO, CHI2_HI))
    assert CHI2_LO < d2.mean() < CHI2_HI, d2.mean()
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))
    assert (quality[:, 1] == 3 * info[:, 2] - 6).all() and (quality[:, 0] > 0).all()


def test_covariance_is_the_inverse_of_a_numerical_hessian():
    """With exact points the cost sum w |exp(omega) q + tau - p|^2 has the Hessian 2 sum w J^T J at its minimum: central
    differences under the left perturbation of the world-to-camera pose catch a wrong sign or column of J."""
    rng = np.random.default_rng(14)
    R, t = P.random_pose(rng)
    Pc = rng.uniform(-2, 2, (40, 3)) + [0.0, 0.0, 3.0]
    X = Pc @ R.T + t
    sig2 = rng.uniform(0.005, 0.04, 40) ** 2
    Sg, cost, dof, n = K.covariance(R, t, Pc, X, sig2, 0.10)
    assert n == 40 and dof == 114.0 and cost < 1e-20
    w = 1.0 / (sig2 + K.f32(0.01) ** 2)
    Rw, tw = R.T, -R.T @ t

    def cost_at(d):
        E = P.rodrigues(d[:3])
        q = X @ (E @ Rw).T + (E @ tw + d[3:])
        return float((w * ((q - Pc) ** 2).sum(1)).sum())
    e = 1e-4
    H = np.zeros((6, 6))
    for i in range(6):
        for k in range(6):
            di, dk = np.eye(6)[i] * e, np.eye(6)[k] * e
            H[i, k] = (cost_at(di + dk) - cost_at(di - dk) - cost_at(dk - di) + cost_at(-di - dk)) / (4 * e * e)
    ref = np.linalg.inv(H / 2.0)
    nrm = np.sqrt(np.outer(np.diag(Sg), np.diag(Sg)))
    assert (np.abs(Sg - ref) / nrm).max() < 1e-5, (np.abs(Sg - ref) / nrm).max()


# ---- what the device tests' tolerances are built from -----------------------------------------------------------------------

def test_stage_inputs_keep_small_triangles_rare_and_the_references_own_spreads_small():
    """On every frame set of tests/test_gpu_kabsch.py, from the reference's own hypotheses: hypotheses with a triangle below
    SMALL_AREA are at most 5 % of the valid ones; d_alg, d_perm and d_round are printed (DESIGN.md records them)."""
    worst_alg = worst_perm = worst_perm_cov = worst_round = 0.0
    for name in K.STAGE_SETS:
        s = K.stage_set(name)
        cams = K.cam_points32(s['depth'], s['camera'])
        kw = s['kw']
        thr = K.f32(kw['inlier_m'])
        valid = small = 0
        for b in range(s['records'].shape[0]):
            samples, hp, counts, (Pc, X, sig2) = K.hypotheses(s['records'][b], cams[b], 5 + b, kw['hypotheses'], kw['seed'],
                                                              kw['min_confidence'], kw['inlier_m'], kw['min_points'])
            for k in np.nonzero(counts >= 0)[0]:
                valid += 1
                if min(K.cross_norm(Pc[samples[k]]), K.cross_norm(X[samples[k]])) < K.SMALL_AREA:
                    small += 1
                else:
                    worst_alg = max(worst_alg, K.algorithm_spread(Pc, X, samples[k]))
            best = K.first_max(counts)
            assert best >= 0 and counts[best] >= 16
            for wt in (False, True):
                for iters in (1, 3, 10):
                    dp, dc = K.permutation_spread(*K.widen(hp[best]), Pc, X, sig2, wt, thr, iters, kw['point_sigma'])
                    worst_perm, worst_perm_cov = max(worst_perm, dp), max(worst_perm_cov, dc)
                R, t = K.refine(*K.widen(hp[best]), Pc, X, K.refine_weights(sig2, wt, kw['point_sigma']), thr, 10)
                worst_round = max(worst_round, K.rounding_spread(R, t, Pc, X, sig2, thr, kw['point_sigma']))
        print('%s: %d valid hypotheses, %d with a triangle below %g m^2 (%.2f %%)' % (name, valid, small, K.SMALL_AREA,
                                                                                     100.0 * small / valid))
        assert valid > 0 and small <= 0.05 * valid, (name, small, valid)
    print('d_alg %.3g, d_perm %.3g (pose) %.3g (covariance, cost), d_round %.3g' % (worst_alg, worst_perm, worst_perm_cov, worst_round))
    assert np.isfinite([worst_alg, worst_perm, worst_perm_cov, worst_round]).all()


# ---- the command line -------------------------------------------------------------------------------------------------------

def _run(args):
    e = dict(os.environ)
    e['PYTHONPATH'] = ROOT + os.pathsep + e.get('PYTHONPATH', '')
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                          timeout=300)


def test_depth_list_refuses_the_flags_of_pnp_with_one_line_and_status_1(tmp_path, capsys):
    lst = tmp_path / 'list.txt'
    lst.write_text(str(tmp_path / 'missing_coord_0.npy') + '\n')      # never read: the flags are checked first
    dl = tmp_path / 'depth_list.txt'
    dl.write_text(str(tmp_path / 'missing_depth_0.png') + '\n')
    out = tmp_path / 'out'
    base = [str(lst), str(out), '--depth_list', str(dl)]
    for flags, word in ((['--inlier_px', '5'], '--inlier_px'),
                        (['--weighted', '--pixel_sigma', '2'], '--pixel_sigma'),
                        (['--sampling', 'confidence'], '--sampling confidence'),
                        (['--sampling', 'confidence2', '--confidence_cap', '500'], '--sampling confidence2'),
                        (['--inlier_m', '0'], '--inlier_m'),
                        (['--point_sigma', '-1'], '--point_sigma'),
                        (['--min_confidence', '-1'], '--min_confidence')):
        capsys.readouterr()
        assert pnp.main(base + flags) == 1, flags
        text = capsys.readouterr()
        assert text.err == '' and text.out.count('\n') == 1 and word in text.out, (flags, text)
        assert not out.exists()
    r = _run(['-m', 'kfnet_amd.KFNet.pnp'] + base + ['--inlier_px', '5'])
    assert r.returncode == 1 and r.stdout.count('\n') == 1 and '--inlier_px' in r.stdout, r.stdout
    assert not out.exists()
    for flags in (['--inlier_m', '0.2'], ['--point_sigma', '0.02'], ['--depth_u', '316']):      # ... and the other way round
        with pytest.raises(SystemExit) as e:
            pnp.main([str(lst), str(out)] + flags)
        assert e.value.code == 2 and '--depth_list' in capsys.readouterr().err
    r = _run(['-m', 'kfnet_amd.KFNet.pnp', '--help'])
    assert r.returncode == 0
    for flag in ('--depth_list', '--inlier_m', '--point_sigma', '--depth_focal_x', '--depth_focal_y', '--depth_u', '--depth_v',
                 '--inlier_px'):
        assert flag in r.stdout, flag


# ---- exports ----------------------------------------------------------------------------------------------------------------

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


NAMES = ('kfn_kabsch_scratch_bytes', 'kfn_kabsch_ransac', 'kfn_kabsch_hypotheses', 'kfn_kabsch_select')


def test_descriptor_matches_the_header_and_the_abi_stays_13():
    hdr = open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()
    ctype = {'int32_t': C.c_int32, 'uint32_t': C.c_uint32, 'float': C.c_float}
    fields = _struct_fields(hdr, 'kfn_kabsch_desc')
    assert [(n, ctype[t]) for n, t in fields] == list(_lib.KabschDesc._fields_)
    assert fields[0][0] == 'struct_size' and _lib.KabschDesc().struct_size == C.sizeof(_lib.KabschDesc) == 4 * len(fields)
    init = re.search(r'#define KFN_KABSCH_DESC_INIT \{(.*)\}', hdr).group(1)
    assert len(init.split(',')) == len(fields)
    lib = _lib.load()
    assert lib.kfn_abi_version() == 13 == _lib.ABI_VERSION and '#define KFN_ABI_VERSION 13' in hdr
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NAMES:
        assert re.search(r'\bint %s\(' % name, hdr) and name in _lib.SYMBOLS and hasattr(lib, name) and name in doc, name
    assert build.EXTRA['kfn_kabsch.hip'] == ['-ffp-contract=off'] and 'kfn_kabsch.hip' in build.sources()
    src = open(os.path.join(ROOT, 'kfnet_amd', 'csrc', 'kfn_kabsch.hip')).read()
    assert len(re.findall(r'\batomicAdd\(&counts\[', src)) == len(re.findall(r'\batomic\w*\(', src)) == 1    # integer, once


def test_entry_points_validate_arguments_without_a_gpu():
    lib = _lib.load()
    dummy = C.c_void_p(16)          # never dereferenced: every call below fails its checks first
    solver = kabsch.KabschSolver(60, 80)
    nbytes = C.c_size_t()
    assert lib.kfn_kabsch_scratch_bytes(C.byref(solver.desc(2)), C.byref(nbytes)) == 0
    assert nbytes.value == 2 * 256 * 12 * 4 + 2 * 256 * 4
    assert lib.kfn_kabsch_scratch_bytes(C.byref(solver.desc(2)), None) == -1
    assert lib.kfn_kabsch_scratch_bytes(None, C.byref(nbytes)) == -1

    def ransac(null=None, **kw):
        d = solver.desc(2)
        for k, v in kw.items():
            setattr(d, k, v)
        args = [dummy] * 7
        if null is not None:
            args[null] = None
        return lib.kfn_kabsch_ransac(C.byref(d), *args, None)
    for kw in (dict(struct_size=8), dict(struct_size=0), dict(struct_size=58), dict(B=0), dict(h=0), dict(h=256, w=256),
               dict(ld=3), dict(ldp=3), dict(t0=-1), dict(hypotheses=0), dict(hypotheses=1025), dict(refine_iters=-1),
               dict(refine_iters=101), dict(min_points=2), dict(min_confidence=-1.0), dict(min_confidence=float('nan')),
               dict(inlier_m=0.0), dict(inlier_m=float('inf')), dict(weighted=2), dict(point_sigma=0.0),
               dict(point_sigma=float('nan'))):
        assert ransac(**kw) == -1, kw
        assert lib.kfn_last_error()
    assert ransac(point_sigma=0.0) == -1 and b'point_sigma' in lib.kfn_last_error()
    assert ransac(ldp=3) == -1 and b'ldp' in lib.kfn_last_error()
    for null in (0, 1, 2, 5, 6):                  # records, cam_points, poses, info, scratch; cov and quality may be null
        assert ransac(null=null) == -1 and b'null' in lib.kfn_last_error(), null
    d = solver.desc(2)
    assert lib.kfn_kabsch_ransac(C.byref(d), dummy, dummy, dummy, None, None, dummy, C.c_void_p(20), None) == -1
    assert b'aligned' in lib.kfn_last_error()
    for null in range(5):
        args = [dummy] * 5
        args[null] = None
        assert lib.kfn_kabsch_hypotheses(C.byref(d), *args, None) == -1, null
    assert lib.kfn_kabsch_select(None, 2, 256, dummy, None) == -1 and lib.kfn_kabsch_select(dummy, 2, 256, None, None) == -1
    assert lib.kfn_kabsch_select(dummy, 0, 256, dummy, None) == -1 and lib.kfn_kabsch_select(dummy, 2, 1025, dummy, None) == -1
    for kw in (dict(point_sigma=0.0), dict(inlier_m=0.0), dict(hypotheses=0), dict(min_confidence=-1.0), dict(min_points=2)):
        with pytest.raises(ValueError):
            kabsch.KabschSolver(60, 80, **kw)


# ---- --pose_depth of the eval programs ------------------------------------------------------------------------------------------

def test_pose_depth_flag_of_the_eval_programs(tmp_path, capsys):
    import argparse
    from kfnet_amd import modes

    def parse(args):
        ap = argparse.ArgumentParser()
        modes.add_pose_flags(ap)
        ap.add_argument('--input_folder', default='')
        a = ap.parse_args(args)
        return a, modes.pose_argument(a, ap)
    with pytest.raises(SystemExit) as e:                                      # no depth_list.txt there
        parse(['--pose_depth', '--input_folder', str(tmp_path)])
    assert e.value.code == 2 and 'depth_list.txt' in capsys.readouterr().err
    (tmp_path / 'depth_list.txt').write_text('a.png\nb.png\n\n')
    a, pose = parse(['--pose_depth', '--input_folder', str(tmp_path)])
    assert a.pose and not a.pose_weighted and isinstance(pose, modes.DepthPoseOptions)
    assert pose.depth_paths == ['a.png', 'b.png'] and not pose.weighted
    a, pose = parse(['--pose_depth', '--pose_smooth', '--input_folder', str(tmp_path)])
    assert a.pose and a.pose_weighted and pose.weighted
    with pytest.raises(SystemExit) as e:
        parse(['--pose_depth', '--pose_sampling', 'confidence2', '--input_folder', str(tmp_path)])
    assert e.value.code == 2 and '--pose_sampling' in capsys.readouterr().err
    a, pose = parse(['--pose', '--input_folder', str(tmp_path)])              # without the flag: what it was
    assert pose is True
    a, pose = parse(['--pose_weighted'])
    assert pose == modes.POSE_WEIGHTED
    solver = modes.solver_of(modes.DepthPoseOptions(True, ['a.png']), 8, 12)
    assert isinstance(solver, modes.DepthPoseSolver) and solver.weighted and solver.solver.camera.fx == 525.0
    with pytest.raises(ValueError):
        solver._depth(2, 0)                                                   # frame 1 has no depth map listed
    for prog in ('kfnet_amd.KFNet.eval', 'kfnet_amd.SCoordNet.eval'):
        r = _run(['-m', prog, '--help'])
        assert r.returncode == 0 and '--pose_depth' in r.stdout, prog
