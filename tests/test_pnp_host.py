"""CPU tests of the camera-pose stage (no GPU): the sampling hash, P3P and RANSAC of the numpy restatement
(tests/pnp_ref.py), pose files and errors, the kfn_pnp_* C surface and its argument checks, the command lines."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pnp_ref as P
from kfnet_amd import _lib
from kfnet_amd.KFNet import pnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hash_known_answers():
    """lowbias32 and the sampling key of DESIGN.md "Camera poses" (constants fixed once; a numpy uint32 restatement
    agrees)."""
    assert P.lowbias32(0) == 0
    assert P.lowbias32(1) == 0x688990c0
    assert P.lowbias32(0xdeadbeef) == 0xe628c683
    assert P.lowbias32(0xffffffff) == 0x6768824a
    assert P.sample_hash(0, 1, 0, 0) == 0x6d523710
    assert P.sample_hash(12345, 7, 200, 3) == 0x1782dcb2
    x = np.array([1, 0xdeadbeef, 0xffffffff], dtype=np.uint32)
    with np.errstate(over='ignore'):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7feb352d)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846ca68b)
        x ^= x >> np.uint32(16)
    assert [int(v) for v in x] == [0x688990c0, 0xe628c683, 0x6768824a]
    # candidate index = (h * n) >> 32; four distinct indices in draw order
    assert P.draw_sample(0, 0, 0, 4800) == [0, 3195, 2218, 4002]
    assert P.draw_sample(0, 5, 17, 100) == [66, 55, 35, 59]
    assert P.draw_sample(0, 0, 0, 3) is None          # 4 distinct out of 3 candidates never happens


def test_p3p_returns_the_true_pose_among_its_solutions():
    rng = np.random.default_rng(11)
    for _ in range(20):
        R, t = P.random_pose(rng)
        pix = np.array([[80., 96.], [560., 120.], [320., 400.]])
        z = rng.uniform(0.5, 5.0, 3)
        Xc = np.stack([(pix[:, 0] - 320) / 525 * z, (pix[:, 1] - 240) / 525 * z, z], 1)
        X = (Xc - t) @ R
        F = np.stack([P.bearing(p, 525., 525., 320., 240.) for p in pix])
        sols = P.p3p(X, F)
        assert 1 <= len(sols) <= 4
        err = min(max(np.abs(Rs - R).max(), np.abs(ts - t).max()) for Rs, ts in sols)
        assert err < 1e-9, err


def test_quartic_roots():
    roots = sorted(P.solve_quartic(1.0, -10.0, 35.0, -50.0, 24.0))      # (x-1)(x-2)(x-3)(x-4)
    assert np.allclose(roots, [1, 2, 3, 4], atol=1e-12)
    assert P.solve_quartic(1.0, 0.0, 0.0, 0.0, 1.0) == []              # x^4 + 1: no real root


def _frames(rng, B, h, w, outliers=0.0, noise=0.0):
    recs, gts = [], []
    for _ in range(B):
        R, t = P.random_pose(rng)
        rec = P.synthetic_records(rng, h, w, R, t)
        if noise:
            rec[..., :3] += rng.normal(scale=noise, size=rec[..., :3].shape).astype(np.float32)
        if outliers:
            out = rng.random((h, w)) < outliers
            rec[..., :3][out] = rng.uniform(-5, 5, size=(int(out.sum()), 3)).astype(np.float32)
        recs.append(rec)
        gts.append(P.cam_to_world(R, t))
    return np.stack(recs), np.stack(gts)


def test_reference_ransac_recovers_synthetic_poses():
    rng = np.random.default_rng(3)
    recs, gts = _frames(rng, 2, 30, 40)
    poses, info = P.ransac(recs, hypotheses_n=64)
    rot, trans = pnp.pose_errors(poses, gts)
    assert (info[:, 0] == P.OK).all() and (info[:, 1] == 1200).all() and (info[:, 2] == 1200).all()
    assert rot.max() < 1e-2 and trans.max() < 1e-3
    recs, gts = _frames(rng, 2, 30, 40, outliers=0.5, noise=0.01)
    poses, info = P.ransac(recs, hypotheses_n=256)
    rot, trans = pnp.pose_errors(poses, gts)
    assert (info[:, 0] == P.OK).all()
    assert rot.max() < 0.5 and trans.max() < 0.02, (rot, trans)


def test_reference_too_few_candidates():
    rng = np.random.default_rng(4)
    recs, _ = _frames(rng, 1, 8, 8)
    recs[0, ..., 3] = 5.0                     # every cell below the confidence threshold
    recs[0, 0, :, 3] = 100.0
    recs[0, 1, :2, 3] = 100.0
    poses, info = P.ransac(recs, min_points=16)
    assert tuple(info[0]) == (P.TOO_FEW, 10, 0, -1) and np.isnan(poses).all()


def test_pose_errors_known_answers():
    I = np.eye(4)
    Rz = np.eye(4)
    Rz[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    rot, trans = pnp.pose_errors(Rz, I)
    assert abs(rot - 90.0) < 1e-9 and trans == 0.0
    T = np.eye(4)
    T[:3, 3] = [0.03, 0.0, 0.04]
    rot, trans = pnp.pose_errors(T, I)
    assert rot == 0.0 and abs(trans - 0.05) < 1e-12
    small = np.eye(4)
    small[:3, :3] = P.rodrigues(np.array([0.0, 0.0, np.radians(0.005)]))
    assert abs(pnp.pose_errors(small.astype(np.float32), I)[0] - 0.005) < 1e-4    # resolved from fp32 poses
    flip = np.diag([-1.0, -1.0, 1.0, 1.0])
    assert abs(pnp.pose_errors(flip, I)[0] - 180.0) < 1e-9
    assert np.isnan(pnp.pose_errors(np.full((4, 4), np.nan), I)[0])
    mr, mt, within = pnp.summarize(np.array([1.0, 10.0, np.nan]), np.array([0.01, 0.01, np.nan]))
    assert within == pytest.approx(1 / 3) and mr == 10.0 and mt == 0.01


def test_pose_file_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    R, t = P.random_pose(rng)
    T = P.cam_to_world(R, t)
    f = str(tmp_path / 'pose_0.txt')
    pnp.write_pose(f, T)
    assert np.abs(pnp.read_pose(f) - T).max() < 1e-8
    assert len(open(f).read().split()) == 16
    pnp.write_pose(f, np.full((4, 4), np.nan))
    assert np.isnan(pnp.read_pose(f)).all()
    (tmp_path / 'bad.txt').write_text('1 2 3\n4 5 6\n')
    with pytest.raises(ValueError):
        pnp.read_pose(str(tmp_path / 'bad.txt'))


def test_pnp_desc_matches_header():
    hdr = open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()
    body = re.search(r'typedef struct kfn_pnp_desc \{(.*?)\} kfn_pnp_desc;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for stmt in body.split(';'):
        stmt = stmt.strip()
        if stmt:
            typ, names = stmt.split(None, 1)
            fields += [(n.strip(), typ) for n in names.split(',')]
    ctype = {'int32_t': C.c_int32, 'uint32_t': C.c_uint32, 'float': C.c_float}
    assert [(n, ctype[t]) for n, t in fields] == [(n, t) for n, t in _lib.PnPDesc._fields_]
    assert fields[0][0] == 'struct_size'
    assert _lib.PnPDesc().struct_size == C.sizeof(_lib.PnPDesc) == 4 * len(fields)
    assert re.search(r'#define KFN_PNP_MAX_HYPOTHESES (\d+)', hdr).group(1) == str(_lib.PNP_MAX_HYPOTHESES)
    for name, val in (('OK', _lib.PNP_OK), ('TOO_FEW_POINTS', _lib.PNP_TOO_FEW_POINTS),
                      ('NO_HYPOTHESIS', _lib.PNP_NO_HYPOTHESIS)):
        assert re.search(r'#define KFN_PNP_%s (\d+)' % name, hdr).group(1) == str(val)
    for name in ('kfn_pnp_scratch_bytes', 'kfn_pnp_ransac', 'kfn_pnp_hypotheses'):
        assert name in _lib.SYMBOLS


def _good_desc(**kw):
    d = pnp.PnPSolver(60, 80).desc(2)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_pnp_entry_points_validate_arguments_without_a_gpu():
    lib = _lib.load()
    nb = C.c_size_t()
    assert lib.kfn_pnp_scratch_bytes(C.byref(_good_desc()), C.byref(nb)) == 0
    assert nb.value >= 2 * 256 * 13 * 4
    dummy = C.c_void_p(16)       # never dereferenced: every call below fails its checks first
    bad = [dict(B=0), dict(B=-1), dict(hypotheses=1025), dict(hypotheses=0), dict(ld=3), dict(min_points=3),
           dict(h=0), dict(h=200, w=200), dict(fx=0.0), dict(inlier_px=0.0), dict(cell_stride=0), dict(t0=-1),
           dict(refine_iters=-1), dict(struct_size=8), dict(struct_size=C.sizeof(_lib.PnPDesc) + 2)]
    for kw in bad:
        d = _good_desc(**kw)
        assert lib.kfn_pnp_scratch_bytes(C.byref(d), C.byref(nb)) == -1, kw
        assert lib.kfn_pnp_ransac(C.byref(d), dummy, dummy, dummy, dummy, None) == -1, kw
        assert lib.kfn_pnp_hypotheses(C.byref(d), dummy, dummy, dummy, dummy, None) == -1, kw
    assert b'hypotheses' in (lib.kfn_pnp_scratch_bytes(C.byref(_good_desc(hypotheses=1025)), C.byref(nb)) == -1
                             and lib.kfn_last_error())
    assert lib.kfn_pnp_scratch_bytes(None, C.byref(nb)) == -1
    assert lib.kfn_pnp_scratch_bytes(C.byref(_good_desc()), None) == -1
    d = _good_desc()
    assert lib.kfn_pnp_ransac(C.byref(d), None, dummy, dummy, dummy, None) == -1
    assert lib.kfn_pnp_ransac(C.byref(d), dummy, None, dummy, dummy, None) == -1
    assert lib.kfn_pnp_ransac(C.byref(d), dummy, dummy, None, dummy, None) == -1
    assert lib.kfn_pnp_ransac(C.byref(d), dummy, dummy, dummy, None, None) == -1
    assert b'null' in lib.kfn_last_error()
    assert lib.kfn_pnp_ransac(C.byref(d), dummy, dummy, dummy, C.c_void_p(20), None) == -1    # misaligned scratch
    assert lib.kfn_pnp_hypotheses(C.byref(d), dummy, None, dummy, dummy, None) == -1
    assert lib.kfn_pnp_hypotheses(C.byref(d), dummy, dummy, dummy, None, None) == -1
    with pytest.raises(ValueError):
        pnp.PnPSolver(60, 80, hypotheses=2048)


def _run(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    e['PYTHONPATH'] = ROOT + os.pathsep + e.get('PYTHONPATH', '')
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, timeout=300)


def test_pnp_cli_help():
    r = _run(['-m', 'kfnet_amd.KFNet.pnp', '--help'])
    assert r.returncode == 0, r.stdout
    for flag in ('coord_file_list', 'output_folder', '--gt', '--thread_num', '--focal_x', '--u', '--v', '--hypotheses',
                 '--batch'):
        assert flag in r.stdout


def test_eval_pose_is_refused_in_the_sharded_run(tmp_path):
    r = _run(['-m', 'kfnet_amd.KFNet.eval', '--scene', 'chess', '--synthetic', '4', '--random_weights', '--pose',
              '--output_folder', str(tmp_path)], env={'WORLD_SIZE': '2', 'RANK': '0'})
    assert r.returncode == 2, r.stdout
    assert '--pose is not supported in the sharded run' in r.stdout
    assert os.listdir(str(tmp_path)) == []
