"""CPU tests of the pose tracker (no GPU): that the numpy restatement tests/pose_track_ref.py is worth comparing a device
against (its walk is pnp_unc_ref.pose_filter, its velocity model and smoother are the textbook linear ones where the
problem is linear, smoothing helps, the velocity model follows smooth motion and its smoothed covariance is consistent),
the C surface of kfn_pose_track with its argument checks, and the command lines' flag checks."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pnp_ref as P
import pnp_unc_ref as U
import pose_track_ref as TR
from kfnet_amd import _lib
from kfnet_amd.KFNet import pose_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (1, 2, 3)
VELOCITY = dict(rot_sigma=0.004, trans_sigma=0.004, rot_rate_sigma=0.05, trans_rate_sigma=0.05)     # the issue's settings


def smooth_trajectory(seed, T=200, missing=0.1, wrong=0.05, twist_rot=0.01, twist_trans=0.03, accel=0.002):
    """pnp_unc_ref.synthetic_trajectory's measurement noise, covariances and kinds (the same seed draws the same ones)
    replayed on a trajectory whose body-frame twist does a random walk: it starts at twist_rot rad and twist_trans m per
    frame (0.6 degrees, 3 cm) and takes a white acceleration of `accel` per frame per axis.  (gt, meas, cov, kind) alike."""
    gt0, meas0, cov, kind = U.synthetic_trajectory(seed, T=T, missing=missing, wrong=wrong)
    rng = np.random.default_rng(seed + 100000)
    R, t = P.random_pose(rng)
    C0 = P.cam_to_world(R, t)
    dirs = rng.normal(size=(2, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    xi = np.concatenate([dirs[0] * twist_rot, dirs[1] * twist_trans])
    gt = np.zeros((T, 4, 4))
    for k in range(T):
        xi = xi + rng.normal(scale=accel, size=6)
        C0 = C0.copy()
        C0[:3, 3] = C0[:3, 3] + C0[:3, :3] @ xi[3:]
        C0[:3, :3] = C0[:3, :3] @ P.rodrigues(xi[:3])
        gt[k] = C0
    meas = np.full((T, 4, 4), np.nan, np.float32)
    for k in range(T):
        if kind[k] != 1:
            # the measurement's own body-frame error, taken from the random-walk set and applied to the new truth
            meas[k] = (gt[k] @ (np.linalg.inv(gt0[k]) @ meas0[k].astype(np.float64))).astype(np.float32)
    return gt, meas, cov, kind


_RUNS = {}


def runs(kind):
    """[(gt, meas, cov, kind, walk outputs, velocity outputs)] of seeds 1-3, both with smoothing; computed once."""
    if kind not in _RUNS:
        out = []
        for seed in SEEDS:
            gt, meas, cov, kd = U.synthetic_trajectory(seed) if kind == 'walk' else smooth_trajectory(seed)
            out.append((gt, meas, cov, kd, TR.track(meas, cov, 'walk', smooth=True),
                        TR.track(meas, cov, 'velocity', smooth=True, **VELOCITY)))
        _RUNS[kind] = out
    return _RUNS[kind]


def _median_cm(est, gt, good):
    return 100.0 * float(np.median(np.linalg.norm(est[good][:, :3, 3] - gt[good][:, :3, 3], axis=1)))


def test_walk_restatement_is_the_pose_filter_restatement():
    for seed in SEEDS:
        _, meas, cov, _ = U.synthetic_trajectory(seed)
        ref = U.pose_filter(meas, cov)
        got = TR.track(meas, cov, 'walk')
        assert len(got) == 4 and np.array_equal(got[2], ref[2])
        for g, r in zip((got[0], got[1], got[3]), (ref[0], ref[1], ref[3])):
            assert np.array_equal(np.isnan(g), np.isnan(r))
            assert np.nanmax(np.abs(g - r)) <= 1e-12


def test_velocity_model_and_smoother_are_the_textbook_linear_ones():
    """Identity rotations, block-diagonal covariances, pure translation: the error state is the state, and the tracker
    must be the linear position-velocity Kalman filter with F = [[I, I], [0, I]], Q = [[q/3, q/2], [q/2, q]] per axis and
    the RTS gain C = P_f F^T P_p^-1 -- written here on its own, with plain inverses."""
    rng = np.random.default_rng(11)
    T, q, r0 = 40, 0.004, 0.05
    vel = np.array([0.03, -0.01, 0.02])
    pos = np.cumsum(np.tile(vel, (T, 1)) + rng.normal(scale=0.002, size=(T, 3)), axis=0)
    Rm = []
    for _ in range(T):
        A = rng.normal(size=(3, 3)) * 0.02
        Rm.append((A @ A.T + 1e-4 * np.eye(3)).astype(np.float32).astype(np.float64))
    Rm = [(M + M.T) / 2 for M in Rm]
    z = (pos + np.stack([np.linalg.cholesky(M) @ rng.normal(size=3) for M in Rm])).astype(np.float32)
    meas = np.tile(np.eye(4, dtype=np.float32), (T, 1, 1))
    meas[:, :3, 3] = z
    cov = np.zeros((T, 6, 6), np.float32)
    for k in range(T):
        cov[k, :3, :3] = 1e-6 * np.eye(3)
        cov[k, 3:, 3:] = Rm[k]
    meas[7] = np.nan                       # a missing frame: predict only
    out = TR.track(meas, cov, 'velocity', smooth=True, rot_sigma=q, trans_sigma=q, rot_rate_sigma=r0, trans_rate_sigma=r0,
                   gate=1e9)
    assert (np.delete(out[2], 7)[1:] == TR.UPDATED).all() and out[2][0] == TR.INIT and out[2][7] == TR.MISSING
    # the textbook filter on (position, velocity), 6 states
    qf, rf = float(np.float32(q)) ** 2, float(np.float32(r0)) ** 2
    F = np.block([[np.eye(3), np.eye(3)], [np.zeros((3, 3)), np.eye(3)]])
    Q = np.block([[qf / 3 * np.eye(3), qf / 2 * np.eye(3)], [qf / 2 * np.eye(3), qf * np.eye(3)]])
    H = np.hstack([np.eye(3), np.zeros((3, 3))])
    xs, Ps, xp, Pp = [], [], [None], [None]
    x = np.concatenate([z[0].astype(np.float64), np.zeros(3)])
    Pk = np.block([[cov[0, 3:, 3:].astype(np.float64), np.zeros((3, 3))], [np.zeros((3, 3)), rf * np.eye(3)]])
    xs.append(x)
    Ps.append(Pk)
    for k in range(1, T):
        x, Pk = F @ x, F @ Pk @ F.T + Q
        xp.append(x)
        Pp.append(Pk)
        if k != 7:
            Rk = cov[k, 3:, 3:].astype(np.float64)
            K = Pk @ H.T @ np.linalg.inv(H @ Pk @ H.T + Rk)
            x = x + K @ (z[k].astype(np.float64) - H @ x)
            Pk = (np.eye(6) - K @ H) @ Pk
        xs.append(x)
        Ps.append(Pk)
    sx, sP = [None] * T, [None] * T
    sx[-1], sP[-1] = xs[-1], Ps[-1]
    for k in range(T - 2, -1, -1):
        G = Ps[k] @ F.T @ np.linalg.inv(Pp[k + 1])
        sx[k] = xs[k] + G @ (sx[k + 1] - xp[k + 1])
        sP[k] = Ps[k] + G @ (sP[k + 1] - Pp[k + 1]) @ G.T
    for k in range(T):
        assert np.abs(out[0][k, :3, 3] - xs[k][:3]).max() < 1e-10, k
        assert np.abs(out[1][k, 3:, 3:] - Ps[k][:3, :3]).max() < 1e-10, k
        assert np.abs(out[4][k, :3, 3] - sx[k][:3]).max() < 1e-10, k
        assert np.abs(out[5][k, 3:, 3:] - sP[k][:3, :3]).max() < 1e-10, k
        assert np.abs(out[0][k, :3, :3] - np.eye(3)).max() < 1e-10 and np.abs(out[4][k, :3, :3] - np.eye(3)).max() < 1e-10
    assert np.abs(out[4][:-1, :3, 3] - out[0][:-1, :3, 3]).max() > 1e-3         # the smoother moved something


def test_smoothing_and_the_velocity_model_help_where_the_issue_says():
    for kind in ('walk', 'smooth'):
        for seed, (gt, meas, cov, kd, walk, vel) in zip(SEEDS, runs(kind)):
            good = kd == 0
            raw = _median_cm(meas.astype(np.float64), gt, good)
            med = {name: (_median_cm(o[0], gt, good), _median_cm(o[4], gt, good)) for name, o in (('walk', walk), ('velocity', vel))}
            rejected = {name: int((o[2][good][1:] != TR.UPDATED).sum()) for name, o in (('walk', walk), ('velocity', vel))}
            print('%s motion, seed %d: raw %.2f cm; walk %.2f -> %.2f with RTS; velocity %.2f -> %.2f with RTS; good frames '
                  'rejected: walk %d, velocity %d of %d' % (kind, seed, raw, med['walk'][0], med['walk'][1], med['velocity'][0],
                                                           med['velocity'][1], rejected['walk'], rejected['velocity'],
                                                           int(good.sum()) - 1))
            for name in med:
                assert med[name][1] < med[name][0], (kind, seed, name, med[name])          # RTS below forward
            for o in (walk, vel):
                assert np.isin(o[2][kd == 2], (TR.REJECTED, TR.INIT)).all(), (kind, seed)     # every planted wrong pose
            if kind == 'smooth':
                assert med['velocity'][0] < raw, (seed, med, raw)
                assert rejected['velocity'] == 0, (seed, rejected)
                # why the model exists: on smooth motion the walk's gate throws good frames away
                assert rejected['walk'] >= 1, (seed, rejected)


def test_smoothed_covariance_is_consistent_on_smooth_motion():
    d2 = []
    for gt, meas, cov, kd, walk, vel in runs('smooth'):
        good = kd == 0
        d2.append(U.mahalanobis2(vel[4][good], vel[5][good], gt[good]))
    d2 = np.concatenate(d2)
    bound = 6.0 + 4.0 * np.sqrt(12.0 / d2.size)
    print('mean squared Mahalanobis distance of the true error under the smoothed covariance: %.3f over %d frames (at most %.3f)'
          % (d2.mean(), d2.size, bound))
    assert d2.mean() <= bound, d2.mean()          # conservative is accepted, optimistic is not


def _header():
    return open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()


def test_exports_descriptor_and_documents():
    hdr = _header()
    body = re.search(r'typedef struct kfn_pose_track_desc \{(.*?)\} kfn_pose_track_desc;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    ctype = {'int32_t': C.c_int32, 'float': C.c_float}
    fields = []
    for stmt in body.split(';'):
        if stmt.strip():
            typ, names = stmt.strip().split(None, 1)
            fields += [(n.strip(), ctype[typ]) for n in names.split(',')]
    assert fields == list(_lib.PoseTrackDesc._fields_)
    assert _lib.PoseTrackDesc().struct_size == C.sizeof(_lib.PoseTrackDesc) == 4 * len(fields) == 44
    assert '#define KFN_POSE_MODEL_WALK 0' in hdr and '#define KFN_POSE_MODEL_VELOCITY 1' in hdr
    assert (_lib.POSE_MODEL_WALK, _lib.POSE_MODEL_VELOCITY) == (0, 1)
    lib = _lib.load()
    assert lib.kfn_abi_version() == 13 == _lib.ABI_VERSION and '#define KFN_ABI_VERSION 13' in hdr
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ('kfn_pose_track', 'kfn_pose_track_state_bytes', 'kfn_pose_track_scratch_bytes'):
        assert re.search(r'\bint %s\(' % name, hdr) and name in _lib.SYMBOLS and hasattr(lib, name) and name in doc, name
    assert 'PoseTracker' in doc


def _desc(**kw):
    d = pose_filter.PoseTracker('velocity', smooth=True).desc(2, 8)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_size_queries():
    lib = _lib.load()
    n = C.c_size_t(7)
    for model, slot in ((0, 12 + 36), (1, 18 + 144)):
        nn = 6 if model == 0 else 12
        d = _desc(model=model, S=3, T=10)
        assert lib.kfn_pose_track_state_bytes(C.byref(d), C.byref(n)) == 0 and n.value == 8 * 3 * (2 + slot)
        assert lib.kfn_pose_track_scratch_bytes(C.byref(d), C.byref(n)) == 0 and n.value == 8 * 3 * (10 * 2 * slot + 2 * nn * nn)
        d.smooth = 0
        assert lib.kfn_pose_track_scratch_bytes(C.byref(d), C.byref(n)) == 0 and n.value == 0
    assert lib.kfn_pose_track_state_bytes(C.byref(_desc()), None) == -1
    assert lib.kfn_pose_track_state_bytes(None, C.byref(n)) == -1
    assert lib.kfn_pose_track_scratch_bytes(C.byref(_desc(model=2)), C.byref(n)) == -1


def test_entry_point_validates_arguments_without_a_gpu():
    lib = _lib.load()
    dummy = C.c_void_p(16)          # never dereferenced: every call below fails its checks first

    def call(d=None, null=(), **kw):
        d = _desc(**kw) if d is None else d
        args = [dummy] * 10          # poses cov state out_poses out_cov flags nis smooth_poses smooth_cov scratch
        for i in null:
            args[i] = None
        return lib.kfn_pose_track(C.byref(d) if d is not False else None, *args, None)
    assert call(d=False) == -1
    nan = float('nan')
    for kw in (dict(struct_size=8), dict(struct_size=0), dict(struct_size=40), dict(struct_size=46), dict(S=0), dict(T=0),
               dict(S=-1), dict(S=1 << 13, T=1 << 12), dict(model=2), dict(model=-1), dict(smooth=2), dict(rot_sigma=-0.1),
               dict(trans_sigma=nan), dict(rot_rate_sigma=0.0), dict(trans_rate_sigma=-1.0), dict(rot_rate_sigma=nan),
               dict(gate=0.0), dict(gate=nan), dict(max_rejects=0)):
        assert call(**kw) == -1, kw
    assert call(model=3) == -1 and b'model' in lib.kfn_last_error()
    assert call(rot_rate_sigma=0.0) == -1 and b'rot_rate_sigma' in lib.kfn_last_error()
    for null in (0, 1, 3, 4, 5, 6):               # the arguments kfn_pose_filter refuses
        assert call(null=(null,)) == -1, null
    for null in (7, 8, 9):                        # smooth = 1 without a smoothed output or scratch
        assert call(null=(null,)) == -1 and b'smooth' in lib.kfn_last_error(), null
    assert call(smooth=0) == -1                   # smooth = 0 with smoothed outputs
    # the walk ignores the rate sigmas
    assert call(model=0, rot_rate_sigma=0.0, null=(0,)) == -1 and b'null argument' in lib.kfn_last_error()
    bad = [dummy] * 10
    bad[2] = C.c_void_p(20)
    assert lib.kfn_pose_track(C.byref(_desc()), *bad, None) == -1 and b'aligned' in lib.kfn_last_error()


def test_pose_tracker_argument_errors():
    for kw in (dict(model='spline'), dict(max_rejects=0), dict(gate=0.0), dict(rot_sigma=-1.0), dict(trans_sigma=-1.0),
               dict(model='velocity', rot_rate_sigma=0.0), dict(model='velocity', trans_rate_sigma=-0.1)):
        with pytest.raises(ValueError):
            pose_filter.PoseTracker(**kw)
    assert pose_filter.PoseTracker('walk', rot_rate_sigma=0.0).rot_sigma == 0.02          # defaults follow the model
    t = pose_filter.PoseTracker('velocity')
    assert (t.rot_sigma, t.trans_sigma, t.rot_rate_sigma, t.trans_rate_sigma, t.smooth) == (0.005, 0.005, 0.05, 0.05, False)
    d = t.desc(2, 8)
    assert (d.model, d.smooth, d.S, d.T, d.max_rejects) == (1, 0, 2, 8, 3)


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
    for flags, word in ((['--rts'], '--rts'), (['--motion', 'velocity'], '--motion'), (['--rot_rate_sigma', '0.1'], '--smooth'),
                        (['--trans_rate_sigma', '0.1'], '--smooth'), (['--smooth', '--motion', 'spline'], '--motion'),
                        (['--smooth', '--motion', 'velocity', '--rot_rate_sigma', '0'], '--rot_rate_sigma')):
        r = _run(['-m', 'kfnet_amd.KFNet.pnp', str(lst), str(out)] + flags)
        assert r.returncode == 2 and word in r.stdout, (flags, r.stdout)
        assert not out.exists()
    r = _run(['-m', 'kfnet_amd.KFNet.pnp', '--help'])
    assert r.returncode == 0
    for flag in ('--motion', '--rts', '--rot_rate_sigma', '--trans_rate_sigma'):
        assert flag in r.stdout, flag
    hidden = {'HIP_VISIBLE_DEVICES': '', 'CUDA_VISIBLE_DEVICES': ''}        # a refusal must come before any device is needed
    for prog in ('kfnet_amd.KFNet.eval', 'kfnet_amd.SCoordNet.eval'):
        r = _run(['-m', prog, '--help'])
        assert r.returncode == 0
        for flag in ('--pose_smooth', '--pose_motion', '--pose_sequence_length'):
            assert flag in r.stdout, (prog, flag)
        r = _run(['-m', prog, '--scene', 'chess', '--synthetic', '4', '--random_weights', '--pose_motion', 'velocity'])
        assert r.returncode == 2 and '--pose_smooth' in r.stdout, (prog, r.stdout)
        r = _run(['-m', prog, '--scene', 'chess', '--synthetic', '4', '--random_weights', '--pose_smooth',
                  '--output_folder', str(out)], env=dict(hidden, WORLD_SIZE='2', RANK='0', LOCAL_RANK='0'))
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert r.returncode == 1 and len(lines) == 1 and '--pose_smooth' in lines[0], (prog, r.stdout)
