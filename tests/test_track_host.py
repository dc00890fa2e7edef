"""Tracking against the TSDF volume, the host side: the exports and their refusals without a device, the
program's parser, refusals and files, hand cases of the numpy restatement (tests/track_ref.py), and the restatement tracking
a rendered sequence.  Nothing here needs a device."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fuse_ref as F
import render_ref as R
import track_ref as T
from kfnet_amd import _lib, synth
from kfnet_amd import track as M
from kfnet_amd.labels import DepthCamera, read_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The restatement on the 12 frames of track_ref.sequence_trajectory (0.03 rad of phase a frame), recorded on the CPU
# (DESIGN.md 6l): its worst translation error in voxels of 0.04 m and its worst rotation error in degrees.
RECORDED_VOXELS, RECORDED_DEGREES = 0.111684, 0.085162


# -- 1. the exports: present, the ABI number, the build entry, the structs ------------------------------------------------------------
def _header_struct(name):
    hdr = open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()
    body = hdr[hdr.index('typedef struct %s {' % name):]
    body = body[:body.index('} %s;' % name)]
    fields = []
    for kind, names in re.findall(r'^\s*(int32_t|float|double)\s+([\w\[\], ]+);', body, re.M):
        fields += [(n.strip().split('[')[0], kind, n.strip()) for n in names.split(',')]
    return fields


def test_exports_abi_number_build_entry_and_structs():
    lib = _lib.load()
    assert lib.kfn_abi_version() == 13 and _lib.ABI_VERSION == 13
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ('kfn_track_scratch_bytes', 'kfn_track_live_maps', 'kfn_track_raycast', 'kfn_track_icp_sums', 'kfn_track_update',
                 'kfn_track_commit'):
        assert name in _lib.SYMBOLS and getattr(raw, name) is not None
    hdr = open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()
    assert '#define KFN_ABI_VERSION 13' in hdr
    for text in ('kfn_track_live_maps:', 'kfn_track_raycast:', 'kfn_track_icp_sums:', 'kfn_track_update (one wave', 'kfn_track_commit (one wave',
                 'compared in float before the conversion', 'No floating-point atomics'):
        assert text in hdr, text
    assert C.sizeof(_lib.FuseDesc) == 104
    assert C.sizeof(_lib.TrackDesc) == 140 and C.sizeof(_lib.TrackState) == 232
    kinds = {C.c_int32: 'int32_t', C.c_float: 'float', C.c_double: 'double'}
    assert [(n, kinds[t]) for n, t in _lib.TrackDesc._fields_] == [(n, k) for n, k, _ in _header_struct('kfn_track_desc')]
    got = [(n, kinds.get(t, 'double'), getattr(t, '_length_', 1)) for n, t in _lib.TrackState._fields_]
    want = [(n, k, int(full.split('[')[1][:-1]) if '[' in full else 1) for n, k, full in _header_struct('kfn_track_state')]
    assert got == want
    from kfnet_amd import build
    assert build.EXTRA['kfn_track.hip'] == ['-ffp-contract=off'] and 'kfn_track.hip' in build.sources()
    cam = DepthCamera(585.0, 583.0, 317.5, 241.25, depth_fx=570.0, depth_v=250.5)
    d = M.track_descriptor(cam, (3, 4, 5), (0.1, 0.2, 0.3), 0.02, 0.08, (48, 64), level=2)
    assert (d.nx, d.ny, d.nz, d.H, d.W, d.levels, d.level) == (3, 4, 5, 48, 64, 3, 2) and d.struct_size == 140
    assert (d.dfx, d.dfy, d.du, d.dv) == (570.0, 583.0, 317.5, 250.5) and d.cos_min == np.float32(math.cos(math.radians(20.0)))
    assert d.scale == np.float32(0.001) and (d.raw_min, d.raw_max, d.min_pairs) == (1, 65534, 50)
    assert M.level_sizes((50, 70), 3) == [(50, 70, 0), (25, 35, 3500), (12, 17, 4375)]
    assert [l[:3] for l in T.levels_of(F.Setup((4, 4, 4), (0, 0, 0), 0.1, image_size=(50, 70)), 3)] == M.level_sizes((50, 70), 3)


# -- 2. the refusals of every export, without a device ---------------------------------------------------------------------------------
CAM = DepthCamera()
A16 = 0x1000


def _desc(**change):
    kw = dict(camera=CAM, dims=(8, 8, 8), origin=(0.0, 0.0, 0.0), voxel=0.05, trunc=0.2, image_size=(16, 24))
    fields = dict((k, change.pop(k)) for k in list(change) if k in ('struct_size', 'raw_min', 'raw_max', 'scale', 'dfx', 'H', 'W'))
    kw.update(change)
    d = M.track_descriptor(kw.pop('camera'), kw.pop('dims'), kw.pop('origin'), kw.pop('voxel'), kw.pop('trunc'), kw.pop('image_size'), **kw)
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def _calls(lib):
    return {
        'live_maps': lambda d, p=(A16,) * 3: lib.kfn_track_live_maps(C.byref(d), p[0], p[1], p[2], None),
        'raycast': lambda d, p=(A16,) * 4: lib.kfn_track_raycast(C.byref(d), p[0], p[1], p[2], p[3], None),
        'icp_sums': lambda d, p=(A16,) * 7: lib.kfn_track_icp_sums(C.byref(d), p[0], p[1], p[2], p[3], p[4], p[5], p[6], None),
        'update': lambda d, p=(A16,) * 2: lib.kfn_track_update(C.byref(d), p[0], p[1], None),
        'commit': lambda d, p=(A16,) * 3: lib.kfn_track_commit(C.byref(d), p[0], p[1], p[2], None),
    }


POINTERS = {'live_maps': 3, 'raycast': 4, 'icp_sums': 7, 'update': 2, 'commit': 3}


def test_argument_checks_of_every_export():
    lib = _lib.load()
    calls = _calls(lib)
    msg = lambda: lib.kfn_last_error().decode()
    common = ((dict(struct_size=136), 'struct_size'), (dict(H=0), 'image size'), (dict(W=-3), 'image size'), (dict(levels=0), 'levels'),
              (dict(levels=5), 'levels'), (dict(image_size=(4, 24)), 'below 2x2'), (dict(level=3), 'level'), (dict(level=-1), 'level'),
              (dict(dfx=0.0), 'focal'), (dict(near=0.0), 'near'))
    own = {
        'live_maps': ((dict(scale=0.0), 'scale'), (dict(raw_min=-1), 'window'), (dict(raw_max=65536), 'window'), (dict(pyr_dist=-1.0), 'pyr_dist'),
                      (dict(jump=float('nan')), 'jump')),
        'raycast': ((dict(dims=(1, 8, 8)), 'lattice'), (dict(dims=(2048, 1024, 1024)), '2^31'), (dict(voxel=0.0), 'voxel'), (dict(trunc=-1.0), 'trunc'),
                    (dict(far=0.01), 'far'), (dict(min_weight=0.5), 'min_weight'), (dict(origin=(np.inf, 0, 0)), 'origin')),
        'icp_sums': ((dict(dist_max=0.0), 'dist_max'), (dict(angle_max=float('nan')), 'cos_min')),
        'update': ((dict(min_pairs=5), 'min_pairs'), (dict(pivot_floor=-1.0), 'pivot_floor'), (dict(pivot_floor=1.0), 'pivot_floor')),
        'commit': ((dict(slot=-1), 'slot'), (dict(slot=65535), 'slot'), (dict(traj_rows=0), 'traj_rows'), (dict(min_share=1.5), 'min_share'),
                   (dict(max_rms=0.0), 'max_rms'), (dict(max_step_m=-1.0), 'max_step_m'), (dict(max_step_rad=0.0), 'max_step_rad')),
    }
    for name, call in calls.items():
        n = POINTERS[name]
        for change, word in common + own[name]:
            assert call(_desc(**change), (A16,) * n) == -1 and word in msg(), (name, change, msg())
        for k in range(n):                                   # every buffer: NULL, then misaligned
            assert call(_desc(), tuple(None if j == k else A16 for j in range(n))) == -1 and 'null' in msg(), (name, k, msg())
            bad = call(_desc(), tuple(A16 + 1 if j == k else A16 for j in range(n)))
            assert bad == -1 and 'aligned' in msg(), (name, k, msg())
    assert lib.kfn_track_live_maps(None, A16, A16, A16, None) == -1 and 'null descriptor' in msg()
    size = C.c_size_t()
    assert lib.kfn_track_scratch_bytes(C.byref(_desc(image_size=(480, 640))), C.byref(size)) == 0 and size.value == 300 * 32 * 8
    assert lib.kfn_track_scratch_bytes(C.byref(_desc(image_size=(50, 70))), C.byref(size)) == 0 and size.value == 4 * 32 * 8
    assert lib.kfn_track_scratch_bytes(C.byref(_desc()), None) == -1 and lib.kfn_track_scratch_bytes(C.byref(_desc(levels=9)), C.byref(size)) == -1


# -- 3. the program: parser, refusals, read_frames, the files it writes ----------------------------------------------------------------
def _touch_frames(folder, count, colour=True):
    for k in range(count):
        (folder / ('frame-%06d.depth.png' % k)).write_bytes(b'')
        if colour:
            (folder / ('frame-%06d.color.png' % k)).write_bytes(b'')


def test_read_frames_with_and_without_pose_files(tmp_path):
    seq = tmp_path / 'seq'
    seq.mkdir()
    with pytest.raises(ValueError) as e:
        read_frames(str(seq))
    assert 'holds no frame-*.depth.png' in str(e.value)
    with pytest.raises(ValueError) as e:
        read_frames(str(tmp_path / 'nowhere'))
    assert 'is not a folder' in str(e.value)
    _touch_frames(seq, 3)
    pairs = read_frames(str(seq))
    assert [os.path.basename(c) for c, d in pairs] == ['frame-%06d.color.png' % k for k in range(3)]
    assert [os.path.basename(d) for c, d in pairs] == ['frame-%06d.depth.png' % k for k in range(3)]
    np.savetxt(str(seq / 'frame-000001.pose.txt'), np.eye(4))
    assert read_frames(str(seq)) == pairs
    (seq / 'frame-000002.color.png').unlink()
    with pytest.raises(ValueError) as e:
        read_frames(str(seq))
    assert 'frame-000002.color.png is missing' in str(e.value)


def test_track_make_argument_errors(tmp_path, capsys):
    out = str(tmp_path / 'out')
    seq = tmp_path / 'seq'
    seq.mkdir()
    ok = ['make', '--sequence', str(seq), '--output_folder', out]
    for args, word in ((['make', '--output_folder', out], '--sequence'), (['make', '--sequence', str(seq)], '--output_folder'),
                       (ok + ['--bounds', '0', '0', '0', '1', '1', '1', '--extent', '3'], 'exclude'),
                       (ok + ['--voxel', '0'], '--voxel'), (ok + ['--trunc', '-1'], '--trunc'), (ok + ['--extent', '0'], '--extent'),
                       (ok + ['--dist_max', '0'], '--dist_max'), (ok + ['--angle_max', '-5'], '--angle_max'),
                       (ok + ['--min_weight', '0.5'], '--min_weight'), (ok + ['--height', '0'], 'multiples of 8'),
                       (ok + ['--width', '-8'], 'multiples of 8'), (ok + ['--levels', '0', '--iterations', '3'], 'levels'),
                       (ok + ['--iterations', '10', '5'], '2 iteration counts for 3 levels'),
                       (ok + ['--levels', '2'], 'needs --iterations'), (ok + ['--levels', '2', '--iterations', '4', '3', '2'], '3 iteration counts'),
                       (ok + ['--iterations', '0', '0', '0'], 'not all zero'), (ok + ['--focal_x', '-3'], 'positive'),
                       (ok, 'holds no frame-*.depth.png'),
                       (['make', '--sequence', str(tmp_path / 'nowhere'), '--output_folder', out], 'nowhere is not a folder')):
        assert M.main(args) == 1, args
        err = capsys.readouterr().err
        assert word in err and len(err.strip().split('\n')) == 1, (args, err)
    _touch_frames(seq, 2)
    for args, word in ((ok + ['--bounds', '0', '0', '0', '1', '0', '1'], 'the box is empty'),
                       (ok + ['--extent', '40', '--voxel', '0.02'], 'do not fit int32'),
                       (ok + ['--first_pose', str(tmp_path / 'none.txt')], 'none.txt')):
        assert M.main(args) == 1, args
        err = capsys.readouterr().err
        assert word in err and len(err.strip().split('\n')) == 1, err
    assert M.main([]) == 1
    assert not os.path.exists(out)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'kfnet_amd.track', 'make', '--help'], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ('--sequence', '--output_folder', '--first_pose', '--mesh', '--voxel', '--trunc', '--bounds', '--extent', '--min_weight',
                 '--no_color', '--depth_focal_x', '--focal_x', '--height', '--gpu', '--dist_max', '--angle_max', '--levels', '--iterations'):
        assert flag in r.stdout, flag


def test_written_lists_pose_files_and_report(tmp_path):
    from kfnet_amd.KFNet.pnp import read_pose
    from kfnet_amd.tools.io import read_lines
    seq, out = tmp_path / 'seq', tmp_path / 'out'
    seq.mkdir()
    _touch_frames(seq, 4)
    pairs = read_frames(str(seq))
    poses = synth.synthetic_poses(4)
    poses[2] = np.nan
    lost = np.array([False, False, True, False])
    diag = np.array([[0, 0, 0, 0, 0, 0, 0, 0], [0, 4208, 0.685, 2.79e-3, 19, 19, 0.0216, 9.5e-3], [1, 0, 0, 0, 0, 19, 0, 0],
                     [0, 4427, 0.72, 2.4e-3, 18, 19, 0.02, 0.01]], dtype=np.float64)
    M.write_outputs(str(out), pairs, poses, lost, diag)
    lists = [[x for x in read_lines(str(out / name)) if x] for name in ('image_list.txt', 'depth_list.txt', 'pose_list.txt')]
    assert [len(l) for l in lists] == [3, 3, 3]
    assert [os.path.basename(p) for p in lists[2]] == ['frame-000000.pose.txt', 'frame-000001.pose.txt', 'frame-000003.pose.txt']
    assert lists[0] == [os.path.abspath(pairs[k][0]) for k in (0, 1, 3)] and lists[1] == [os.path.abspath(pairs[k][1]) for k in (0, 1, 3)]
    assert not (out / 'frame-000002.pose.txt').exists()
    for p, k in zip(lists[2], (0, 1, 3)):
        assert np.abs(read_pose(p) - poses[k]).max() <= 1e-9 * 2.0                 # %.9e: nine digits behind the first
    # the output folder is a sequence for the other programs as they are
    from kfnet_amd.labels import read_sequence
    assert [t[2] for t in read_sequence(str(out))] == lists[2]
    report = [x for x in read_lines(str(out / 'track_report.txt')) if x]
    assert report[0].startswith('# frame state pairs share rms accepted iterations step_m step_rad') and len(report) == 5
    words = report[2].split()
    assert words[:2] == ['frame-000001.depth.png', 'tracked'] and int(words[2]) == 4208 and float(words[3]) == 0.685 and int(words[5]) == 19
    assert report[3].split()[:2] == ['frame-000002.depth.png', 'lost']
    lo, hi = M.box_in_front(np.eye(4), 4.0)
    assert lo.tolist() == [-2.0, -2.0, 0.0] and hi.tolist() == [2.0, 2.0, 4.0]


def test_tracker_refusals_before_a_device():
    with pytest.raises(ValueError) as e:
        M.check_levels((64, 96), 3, (10, 5))
    assert '2 iteration counts for 3 levels' in str(e.value)
    with pytest.raises(ValueError):
        M.check_levels((64, 96), 5, (1,) * 5)
    with pytest.raises(ValueError):
        M.check_levels((4, 96), 3, (1, 1, 1))
    assert M.check_levels((64, 96), 3, [10, 5, 4]) == (10, 5, 4)
    st = M.pose_record(np.eye(4), frame=3)
    assert list(st.committed) == list(st.estimate) == np.eye(4)[:3].ravel().tolist() and st.frame == 3
    with pytest.raises(ValueError):
        M.pose_record(np.eye(3))


# -- 4. hand cases of the restatement ----------------------------------------------------------------------------------------------------
PLANE = F.Setup(dims=(24, 24, 24), origin=(0.0, 0.0, 0.0), voxel=0.125, fx=20.0, fy=20.0, u=11.5, v=7.5, image_size=(16, 24))
PARAMS1 = T.Params(levels=1, iterations=(1,), min_pairs=6)


def _plane_volume():
    return F.field_volume(PLANE, lambda X, Y, Z: F.PLANE_OFFSET - Z)


def _camera_at(z):
    P = np.eye(4)
    P[:3, 3] = (1.5, 1.5, z)
    return P


def test_ray_cast_of_a_fronto_parallel_plane():
    mv, mn = T.raycast(_plane_volume(), _camera_at(0.2)[:3].reshape(12), PLANE, PARAMS1, 0)
    assert (mv[:, 3] == 1).all() and (mn[:, 3] == 1).all()
    assert np.abs(mv[:, 2].astype(np.float64) - F.PLANE_OFFSET).max() <= 0.01 * PLANE.voxel        # a fraction of a voxel
    assert np.abs(mn[:, :3] - np.array([0, 0, -1], dtype=np.float32)).max() <= 1e-5
    xs = (np.arange(24) - 11.5) / 20.0 * (F.PLANE_OFFSET - 0.2) + 1.5
    assert np.abs(mv[:24, 0] - xs).max() <= 1e-5
    # looking away: every pixel is invalid; so is a non-finite pose, and a camera behind the plane sees a back face
    away = _camera_at(0.2)
    away[:3, :3] = np.diag([1.0, -1.0, -1.0])
    for pose in (away, _camera_at(np.nan), _camera_at(2.5)):
        v, n = T.raycast(_plane_volume(), pose[:3].reshape(12), PLANE, PARAMS1, 0)
        assert not v.any() and not n.any()
    # a slab of W = 0 over the crossing: the rays through it are invalid, the others as before
    tsdf = _plane_volume()
    tsdf[9:13, :, :12, 1] = 0.0
    v, n = T.raycast(tsdf, _camera_at(0.2)[:3].reshape(12), PLANE, PARAMS1, 0)
    hidden = mv[:, 0] < 11 * PLANE.voxel - 1e-6
    assert hidden.any() and not v[hidden, 3].any() and np.array_equal(v[mv[:, 0] > 12 * PLANE.voxel], mv[mv[:, 0] > 12 * PLANE.voxel])


def test_icp_sums_of_a_translation_along_the_normal():
    committed, truth = _camera_at(0.2), _camera_at(0.2325)
    mv, mn = T.raycast(_plane_volume(), committed[:3].reshape(12), PLANE, PARAMS1, 0)
    depth = np.full((16, 24), 1080, dtype=np.uint16)                  # the plane from z = 0.2325
    lv, ln = T.live_maps(depth, PLANE, PARAMS1)
    assert (lv[:, 3] == 1).all() and np.abs(ln[ln[:, 3] == 1, :3] - np.array([0, 0, -1], dtype=np.float32)).max() <= 1e-6
    assert (ln[:, 3] == 0).sum() == 16 + 24 - 1                        # the last row and column
    J, r = T.icp_rows(lv, ln, mv, mn, committed[:3].reshape(12), committed[:3].reshape(12), PLANE, PARAMS1, 0)
    assert len(r) == 15 * 23 and np.abs(r + 0.0325).max() <= 1e-6 and np.abs(J[:, 3:] - np.array([0, 0, -1], dtype=np.float32)).max() <= 1e-5
    sums, mags = T.icp_sums(J, r)
    assert sums[28] == len(r) and sums[27] > 0 and (mags >= np.abs(sums)).all()
    # all normals are -z: the sums hold the step along the normal, and one Gauss-Newton step along it recovers the offset
    A55, b5 = sums[20], sums[26]
    assert abs(b5 / A55 - 0.0325) <= 1e-6
    assert T.solve(sums, PARAMS1.pivot_floor) is None                  # a plane leaves three freedoms: the factorisation refuses
    st = T.new_state(committed)
    before = st['estimate'].copy()
    assert not T.update(sums, st, 16 * 24, PARAMS1) and np.array_equal(st['estimate'], before) and st['last_pairs'] == len(r)
    assert abs(st['last_rms'] - 0.0325) <= 1e-6 and st['accepted'] == 0 and st['iterations'] == 1
    # the same step along the normal with the other five directions pinned by a unit diagonal: the full solve recovers the offset
    full = np.zeros(T.SUMS)
    for s, (i, j) in enumerate(T.PAIRS):
        full[s] = 1.0 if i == j else 0.0
    full[20], full[26], full[27], full[28] = A55, b5, sums[27], sums[28]
    assert T.update(full, st, 16 * 24, PARAMS1)
    assert np.abs(st['estimate'].reshape(3, 4) - truth[:3]).max() <= 1e-6


def test_a_twist_of_zero_is_the_identity_and_exp_is_a_rigid_motion():
    Rz, tz = T.twist_exp(np.zeros(6))
    assert np.array_equal(Rz, np.eye(3)) and np.array_equal(tz, np.zeros(3))
    sums = np.zeros(T.SUMS)
    for s, (i, j) in enumerate(T.PAIRS):
        sums[s] = 1.0 if i == j else 0.0
    sums[28] = 100
    st = T.new_state(synth.synthetic_poses(1)[0])
    before = st['estimate'].copy()
    assert T.update(sums, st, 400, PARAMS1) and np.abs(st['estimate'] - before).max() <= 4e-16 and st['accepted'] == 1
    for th in (1e-9, 1e-5, 1e-4, 1e-3, 0.1, 1.0):
        xi = np.concatenate([th * np.array([0.6, -0.48, 0.64]), [0.3, -0.2, 0.1]])
        Rm, t = T.twist_exp(xi)
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(Rm) - 1) <= 1e-15
        half, _ = T.twist_exp(0.5 * xi)                              # exp(xi) = exp(xi / 2)^2
        th2, t2 = T.twist_exp(0.5 * xi)
        assert np.abs(half @ half - Rm).max() <= 1e-15 and np.abs(half @ t2 + t2 - t).max() <= 1e-15


def test_a_lost_frame_leaves_the_committed_pose_alone():
    pose = synth.synthetic_poses(2)
    P = T.Params()
    st = T.new_state(pose[0])
    st['estimate'] = pose[1][:3].reshape(12).copy()
    st['last_share'], st['last_rms'], st['last_pairs'], st['iterations'] = 0.0, 0.0, 0.0, 19          # nothing accepted
    row32, row = T.commit(st, P)
    assert np.isnan(row32).all() and row32.dtype == np.float32 and row[12] == 1 and np.isnan(row[:12]).all()
    assert np.array_equal(st['committed'], pose[0][:3].reshape(12)) and np.array_equal(st['estimate'], st['committed'])
    assert (st['lost'], st['frame'], st['accepted'], st['iterations']) == (1, 2, 0, 0) and row[17] == 19
    for change in (dict(last_share=0.05), dict(last_rms=0.05), dict(move=0.5)):
        st = T.new_state(pose[0])
        st.update(last_share=0.7, last_rms=0.002, last_pairs=4000.0, accepted=19, iterations=19)
        if 'move' in change:
            st['estimate'][3] += change['move']
        else:
            st.update(change)
        assert T.commit(st, P)[1][12] == 1 and np.array_equal(st['committed'], pose[0][:3].reshape(12))
    st = T.new_state(pose[0])
    st.update(last_share=0.7, last_rms=0.002, last_pairs=4000.0, accepted=19, iterations=19, estimate=pose[1][:3].reshape(12).copy())
    row32, row = T.commit(st, P)
    assert row[12] == 0 and np.array_equal(st['committed'], pose[1][:3].reshape(12)) and np.array_equal(row32, st['committed'].astype(np.float32))


def test_live_map_pyramid_by_hand():
    S = F.Setup((4, 4, 4), (0, 0, 0), 0.1, fx=4.0, fy=4.0, u=2.5, v=1.5, image_size=(4, 6))
    P = T.Params(levels=2, iterations=(1, 1), pyr_dist=0.1)
    depth = np.array([[1000, 1040, 0, 0, 2000, 0], [1080, 1200, 0, 0, 0, 0], [3000] * 6, [3000] * 6], dtype=np.uint16)
    v, n = T.live_maps(depth, S, P)
    assert v.shape == (24 + 6, 4)
    z1, w1 = v[24:, 2].reshape(2, 3), v[24:, 3].reshape(2, 3)
    assert w1.tolist() == [[1, 0, 1], [1, 1, 1]]
    assert abs(z1[0, 0] - (1.0 + 1.04 + 1.08) / 3) <= 1e-6 and z1[0, 2] == np.float32(2000) * np.float32(0.001)      # 1.2 lies beyond pyr_dist
    assert v[24, 0] == (np.float32(0) - np.float32(1.0)) / np.float32(2.0) * z1[0, 0]                                 # cu_1 = (2.5 - 0.5) / 2, fx_1 = 2
    assert v[0, 0] == np.float32(-2.5) / np.float32(4.0) * np.float32(1.0)


# -- 5. the restatement tracks -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tracked():
    v, c, t = synth.synthetic_scene(3, 8)
    poses = T.sequence_trajectory()
    depth = R.render(v, c, t, poses, T.SEQ_H, T.SEQ_W, 1, R.Camera(**T.SEQ_CAM))['depth']
    trk = T.Tracker(T.sequence_setup(), T.Params())
    trk.start(poses[0], depth[0])
    for k in range(1, len(poses)):
        trk.push(depth[k])
    return poses, depth, trk


def test_the_restatement_tracks_the_sequence(tracked):
    poses, depth, trk = tracked
    step = T.pose_errors(poses[1:], poses[:-1])
    full = T.pose_errors(synth.synthetic_trajectory(12, 3)[1:], synth.synthetic_trajectory(12, 3)[:-1])
    assert step[0].max() < 0.5 * full[0].max() and len(poses) == 12              # slower than synthetic_trajectory
    est, lost, diag = trk.trajectory()
    dt, dr = T.pose_errors(est, poses)
    print('translation error (voxels):', np.round(dt / T.SEQ_VOXEL, 4).tolist())
    print('rotation error (degrees):', np.round(dr, 4).tolist())
    print('worst %.6f voxel, %.6f degrees; accepted pairs %s' % ((dt / T.SEQ_VOXEL).max(), dr.max(), diag[1:, 1].astype(int).tolist()))
    assert not lost.any() and (diag[1:, 4] == 19).all()
    assert (dt / T.SEQ_VOXEL).max() <= 1.5 * RECORDED_VOXELS
    assert dr.max() <= 1.5 * RECORDED_DEGREES
    assert (diag[1:, 2] > 0.5).all() and (diag[1:, 3] < 0.01).all()


def test_a_lost_frame_in_the_restatement_is_kept_out_of_the_volume(tracked):
    poses, depth, _ = tracked
    S, P = T.sequence_setup(), T.Params()
    a, b = T.Tracker(S, P), T.Tracker(S, P)
    a.start(poses[0], depth[0])
    b.start(poses[0], depth[0])
    a.push(depth[1])
    b.push(depth[1])
    row = a.push(np.zeros_like(depth[2]))
    assert row[12] == 1 and row[13] == 0 and row[16] == 0 and a.state['lost'] == 1
    assert np.array_equal(a.tsdf.view(np.uint32), b.tsdf.view(np.uint32)) and np.array_equal(a.state['committed'], b.state['committed'])
    ra, rb = a.push(depth[3]), b.push(depth[3])
    assert ra[12] == 0 and np.array_equal(ra[:12], rb[:12])                      # frame 3 is tracked from frame 1's pose in both
