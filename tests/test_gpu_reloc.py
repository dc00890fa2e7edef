"""The kfn_reloc_* launches on the device against the numpy restatement of tests/reloc_ref.py: the fern code
byte for byte, the search exactly, every branch of the seed / settle state machine field by field, the scenario of
tests/test_reloc_host.py (a loss the plain tracker cannot recover from), repeatability, and `track make --reloc`."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fuse_ref as F
import render_ref as R
import reloc_ref as Q
import track_ref as T
from kfnet_amd import _lib, synth
from kfnet_amd import fuse as M
from kfnet_amd import render
from kfnet_amd import track as K
from kfnet_amd.labels import DepthCamera

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the bound tests/test_gpu_track.py asserts for tracked frames of this scene: twice the restatement's recorded worst errors
RECORDED_VOXELS, RECORDED_DEGREES = 0.111684, 0.085162
ROWS = 32


def _tracker(S, color=False, reloc=None, **kw):
    cam = DepthCamera(S.fx, S.fy, S.u, S.v, scale=S.scale, raw_min=S.raw_min, raw_max=S.raw_max)
    vol = M.Volume(S.dims, S.origin, S.voxel, S.trunc, cam, S.image_size, 1, color, S.max_weight, S.near)
    return K.Tracker(vol, max_frames=ROWS, reloc=reloc, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope='module')
def scene():
    return synth.synthetic_scene(3, 8)


def _render(scene, poses):
    v, c, t = scene
    return R.render(v, c, t, poses, T.SEQ_H, T.SEQ_W, 1, R.Camera(**T.SEQ_CAM))


# -- encode, byte for byte -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def one_frame(scene):
    out = _render(scene, T.sequence_trajectory(1))
    return out['depth'][0], out['frames'][0]


@pytest.mark.parametrize('size', ((64, 96), (50, 70)))
@pytest.mark.parametrize('colour', (False, True))
def test_encode_byte_for_byte(one_frame, size, colour):
    import torch
    H, W = size
    depth, frame = one_frame[0][:H, :W].copy(), np.ascontiguousarray(one_frame[1][:H, :W])
    rng = np.random.default_rng(5)
    depth[rng.random((H, W)) < 0.3] = 0                               # invalid pixels, many under ferns
    depth[8:32, 16:56] = 0                                            # and whole blocks of level 2
    S = F.Setup((8, 8, 8), (0, 0, 0), 0.1, fx=78.75, fy=80.0, u=W / 2.0 - 0.25, v=H / 2.0, image_size=size)
    trk = _tracker(S, color=colour, reloc=dict(ferns=500, keyframes=4, depth_range=(1.0, 3.5)))
    rc = trk.reloc
    Hl, Wl, _ = trk.sizes[2]
    assert (Hl, Wl) == (H // 4, W // 4) and (size != (50, 70) or (Hl * 4 < H and Wl * 4 < W))     # floor halving drops a row and a column
    table = rc.table_host.copy()
    table[:8, 0] = (-1, Wl, 0, 0, 1 << 30, -(1 << 31), Wl - 1, 0)    # positions out of range beside the last ones in range
    table[:8, 1] = (0, 0, -1, Hl, 0, 0, Hl - 1, 1 << 30)
    rc.table.copy_(torch.from_numpy(table))
    trk._stage(depth, frame if colour else None)
    trk.live_maps()
    rc.code.fill_(255)
    rc.encode()
    got = rc.code.cpu().numpy()
    live_v, _ = T.live_maps(depth, S, T.Params())
    want = Q.encode(table, live_v, frame if colour else None, size, 2)
    under = live_v[trk.sizes[2][2]:][table[8:, 1] * Wl + table[8:, 0], 3]
    assert (under == 0).sum() > 20 and (under == 1).sum() > 200                    # ferns over invalid and over valid vertices
    assert not want[[0, 1, 2, 3, 4, 5, 7]].any() and (want & 1).sum() > 50 and ((want & 1) == 0).sum() > 50
    if colour:
        assert all(((want >> b) & 1).sum() > 50 and ((want >> b) & 1).sum() < 450 for b in (1, 2, 3))
    else:
        assert want.max() == 1
    assert np.array_equal(got, want), (np.flatnonzero(got != want)[:10], got[got != want][:10], want[got != want][:10])


# -- search, exactly ------------------------------------------------------------------------------------------------------------------------
def _reloc_state(**fields):
    st = _lib.RelocState()
    for k, v in fields.items():
        if k in ('anchor', 'cand_d', 'cand_index'):
            v = type(getattr(st, k))(*v)
        setattr(st, k, v)
    return st


def _ref_state(st):
    return dict(anchor=np.array(st.anchor), n=st.n, streak=st.streak, seeded=st.seeded, seed_key=st.seed_key, candidates=st.candidates,
                min_d=st.min_d, recovered=st.recovered, reserved=st.reserved, cand_d=list(st.cand_d), cand_index=list(st.cand_index))


def _same_state(dev, ref, what):
    got = _ref_state(dev)
    for k in ref:
        assert np.array_equal(np.asarray(got[k]), np.asarray(ref[k]), equal_nan=True), (what, k, got[k], ref[k])


@pytest.mark.parametrize('ferns', (1, 500))
def test_search_exactly(ferns):
    import torch
    S = F.Setup((8, 8, 8), (0, 0, 0), 0.1, image_size=(16, 24))
    rng = np.random.default_rng(ferns)
    for tries in (3, 4):
        trk = _tracker(S, reloc=dict(ferns=ferns, keyframes=64, tries=tries, level=0))
        rc = trk.reloc
        P = Q.Params(ferns=ferns, capacity=64, tries=tries)
        codes = rng.integers(0, 16 if ferns > 1 else 2, size=(64, ferns)).astype(np.uint8)
        code = rng.integers(0, 16 if ferns > 1 else 2, size=ferns).astype(np.uint8)
        near = np.tile(code, (64, 1))                                 # few ferns differ, so that distances tie
        flip = rng.random((64, ferns)) < 0.02
        near[flip] ^= 1
        near[[5, 9, 40]] = code                                       # duplicated codes at distance 0: the lower index comes first
        for name, store in (('random', codes), ('near', near)):
            rc.codes.copy_(torch.from_numpy(store))
            rc.code.copy_(torch.from_numpy(code))
            for n in (0, 1, 2, 63, 64, 99, -4):
                start = _reloc_state(n=n, streak=2, recovered=5, candidates=77, min_d=-3, cand_d=(9, 9, 9, 9), cand_index=(8, 8, 8, 8))
                rc.set_state(start)
                rc.dist.fill_(-7)
                rc.search()
                ref = _ref_state(start)
                Q.search(ref, code, store, P)
                _same_state(rc.state(), ref, (name, tries, n))
                dist = rc.dist.cpu().numpy()
                m = min(max(n, 0), 64)
                assert np.array_equal(dist[:m], (store[:m] != code).sum(axis=1)) and (dist[m:] == -7).all(), (name, n)     # slots >= n exit
                if name == 'near' and n == 64:                        # the ties are there, in index order
                    assert ref['cand_d'][:3] == [0, 0, 0] and ref['cand_index'][:3] == sorted(ref['cand_index'][:3])
                    assert ferns == 1 or ref['cand_index'][:3] == [5, 9, 40]


# -- seed and settle: every branch, field by field ----------------------------------------------------------------------------------------------
FERNS, CAP = 70, 4                                                    # more ferns than lanes: the copy of the code strides


def _track_state(committed, estimate, share, rms, frame, lost):
    st = K.pose_record(committed, estimate, frame)
    st.last_share, st.last_rms, st.last_pairs, st.lost = share, rms, 321.0, lost
    return st


def _ref_track(st):
    return dict(committed=np.array(st.committed), estimate=np.array(st.estimate), last_share=st.last_share, last_rms=st.last_rms,
                last_pairs=st.last_pairs, frame=st.frame, lost=st.lost, accepted=st.accepted, iterations=st.iterations)


def _pose(k):
    return synth.synthetic_poses(8)[k][:3].reshape(12).copy()


BRANCHES = {
    # name: (reloc record, tracked by the commit, last_share, last_rms, first, the frame of the record)
    'tracked_harvest': (dict(n=2, min_d=15, candidates=2, cand_index=(1, 0, -1, -1), cand_d=(15, 20, 71, 71)), True, 0.7, 0.002, 0, 6),
    'tracked_near': (dict(n=2, min_d=14, candidates=2, cand_index=(1, 0, -1, -1), cand_d=(14, 20, 71, 71)), True, 0.7, 0.002, 0, 6),
    'tracked_full': (dict(n=4, min_d=60, candidates=3, cand_index=(3, 0, 1, -1), cand_d=(60, 61, 62, 71)), True, 0.7, 0.002, 0, 6),
    'tracked_ends_streak': (dict(n=2, streak=3, min_d=15, candidates=2, cand_index=(1, 0, -1, -1)), True, 0.7, 0.002, 0, 6),
    'first': (dict(n=0, min_d=71, candidates=0, cand_index=(-1,) * 4, seeded=1, streak=2), True, 0.0, 0.0, 1, 1),
    'lost_begins': (dict(n=2, min_d=3, candidates=2, cand_index=(0, 1, -1, -1)), False, 0.0, 0.0, 0, 6),
    'lost_goes_on': (dict(n=2, streak=4, min_d=3, candidates=2, cand_index=(0, 1, -1, -1)), False, 0.0, 0.0, 0, 6),
    'lost_seeded': (dict(n=2, streak=4, seeded=1, seed_key=1, min_d=3, candidates=2, cand_index=(0, 1, -1, -1)), False, 0.05, 0.001, 0, 6),
    'recovered': (dict(n=2, streak=4, seeded=1, seed_key=0, recovered=2, min_d=30, candidates=2, cand_index=(0, 1, -1, -1)), True, 0.7, 0.002, 0, 6),
    'demoted_share': (dict(n=2, streak=1, seeded=1, seed_key=0, min_d=30, candidates=2, cand_index=(0, 1, -1, -1)), True, 0.19, 0.002, 0, 6),
    'demoted_rms': (dict(n=2, streak=1, seeded=1, seed_key=1, min_d=30, candidates=2, cand_index=(0, 1, -1, -1)), True, 0.7, 0.031, 0, 6),
    'garbage': (dict(n=1 << 30, streak=-5, seeded=7, seed_key=1 << 29, min_d=-9, candidates=1 << 28, cand_index=(1 << 27, -3, 9, 9)), True, 0.7,
                0.002, 0, 6),
    'row_beyond': (dict(n=2, min_d=15, candidates=2, cand_index=(1, 0, -1, -1)), True, 0.7, 0.002, 0, 1 << 20),
    'row_negative': (dict(n=2, min_d=15, candidates=2, cand_index=(1, 0, -1, -1)), True, 0.7, 0.002, 0, -(1 << 30)),
}


@pytest.fixture(scope='module')
def machine():
    S = F.Setup((8, 8, 8), (0, 0, 0), 0.1, image_size=(16, 24))
    # the verification gates are stricter than the tracker's here, so that a frame the commit tracked can fail them
    return _tracker(S, reloc=dict(ferns=FERNS, keyframes=CAP, tries=3, harvest_share=0.2, level=0, min_share=0.2, max_rms=0.03))


@pytest.mark.parametrize('name', sorted(BRANCHES))
def test_settle_branches(machine, name):
    import torch
    trk, rc = machine, machine.reloc
    fields, tracked, share, rms, first, frame = BRANCHES[name]
    P = Q.Params(ferns=FERNS, capacity=CAP, tries=3, harvest_share=0.2, rows=ROWS, traj_rows=ROWS, min_share=0.2, max_rms=0.03)
    assert P.harvest == 14 and rc.harvest == 14
    rng = np.random.default_rng(3)
    code, codes = rng.integers(0, 2, size=FERNS).astype(np.uint8), rng.integers(0, 2, size=(CAP, FERNS)).astype(np.uint8)
    key_poses = np.stack([_pose(k) for k in range(CAP)])
    rstate = _reloc_state(anchor=_pose(5), **fields)
    committed = _pose(6)
    tstate = _track_state(committed, committed if tracked else _pose(7), share, rms, frame, 3)
    trajectory = rng.normal(size=(ROWS, 20))
    if 0 <= frame - 1 < ROWS:
        trajectory[frame - 1, :12], trajectory[frame - 1, 12] = (committed, 0.0) if tracked else (np.nan, 1.0)
    pose_rows = committed.astype(np.float32) if tracked else np.full(12, np.nan, dtype=np.float32)
    rows = rng.integers(-50, 50, size=(ROWS, 8)).astype(np.int32)
    # the device
    rc.set_state(rstate)
    trk.record.copy_(torch.frombuffer(bytearray(bytes(tstate)), dtype=torch.int64))
    rc.code.copy_(torch.from_numpy(code))
    rc.codes.copy_(torch.from_numpy(codes))
    rc.key_poses.copy_(torch.from_numpy(key_poses))
    trk.trajectory_rows.copy_(torch.from_numpy(trajectory))
    trk.vol.poses[0].copy_(torch.from_numpy(pose_rows))
    rc.rows.copy_(torch.from_numpy(rows))
    rc.settle(first=bool(first))
    # the restatement
    rs, ts = _ref_state(rstate), _ref_track(tstate)
    Q.settle(rs, ts, code, codes, key_poses, pose_rows, trajectory, rows, P, first=bool(first))
    _same_state(rc.state(), rs, name)
    got = _ref_track(trk.state())
    for k in ts:
        assert np.array_equal(np.asarray(got[k]), np.asarray(ts[k]), equal_nan=True), (name, k, got[k], ts[k])
    for what, dev, ref in (('codes', rc.codes, codes), ('key_poses', rc.key_poses, key_poses), ('trajectory', trk.trajectory_rows, trajectory),
                           ('pose row', trk.vol.poses[0], pose_rows), ('rows', rc.rows, rows)):
        assert np.array_equal(dev.cpu().numpy(), ref, equal_nan=True), (name, what)
    # what each branch must have done, on the restatement (the device equals it)
    row = rows[frame - 1].tolist() if 0 <= frame - 1 < ROWS else None
    if name == 'tracked_harvest':
        assert row == [15, 1, -1, 2, 0, 2, 0, 0] and rs['n'] == 3 and np.array_equal(codes[2], code) and np.array_equal(key_poses[2], committed)
    if name in ('tracked_near', 'tracked_full'):
        assert row[3] == -1 and rs['n'] == fields['n'] and rs['streak'] == 0
    if name == 'first':
        assert row == [71, -1, -1, 0, 0, 0, 0, 0] and rs['n'] == 1 and rs['streak'] == 0 and rs['seeded'] == 0
    if name == 'lost_begins':
        assert row[4] == 1 and np.array_equal(rs['anchor'], committed)
    if name == 'lost_seeded':
        assert row[2:5] == [1, -1, 5] and np.array_equal(ts['committed'], _pose(5)) and np.array_equal(ts['estimate'], _pose(5))
    if name == 'recovered':
        assert row[2:7] == [0, -1, 0, 2, 0] and rs['recovered'] == 3 and np.array_equal(ts['committed'], committed) and rs['n'] == 2
    if name.startswith('demoted'):
        assert row[4:7] == [2, 2, 1] and ts['lost'] == 4 and np.isnan(pose_rows).all() and np.isnan(trajectory[5, :12]).all()
        assert trajectory[5, 12] == 1 and np.array_equal(ts['committed'], _pose(5))
    if name == 'garbage':
        assert rs['n'] == CAP and row[5] == 3 and row[6] == 0 and rs['streak'] == 0
    if name.startswith('row_'):
        assert row is None and rs['streak'] == 1 and rs['n'] == 2                       # no row to read: the frame counts as lost


SEEDS = {
    'acts': (dict(n=3, streak=2, candidates=3, cand_index=(2, 0, 1, -1)), 0),
    'wraps': (dict(n=3, streak=7, candidates=2, cand_index=(2, 1, 0, -1)), 2),
    'not_lost': (dict(n=3, streak=0, candidates=3, cand_index=(2, 0, 1, -1)), None),
    'no_keyframes': (dict(n=0, streak=2, candidates=0, cand_index=(-1,) * 4), None),
    'candidates_clamped': (dict(n=1, streak=2, candidates=3, cand_index=(0, 3, 3, 3)), 0),
    'index_beyond_n': (dict(n=2, streak=1, candidates=2, cand_index=(2, 0, -1, -1)), None),
    'index_negative': (dict(n=2, streak=1, candidates=2, cand_index=(-1, 0, -1, -1)), None),
    'garbage': (dict(n=-(1 << 30), streak=1 << 30, candidates=1 << 30, cand_index=(1 << 30,) * 4), None),
    'garbage_n': (dict(n=1 << 30, streak=2, candidates=1 << 30, cand_index=(0, 1 << 20, 0, 0)), None),
}


@pytest.mark.parametrize('name', sorted(SEEDS))
def test_seed_branches(machine, name):
    import torch
    trk, rc = machine, machine.reloc
    fields, key = SEEDS[name]
    P = Q.Params(ferns=FERNS, capacity=CAP, tries=3)
    key_poses = np.stack([_pose(k) for k in range(CAP)])
    rstate, tstate = _reloc_state(anchor=_pose(5), **fields), _track_state(_pose(6), _pose(7), 0.5, 0.01, 4, 1)
    rc.set_state(rstate)
    trk.record.copy_(torch.frombuffer(bytearray(bytes(tstate)), dtype=torch.int64))
    rc.key_poses.copy_(torch.from_numpy(key_poses))
    rc.seed()
    rs, ts = _ref_state(rstate), _ref_track(tstate)
    Q.seed(rs, ts, key_poses, P)
    _same_state(rc.state(), rs, name)
    got = _ref_track(trk.state())
    for k in ts:
        assert np.array_equal(np.asarray(got[k]), np.asarray(ts[k])), (name, k)
    if key is None:
        assert rs['seeded'] == 0 and np.array_equal(ts['committed'], _pose(6)) and np.array_equal(ts['estimate'], _pose(7))
    else:
        assert rs['seeded'] == 1 and rs['seed_key'] == key and np.array_equal(ts['committed'], key_poses[key])
        assert np.array_equal(ts['estimate'], key_poses[key])


# -- the scenario on the device ---------------------------------------------------------------------------------------------------------------
SCENARIO_RELOC = dict(ferns=Q.SCENARIO_FERNS, keyframes=Q.SCENARIO_KEYFRAMES, harvest_share=Q.SCENARIO_HARVEST_SHARE, tries=Q.SCENARIO_TRIES,
                      seed=Q.SCENARIO_SEED)


def _run(depth, first, reloc):
    trk = _tracker(T.sequence_setup(), reloc=reloc)
    trk.start(first, depth[0])
    for k in range(1, len(depth)):
        trk.push(depth[k])
    return trk


@pytest.fixture(scope='module')
def scenario(scene):
    import torch
    poses, phase = Q.scenario_poses()
    depth = Q.scenario_depth(lambda p: _render(scene, p)['depth'], poses, phase)
    P = Q.scenario_params(ROWS)
    ref = Q.run_scenario(depth, poses[0], P, K.fern_table(Q.SCENARIO_SEED, P.ferns, (16, 24)))
    trk = _run(depth, poses[0], SCENARIO_RELOC)
    out = trk.trajectory(), trk.relocalisation()
    torch.cuda.synchronize()
    return poses, phase, depth, ref, trk, out


def test_the_scenario_equals_the_restatement(scenario):
    poses, phase, depth, ref, trk, ((est, lost, diag), (rows, count, key_poses)) = scenario
    rest, rlost, rdiag = ref.trajectory()
    rrows, rcount, rkeys = ref.relocalisation()
    print('lost', lost.astype(int).tolist())
    print('rows', rows[:, :7].tolist())
    assert np.array_equal(lost, rlost)
    assert np.array_equal(rows, rrows), (rows.tolist(), rrows.tolist())              # distances, keyframe indices, seeds, streaks
    assert count == rcount >= 3 and np.array_equal(diag[:, [0, 4, 5]], rdiag[:, [0, 4, 5]])
    a, b, c = (np.array([p == x for p in phase]) for x in 'ABC')
    assert not lost[a].any() and lost[b].all() and lost[c].sum() <= Q.SCENARIO_TRIES and not lost[np.flatnonzero(c)[0] + Q.SCENARIO_TRIES:].any()
    assert (rows[c, 2] >= 0).any() and trk.reloc.state().recovered == 1 and trk.state().lost == lost.sum()
    keep = ~lost
    dt, dr = T.pose_errors(est[keep], poses[keep])
    against = T.pose_errors(est[keep], rest[keep])
    kd, kr = T.pose_errors(key_poses, np.stack([T.pose_of(k) for k in rkeys]))
    print('worst %.4f voxel, %.4f degrees; against the restatement %.3g voxel, %.3g degrees; keyframes %.3g voxel' %
          ((dt / T.SEQ_VOXEL).max(), dr.max(), against[0].max() / T.SEQ_VOXEL, against[1].max(), kd.max() / T.SEQ_VOXEL))
    assert (dt / T.SEQ_VOXEL).max() <= 2 * RECORDED_VOXELS and dr.max() <= 2 * RECORDED_DEGREES
    assert np.isnan(est[lost][:, :3]).all()
    # a keyframe's pose is the pose reported for the frame that became it, bit for bit
    for k in np.flatnonzero(rows[:, 3] >= 0):
        assert np.array_equal(key_poses[rows[k, 3]].view(np.uint64), est[k].view(np.uint64)), k


def test_without_the_relocaliser_everything_after_phase_a_is_lost(scenario):
    poses, phase, depth, ref, _, _ = scenario
    trk = _run(depth, poses[0], None)
    assert trk.reloc is None
    est, lost, diag = trk.trajectory()
    print('lost', lost.astype(int).tolist())
    assert lost.tolist() == [p != 'A' for p in phase]
    with pytest.raises(ValueError):
        trk.relocalisation()


def test_no_lost_frame_reached_the_volume(scenario):
    import torch
    poses, phase, depth, ref, trk, ((est, lost, diag), _) = scenario
    other = _tracker(T.sequence_setup())
    for k in np.flatnonzero(~lost):
        other._stage(depth[k], None)
        row = K.pose_rows(est[k][None]) if k == 0 else est[k][:3].reshape(1, 12).astype(np.float32)
        other.vol.poses[:1].copy_(torch.from_numpy(row))
        other.integrate()
    torch.cuda.synchronize()
    assert lost.sum() >= 2 and np.array_equal(_bits(trk.vol.tsdf()), _bits(other.vol.tsdf()))


def test_two_runs_give_the_same_bits(scenario):
    poses, phase, depth, ref, trk, ((est, lost, diag), (rows, count, key_poses)) = scenario
    again = _run(depth, poses[0], SCENARIO_RELOC)
    est2, lost2, diag2 = again.trajectory()
    rows2, count2, key_poses2 = again.relocalisation()
    assert np.array_equal(est.view(np.uint64), est2.view(np.uint64)) and np.array_equal(diag.view(np.uint64), diag2.view(np.uint64))
    assert np.array_equal(rows, rows2) and count == count2 and np.array_equal(key_poses.view(np.uint64), key_poses2.view(np.uint64))
    assert np.array_equal(trk.reloc.codes.cpu().numpy(), again.reloc.codes.cpu().numpy())
    assert bytes(trk.reloc.state()) == bytes(again.reloc.state())
    assert np.array_equal(_bits(trk.vol.tsdf()), _bits(again.vol.tsdf()))


# -- the program --------------------------------------------------------------------------------------------------------------------------------
def test_track_make_with_reloc(scene, scenario, tmp_path):
    from kfnet_amd.KFNet.pnp import write_pose
    from kfnet_amd.tools.io import read_lines
    poses, phase, depth, ref, _, ((est, lost, diag), (rows, count, _)) = scenario
    seq, out = tmp_path / 'seq-01', tmp_path / 'tracked'
    seq.mkdir()
    grey = np.zeros((T.SEQ_H, T.SEQ_W, 3), dtype=np.uint8)
    for k in range(len(depth)):
        render.write_png(str(seq / ('frame-%06d.color.png' % k)), grey)
        render.write_png(str(seq / ('frame-%06d.depth.png' % k)), depth[k])
    write_pose(str(tmp_path / 'first.txt'), poses[0])
    flags = ['--focal_x', repr(T.SEQ_CAM['fx']), '--focal_y', repr(T.SEQ_CAM['fy']), '--u', repr(T.SEQ_CAM['u']), '--v', repr(T.SEQ_CAM['v']),
             '--height', str(T.SEQ_H), '--width', str(T.SEQ_W), '--no_color']
    bounds = ['--bounds', '-0.1', '-0.1', '-0.1', '4.1', '3.1', '2.6', '--voxel', repr(T.SEQ_VOXEL)]
    reloc = ['--reloc', '--reloc_harvest', repr(Q.SCENARIO_HARVEST_SHARE), '--reloc_keyframes', str(Q.SCENARIO_KEYFRAMES)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'kfnet_amd.track', 'make', '--sequence', str(seq), '--output_folder', str(out), '--first_pose',
                        str(tmp_path / 'first.txt')] + bounds + flags + reloc, cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    n, tracked = len(depth), int((~lost).sum())
    last = r.stdout.strip().split('\n')[-1]
    assert last.startswith('%d frames, %d tracked, %d lost; ' % (n, tracked, n - tracked)) and last.endswith('; %d keyframes, 1 relocalised' % count), last
    names = [[os.path.basename(x) for x in read_lines(str(out / name)) if x] for name in ('depth_list.txt', 'pose_list.txt')]
    keep = np.flatnonzero(~lost)
    assert names[0] == ['frame-%06d.depth.png' % k for k in keep] and names[1] == ['frame-%06d.pose.txt' % k for k in keep]
    report = [x.split() for x in read_lines(str(out / 'track_report.txt')) if x][1:]
    want = ['lost' if lost[k] else ('relocalised' if rows[k, 2] >= 0 else 'tracked') for k in range(n)]
    assert [w[1] for w in report] == want and want.count('relocalised') == 1
    rel = [x.split() for x in read_lines(str(out / 'reloc_report.txt')) if x]
    assert rel[0] == ['#', 'frame', 'nearest', 'distance', 'seeded_key', 'keyframe_added', 'streak'] and len(rel) == n + 1
    assert [[int(v) for v in w[1:]] for w in rel[1:]] == rows[:, [1, 0, 2, 3, 4]].tolist()
