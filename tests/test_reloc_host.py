"""Relocalisation from fern-coded keyframes, the host side: the fern table, the exports and their refusals
without a device, Relocaliser's own refusals, hand cases of the numpy restatement (tests/reloc_ref.py), the scenario's
conditions on the restated trackers, and the files `track make --reloc` writes.  Nothing here needs a device."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import render_ref as R
import reloc_ref as Q
import track_ref as T
from kfnet_amd import _lib, synth
from kfnet_amd import track as M
from kfnet_amd.labels import read_frames
from test_track_host import _header_struct, _touch_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the bound tests/test_gpu_track.py asserts for tracked frames of this scene: twice the restatement's recorded worst errors
RECORDED_VOXELS, RECORDED_DEGREES = 0.111684, 0.085162


# -- 1. the exports, the structs, the fern table ------------------------------------------------------------------------------------------
def test_exports_structs_and_build_entry():
    lib = _lib.load()
    assert lib.kfn_abi_version() == 13
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ('kfn_reloc_encode', 'kfn_reloc_search', 'kfn_reloc_seed', 'kfn_reloc_settle'):
        assert name in _lib.SYMBOLS and getattr(raw, name) is not None
    hdr = open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()
    for text in ('kfn_reloc_encode:', 'kfn_reloc_search:', 'kfn_reloc_seed (one wave', 'kfn_reloc_settle (one wave', 'tests it before any use',
                 'a record of garbage cannot cause an access out of range'):
        assert text in hdr, text
    assert C.sizeof(_lib.RelocDesc) == 64 and C.sizeof(_lib.RelocState) == 160
    assert C.sizeof(_lib.TrackDesc) == 140 and C.sizeof(_lib.TrackState) == 232                 # unchanged
    kinds = {C.c_int32: 'int32_t', C.c_float: 'float', C.c_double: 'double'}
    assert [(n, kinds[t]) for n, t in _lib.RelocDesc._fields_] == [(n, k) for n, k, _ in _header_struct('kfn_reloc_desc')]
    got = [(n, getattr(t, '_length_', 1)) for n, t in _lib.RelocState._fields_]
    want = [(n, int(full.split('[')[1][:-1]) if '[' in full else 1) for n, k, full in _header_struct('kfn_reloc_state')]
    assert got == want
    from kfnet_amd import build
    assert build.EXTRA['kfn_reloc.hip'] == ['-ffp-contract=off'] and 'kfn_reloc.hip' in build.sources()


def test_fern_table_is_deterministic_and_in_range():
    a, b = M.fern_table(1, 500, (16, 24), True), M.fern_table(1, 500, (16, 24), True)
    assert a.dtype == np.int32 and a.shape == (500, 4) and np.array_equal(a, b)
    assert not np.array_equal(a, M.fern_table(2, 500, (16, 24), True))
    assert a[:, 0].min() >= 0 and a[:, 0].max() <= 23 and a[:, 1].min() >= 0 and a[:, 1].max() <= 15
    assert len(np.unique(a[:, 0])) == 24 and len(np.unique(a[:, 1])) == 16
    thr = a[:, 2].copy().view(np.float32)
    assert thr.min() >= 0.5 and thr.max() <= 4.0 and thr.max() - thr.min() > 3.0
    assert (a[:, 3] >= 0).all() and (a[:, 3] < 1 << 24).all() and len(np.unique(a[:, 3] & 255)) > 100
    plain = M.fern_table(1, 500, (16, 24), False)
    assert np.array_equal(plain[:, :3], a[:, :3]) and not plain[:, 3].any()            # colour changes the last column alone
    narrow = M.fern_table(5, 64, (120, 160), False, 1.0, 1.0)[:, 2].copy().view(np.float32)
    assert (narrow == 1.0).all()
    for kw in (dict(ferns=0), dict(ferns=4097), dict(level_size=(0, 4)), dict(depth_lo=0.0), dict(depth_lo=2.0, depth_hi=1.0)):
        args = dict(seed=1, ferns=8, level_size=(4, 4), colour=False, depth_lo=0.5, depth_hi=4.0)
        args.update(kw)
        with pytest.raises(ValueError):
            M.fern_table(**args)


# -- 2. the refusals of every export, without a device -------------------------------------------------------------------------------------
A16 = 0x1000


def _desc(**change):
    kw = dict(H=64, W=96, levels=3, reloc_level=2, ferns=500, capacity=64, tries=3, harvest=100, rows=16, traj_rows=16, slot=0, first=0,
              colour=0, reloc_min_share=0.1, reloc_max_rms=0.04)
    kw.update(change)
    size = kw.pop('struct_size', None)
    floats = dict((k, kw.pop(k)) for k in ('reloc_min_share', 'reloc_max_rms'))
    d = _lib.RelocDesc(**kw)
    d.reloc_min_share, d.reloc_max_rms = floats['reloc_min_share'], floats['reloc_max_rms']
    if size is not None:
        d.struct_size = size
    return d


# name: (pointers, the alignment each needs, the call); encode's frame is apart
def _calls(lib):
    return {
        'encode': (3, (16, 16, 1), lambda d, p: lib.kfn_reloc_encode(C.byref(d), p[0], p[1], A16 if d.colour else None, p[2], None)),
        'search': (4, (1, 1, 8, 4), lambda d, p: lib.kfn_reloc_search(C.byref(d), p[0], p[1], p[2], p[3], None)),
        'seed': (3, (8, 8, 8), lambda d, p: lib.kfn_reloc_seed(C.byref(d), p[0], p[1], p[2], None)),
        'settle': (8, (8, 8, 1, 1, 8, 4, 8, 4), lambda d, p: lib.kfn_reloc_settle(C.byref(d), *(list(p) + [None]))),
    }


def test_argument_checks_of_every_export():
    lib = _lib.load()
    msg = lambda: lib.kfn_last_error().decode()
    common = ((dict(struct_size=60), 'struct_size'), (dict(H=0), 'image size'), (dict(W=-3), 'image size'), (dict(levels=0), 'levels'),
              (dict(levels=5), 'levels'), (dict(H=4), 'below 2x2'), (dict(reloc_level=3), 'reloc_level'), (dict(reloc_level=-1), 'reloc_level'),
              (dict(ferns=0), 'ferns'), (dict(ferns=4097), 'ferns'), (dict(capacity=0), 'capacity'), (dict(capacity=65537), 'capacity'),
              (dict(tries=0), 'tries'), (dict(tries=5), 'tries'), (dict(rows=0), 'rows'), (dict(harvest=-1), 'harvest'),
              (dict(harvest=501), 'harvest'), (dict(colour=2), 'colour'))
    own = {'encode': (), 'search': (), 'seed': (),
           'settle': ((dict(slot=-1), 'slot'), (dict(slot=65535), 'slot'), (dict(traj_rows=0), 'traj_rows'), (dict(first=2), 'first'),
                      (dict(reloc_min_share=1.5), 'reloc_min_share'), (dict(reloc_min_share=-0.1), 'reloc_min_share'),
                      (dict(reloc_max_rms=0.0), 'reloc_max_rms'), (dict(reloc_max_rms=float('inf')), 'reloc_max_rms'),
                      (dict(reloc_max_rms=float('nan')), 'reloc_max_rms'))}
    for name, (n, align, call) in _calls(lib).items():
        for change, word in common + own[name]:
            assert call(_desc(**change), (A16,) * n) == -1 and word in msg(), (name, change, msg())
        for k in range(n):                                   # every buffer: NULL, then misaligned where it has an alignment
            assert call(_desc(), tuple(None if j == k else A16 for j in range(n))) == -1 and 'null' in msg(), (name, k, msg())
            if align[k] > 1:
                bad = call(_desc(), tuple(A16 + align[k] // 2 if j == k else A16 for j in range(n)))
                assert bad == -1 and 'aligned' in msg(), (name, k, msg())
    # a colour table without a frame, and a frame without a colour table
    assert lib.kfn_reloc_encode(C.byref(_desc(colour=1)), A16, A16, None, A16, None) == -1 and 'both or neither' in msg()
    assert lib.kfn_reloc_encode(C.byref(_desc(colour=0)), A16, A16, A16, A16, None) == -1 and 'both or neither' in msg()
    assert lib.kfn_reloc_seed(None, A16, A16, A16, None) == -1 and 'null descriptor' in msg()


def _fake_tracker(started=False):
    gate = types.SimpleNamespace(min_share=0.1, max_rms=0.04)
    return types.SimpleNamespace(torch=None, first=np.eye(4) if started else None, levels=3, desc=[gate], max_frames=8)


def test_relocaliser_refusals_before_a_device():
    for kw, word in ((dict(ferns=0), 'ferns'), (dict(ferns=4097), 'ferns'), (dict(keyframes=0), 'keyframes'), (dict(keyframes=65537), 'keyframes'),
                     (dict(tries=0), 'tries'), (dict(tries=5), 'tries'), (dict(level=3), 'level'), (dict(level=-1), 'level'),
                     (dict(harvest_share=-0.1), 'harvest_share'), (dict(harvest_share=1.5), 'harvest_share'),
                     (dict(min_share=2.0), 'min_share'), (dict(max_rms=0.0), 'max_rms'), (dict(max_rms=float('inf')), 'max_rms')):
        with pytest.raises(ValueError) as e:
            M.Relocaliser(_fake_tracker(), **kw)
        assert word in str(e.value), (kw, str(e.value))
    with pytest.raises(ValueError) as e:
        M.Relocaliser(_fake_tracker(started=True))
    assert 'before start()' in str(e.value)
    ap = M.build_parser()
    a = ap.parse_args(['make', '--reloc', '--reloc_ferns', '300', '--reloc_keyframes', '50', '--reloc_harvest', '0.1', '--reloc_tries', '2',
                       '--reloc_seed', '7', '--reloc_min_share', '0.2', '--reloc_max_rms', '0.03'])
    assert (a.reloc, a.reloc_ferns, a.reloc_keyframes, a.reloc_harvest, a.reloc_tries, a.reloc_seed, a.reloc_min_share, a.reloc_max_rms) == \
        (True, 300, 50, 0.1, 2, 7, 0.2, 0.03)
    b = ap.parse_args(['make'])
    assert (b.reloc, b.reloc_ferns, b.reloc_keyframes, b.reloc_harvest, b.reloc_tries, b.reloc_seed, b.reloc_min_share, b.reloc_max_rms) == \
        (False, 500, 1024, 0.2, 3, 1, None, None)


# -- 3. hand cases of the restatement -------------------------------------------------------------------------------------------------------
def test_encode_by_hand():
    live = np.zeros((8 * 12 + 4 * 6 + 2 * 3, 4), dtype=np.float32)
    off = 8 * 12 + 4 * 6
    live[off + 0] = (0, 0, 2.0, 1)                              # (0, 0) at level 2
    live[off + 1 * 3 + 2] = (0, 0, 1.0, 1)                      # (2, 1)
    bits = lambda z: int(np.array([z], dtype=np.float32).view(np.int32)[0])
    table = np.array([[0, 0, bits(1.5), 0], [0, 0, bits(2.0), 0], [2, 1, bits(0.5), 0], [1, 0, bits(0.5), 0], [3, 0, bits(0.5), 0],
                      [0, 2, bits(0.5), 0], [-1, 0, bits(0.5), 0], [0, 0, bits(1.5), 100 + 256 * 101 + 65536 * 99]], dtype=np.int32)
    assert Q.encode(table, live, None, (8, 12), 2).tolist() == [1, 0, 1, 0, 0, 0, 0, 1]   # z > thr strictly; invalid; three out of range
    frame = np.full((8, 12, 3), 100, dtype=np.uint8)
    frame[0, 0] = (101, 101, 101)                               # sums 1601: above 100 x 16 and 99 x 16, not above 101 x 16
    assert Q.encode(table, live, frame, (8, 12), 2).tolist() == [1 | 14, 0 | 14, 1 | 14, 0 | 14, 0, 0, 0, 1 | 2 | 8]


def test_search_ties_empty_short_and_full():
    P = Q.Params(ferns=6, capacity=5, tries=3)
    codes = np.array([[1, 1, 1, 0, 0, 0], [0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0]], dtype=np.uint8)
    code = np.zeros(6, dtype=np.uint8)
    rs = Q.new_state()
    Q.search(rs, code, codes, P)                                # n = 0
    assert (rs['candidates'], rs['min_d'], rs['cand_d'], rs['cand_index']) == (0, 7, [7] * 4, [-1] * 4)
    rs['n'] = 2                                                 # n < tries
    Q.search(rs, code, codes, P)
    assert (rs['candidates'], rs['min_d'], rs['cand_d'], rs['cand_index']) == (2, 1, [1, 3, 7, 7], [1, 0, -1, -1])
    rs['n'] = 5                                                 # a full store, ties by the lower index
    Q.search(rs, code, codes, P)
    assert (rs['candidates'], rs['min_d'], rs['cand_d'], rs['cand_index']) == (3, 0, [0, 1, 1, 7], [2, 1, 3, -1])
    rs['n'] = 99                                                # clamped to the capacity
    Q.search(rs, code, codes, P)
    assert rs['cand_index'] == [2, 1, 3, -1] and rs['candidates'] == 3
    P4 = Q.Params(ferns=6, capacity=5, tries=4)
    Q.search(rs, code, codes, P4)
    assert rs['cand_d'] == [0, 1, 1, 1] and rs['cand_index'] == [2, 1, 3, 4]


def _machine(P):
    ts = T.new_state(synth.synthetic_poses(1)[0])
    return dict(rs=Q.new_state(), ts=ts, codes=np.zeros((P.capacity, P.ferns), dtype=np.uint8), key_poses=np.zeros((P.capacity, 12)),
                pose_row=np.zeros(12, dtype=np.float32), trajectory=np.zeros((P.traj_rows, 20)), rows=np.zeros((P.rows, 8), dtype=np.int32))


def _frame(m, P, code, pose, tracked, share=0.7, rms=0.002, first=False):
    """One frame of the machine without ICP: search, seed, a commit that tracks under `pose` or loses, settle."""
    rs, ts = m['rs'], m['ts']
    Q.search(rs, code, m['codes'], P)
    if not first:
        Q.seed(rs, ts, m['key_poses'], P)
        seeded_from = ts['committed'].copy()
        ts.update(last_share=share, last_rms=rms, last_pairs=100.0, accepted=1 if tracked else 0, iterations=1)
        if tracked:
            ts['estimate'] = np.asarray(pose, dtype=np.float64).reshape(12).copy()
        frame = ts['frame']
        # the commit's own gates are held wide open, so that only the verification gates (0.1, 0.04) can fail
        m['pose_row'], m['trajectory'][frame] = T.commit(ts, T.Params(min_share=0.01, max_rms=1.0, max_step_m=1e6, max_step_rad=4.0))
        assert m['trajectory'][frame, 12] == (0 if tracked else 1)
    Q.settle(rs, ts, code, m['codes'], m['key_poses'], m['pose_row'], m['trajectory'], m['rows'], P, first=first)
    return m['rows'][ts['frame'] - 1].tolist()


def test_state_machine_by_hand():
    P = Q.Params(ferns=8, capacity=3, tries=2, harvest=2, rows=16, traj_rows=16)
    m = _machine(P)
    rs, ts = m['rs'], m['ts']
    pose = [np.arange(12.0) + 100 * k for k in range(12)]
    code = lambda *ones: np.array([1 if f in ones else 0 for f in range(8)], dtype=np.uint8)
    p0 = ts['committed'].copy()
    # frame 0: tracked by decree, keyframe 0 under the given pose
    assert _frame(m, P, code(), None, True, first=True) == [9, -1, -1, 0, 0, 0, 0, 0]
    assert rs['n'] == 1 and np.array_equal(m['key_poses'][0], p0) and ts['frame'] == 1
    # frame 1: tracked, two ferns differ: not more than harvest, no keyframe
    assert _frame(m, P, code(0, 1), pose[1], True) == [2, 0, -1, -1, 0, 1, 0, 0]
    # frame 2: tracked, three differ: keyframe 1
    assert _frame(m, P, code(0, 1, 2), pose[2], True) == [3, 0, -1, 1, 0, 1, 0, 0]
    assert rs['n'] == 2 and np.array_equal(m['key_poses'][1], pose[2]) and np.array_equal(m['codes'][1], code(0, 1, 2))
    # frame 3: lost, not seeded: the streak begins and the anchor is frame 2's pose
    assert _frame(m, P, code(), pose[3], False) == [0, 0, -1, -1, 1, 2, 0, 0]
    assert np.array_equal(rs['anchor'], pose[2]) and np.array_equal(ts['committed'], pose[2]) and ts['lost'] == 1
    # frame 4: seeded from candidate (1 - 1) mod 2 = the nearest (keyframe 1 for this code), lost again: back to the anchor
    assert _frame(m, P, code(0, 1, 2, 3), pose[4], False) == [1, 1, 1, -1, 2, 2, 0, 0]
    assert np.array_equal(ts['committed'], pose[2]) and np.array_equal(ts['estimate'], pose[2]) and rs['seeded'] == 0
    # frame 5: streak 2 takes candidate 1, the second nearest (keyframe 0); tracked but the share fails verification: demoted
    row = _frame(m, P, code(0, 1, 2, 3), pose[5], True, share=0.05)
    assert row == [1, 1, 0, -1, 3, 2, 1, 0] and ts['lost'] == 3 and rs['recovered'] == 0
    assert np.isnan(m['pose_row']).all() and np.isnan(m['trajectory'][5, :12]).all() and m['trajectory'][5, 12] == 1
    assert m['trajectory'][5, 14] == 0.05 and np.array_equal(ts['committed'], pose[2]) and np.array_equal(ts['estimate'], pose[2])
    # frame 6: the rms fails verification as well
    assert _frame(m, P, code(0, 1, 2, 3), pose[6], True, rms=0.05)[4:7] == [4, 2, 1]
    # frame 7: streak 4 takes candidate 1 again; tracked and verified: recovered, no harvest although the code is far
    assert _frame(m, P, code(3, 4, 5, 6, 7), pose[7], True) == [5, 0, 1, -1, 0, 2, 0, 0]
    assert rs['recovered'] == 1 and rs['n'] == 2 and np.array_equal(ts['committed'], pose[7]) and rs['streak'] == 0
    assert np.array_equal(m['pose_row'], pose[7].astype(np.float32))
    # frame 8: tracked, far from both: keyframe 2 fills the store; frame 9 is as far and finds it full
    assert _frame(m, P, code(3, 4, 5, 6, 7), pose[8], True)[3] == 2 and rs['n'] == 3
    assert _frame(m, P, code(0, 4, 5, 6), pose[9], True) == [3, 2, -1, -1, 0, 2, 0, 0] and rs['n'] == 3
    # a record of garbage: indices out of range are not followed
    rs.update(n=7, streak=3, candidates=9, cand_index=[5, -2, 1, 1])
    before = ts['committed'].copy()
    Q.seed(rs, ts, m['key_poses'], P)                           # candidate (3 - 1) mod 2 = 0 -> index 5 >= n = 3
    assert rs['seeded'] == 0 and np.array_equal(ts['committed'], before)
    ts['frame'] = 99                                            # a row beyond both buffers: lost, nothing written
    rows = m['rows'].copy()
    Q.settle(rs, ts, code(), m['codes'], m['key_poses'], m['pose_row'], m['trajectory'], m['rows'], P)
    assert np.array_equal(rows, m['rows']) and rs['streak'] == 4 and rs['n'] == 3


# -- 4. the scenario on the restated trackers --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scenario():
    v, c, t = synth.synthetic_scene(3, 8)
    poses, phase = Q.scenario_poses()
    depth = Q.scenario_depth(lambda p: R.render(v, c, t, p, T.SEQ_H, T.SEQ_W, 1, R.Camera(**T.SEQ_CAM))['depth'], poses, phase)
    P = Q.scenario_params()
    table = M.fern_table(Q.SCENARIO_SEED, P.ferns, (16, 24))
    return poses, phase, depth, Q.run_scenario(depth, poses[0]), Q.run_scenario(depth, poses[0], P, table), P


def test_the_scenario_conditions(scenario):
    poses, phase, depth, plain, reloc, P = scenario
    a, b, c = (np.array([p == x for p in phase]) for x in 'ABC')
    assert (Q.N_A, Q.N_B, Q.N_C) == (a.sum(), b.sum(), c.sum()) and Q.N_B >= 2 and Q.N_C >= 4 and not depth[b].any() and depth[~b].all()
    # phase C starts half a step between two frames of phase A, and far from the end of phase A
    gap = T.pose_errors(np.repeat(poses[c][:1], 2, 0), poses[a][Q.REAPPEAR:Q.REAPPEAR + 2])[0]
    assert abs(gap[0] - gap[1]) < 0.1 * gap.sum() and gap.min() > 0.005
    est0, lost0, diag0 = plain.trajectory()
    est, lost, diag = reloc.trajectory()
    rows, count, key_poses = reloc.relocalisation()
    print('plain lost', lost0.astype(int).tolist())
    print('reloc lost', lost.astype(int).tolist())
    print('rows', rows[:, :7].tolist())
    # (a) the plain tracker loses every frame of phases B and C
    assert not lost0[a].any() and lost0[b].all() and lost0[c].all()
    # (b) the relocalising tracker loses at most the first `tries` frames of phase C
    assert not lost[a].any() and lost[b].all()
    first_c = np.flatnonzero(c)[0]
    assert not lost[first_c + P.tries:].any() and lost[c].sum() <= P.tries and not lost[c][np.flatnonzero(~lost[c])[0]:].any()
    assert reloc.rs['recovered'] == 1 and (rows[c, 2] >= 0).sum() == lost[c].sum() + 1
    # (c) at least 3 keyframes in phase A, none in B
    assert (rows[a, 3] >= 0).sum() >= 3 and (rows[b, 3] == -1).all() and count == (rows[:, 3] >= 0).sum()
    # (d) no gate quantity within a relative 1e-6 of its threshold, on any frame of either tracker
    Tp = T.Params()
    for d in (diag0[1:], diag[1:]):
        for column, limit in ((2, Tp.min_share), (3, Tp.max_rms), (6, Tp.max_step_m), (7, Tp.max_step_rad)):
            assert (np.abs(d[:, column] - limit) > 1e-6 * limit).all(), (column, d[:, column])
    assert (np.abs(rows[:, 0] - P.harvest) > 1e-6 * P.harvest).all(), rows[:, 0]
    for limit, x in ((P.min_share, diag[1:, 2]), (P.max_rms, diag[1:, 3])):
        assert (np.abs(x - limit) > 1e-6 * limit).all()
    # the recovered frames are ordinary tracked frames: the bound of tests/test_gpu_track.py
    keep = ~lost
    dt, dr = T.pose_errors(est[keep], poses[keep])
    print('worst %.6f voxel, %.6f degrees over %d tracked frames; phase C %s voxel' % ((dt / T.SEQ_VOXEL).max(), dr.max(), keep.sum(),
                                                                                      np.round(dt[c[keep]] / T.SEQ_VOXEL, 4).tolist()))
    assert (dt / T.SEQ_VOXEL).max() <= 2 * RECORDED_VOXELS and dr.max() <= 2 * RECORDED_DEGREES
    # no lost frame reached the volume: phase A's volume is the plain tracker's, which saw nothing after it
    assert np.array_equal(est[a].view(np.uint64), est0[a].view(np.uint64))


# -- 5. the files ---------------------------------------------------------------------------------------------------------------------------
def test_written_reports_with_and_without_the_relocaliser(tmp_path):
    from kfnet_amd.tools.io import read_lines
    seq = tmp_path / 'seq'
    seq.mkdir()
    _touch_frames(seq, 4)
    pairs = read_frames(str(seq))
    poses = synth.synthetic_poses(4)
    poses[2] = np.nan
    lost = np.array([False, False, True, False])
    diag = np.array([[0, 0, 0, 0, 0, 0, 0, 0], [0, 4208, 0.685, 2.79e-3, 19, 19, 0.0216, 9.5e-3], [1, 0, 0, 0, 0, 19, 0, 0],
                     [0, 4427, 0.72, 2.4e-3, 18, 19, 0.02, 0.01]], dtype=np.float64)
    rows = np.array([[501, -1, -1, 0, 0, 0, 0, 0], [120, 0, -1, 1, 0, 1, 0, 0], [250, 1, -1, -1, 1, 2, 0, 0], [3, 1, 1, -1, 0, 2, 0, 0]], dtype=np.int32)
    plain, with_rows = tmp_path / 'plain', tmp_path / 'reloc'
    M.write_outputs(str(plain), pairs, poses, lost, diag)
    M.write_outputs(str(with_rows), pairs, poses, lost, diag, rows)
    assert not (plain / 'reloc_report.txt').exists()
    states = lambda folder: [x.split()[1] for x in read_lines(str(folder / 'track_report.txt')) if x][1:]
    assert states(plain) == ['tracked', 'tracked', 'lost', 'tracked'] and states(with_rows) == ['tracked', 'tracked', 'lost', 'relocalised']
    for name in ('image_list.txt', 'depth_list.txt'):
        assert open(str(plain / name)).read() == open(str(with_rows / name)).read()
    assert len([x for x in read_lines(str(with_rows / 'pose_list.txt')) if x]) == 3
    report = [x for x in read_lines(str(with_rows / 'reloc_report.txt')) if x]
    assert report[0] == '# frame nearest distance seeded_key keyframe_added streak' and len(report) == 5
    assert report[1].split() == ['frame-000000.depth.png', '-1', '501', '-1', '0', '0']
    assert report[3].split() == ['frame-000002.depth.png', '1', '250', '-1', '-1', '1']
    assert report[4].split() == ['frame-000003.depth.png', '1', '3', '1', '-1', '0']
