"""The mesh renderer's host side: PLY files, the float32 restatement against the fp64 one, the hand cases,
the synthetic scene, and the refusals of the exports and of the program.  Nothing here needs a device."""
import collections
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import render_ref as R
from kfnet_amd import _lib, synth
from kfnet_amd import render as M
from kfnet_amd.labels import DepthCamera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- 1. PLY -----------------------------------------------------------------------------------------------------------------
def _independent_ply(path, verts, faces, colors, binary, double=False, extra=False, int_count=False):
    """A writer that shares nothing with kfnet_amd.render.write_ply: struct.pack row by row."""
    ft = 'double' if double else 'float'
    head = ['ply', 'format %s 1.0' % ('binary_little_endian' if binary else 'ascii'), 'comment made by the test',
            'element vertex %d' % len(verts)]
    if extra:
        head += ['property float nx']
    head += ['property %s x' % ft, 'property %s y' % ft, 'property %s z' % ft]
    if extra:
        head += ['property ushort quality']
    if colors is not None:
        head += ['property uchar red', 'property uchar green', 'property uchar blue', 'property uchar alpha']
    head += ['element face %d' % len(faces), 'property list %s %s vertex_indices' % ('int' if int_count else 'uchar', 'uint' if int_count else 'int')]
    if extra:
        head += ['property uchar flags']
    head += ['end_header']
    body = b''
    for k, p in enumerate(verts):
        if binary:
            row = (struct.pack('<f', 0.5) if extra else b'') + struct.pack('<3d' if double else '<3f', *p)
            row += struct.pack('<H', 7) if extra else b''
            row += struct.pack('<4B', *(list(colors[k]) + [255])) if colors is not None else b''
        else:
            words = (['0.5'] if extra else []) + [repr(float(x)) for x in p] + (['7'] if extra else [])
            words += [str(int(x)) for x in colors[k]] + ['255'] if colors is not None else []
            row = (' '.join(words) + '\n').encode()
        body += row
    for f in faces:
        if binary:
            row = struct.pack('<i' if int_count else '<B', len(f)) + struct.pack('<%d%s' % (len(f), 'I' if int_count else 'i'), *f)
            row += struct.pack('<B', 1) if extra else b''
        else:
            row = (' '.join([str(len(f))] + [str(i) for i in f] + (['1'] if extra else [])) + '\n').encode()
        body += row
    with open(path, 'wb') as fh:
        fh.write(('\n'.join(head) + '\n').encode() + body)


@pytest.mark.parametrize('binary', (False, True))
@pytest.mark.parametrize('double,extra,coloured,int_count', ((False, False, True, False), (True, True, True, True),
                                                              (True, False, False, False), (False, True, False, True)))
def test_read_ply_against_an_independent_writer(tmp_path, binary, double, extra, coloured, int_count):
    rng = np.random.default_rng(3)
    verts = rng.normal(size=(7, 3)).astype(np.float32).astype(np.float64)
    colors = rng.integers(0, 256, size=(7, 3)).astype(np.uint8) if coloured else None
    faces = [[0, 1, 2], [2, 3, 4, 5], [6, 5, 4, 3, 2]]                     # a triangle, a quad, a pentagon
    path = str(tmp_path / 'm.ply')
    _independent_ply(path, verts, faces, colors, binary, double, extra, int_count)
    v, c, t = M.read_ply(path)
    assert v.dtype == np.float32 and t.dtype == np.int32
    assert np.array_equal(v, verts.astype(np.float32))
    assert (c is None) if colors is None else (c.dtype == np.uint8 and np.array_equal(c, colors))
    assert t.tolist() == [[0, 1, 2], [2, 3, 4], [2, 4, 5], [6, 5, 4], [6, 4, 3], [6, 3, 2]]


@pytest.mark.parametrize('binary', (False, True))
@pytest.mark.parametrize('coloured', (False, True))
def test_write_ply_round_trip(tmp_path, binary, coloured):
    v, c, t = synth.synthetic_scene(2, 2)
    path = str(tmp_path / 's.ply')
    M.write_ply(path, v, t, c if coloured else None, binary=binary)
    v2, c2, t2 = M.read_ply(path)
    assert np.array_equal(v2, v) and np.array_equal(t2, t)
    assert np.array_equal(c2, c) if coloured else c2 is None


def test_read_ply_refusals_name_the_file_and_the_place(tmp_path):
    verts = np.eye(3)
    path = str(tmp_path / 'bad.ply')

    def refused(*words):
        with pytest.raises(ValueError) as e:
            M.read_ply(path)
        assert 'bad.ply' in str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)
    _independent_ply(path, verts, [[0, 1, 2]], None, True)
    data = open(path, 'rb').read()
    open(path, 'wb').write(data.replace(b'binary_little_endian', b'binary_big_endian'))
    refused('big-endian', 'line 2')
    open(path, 'wb').write(data[:-3])
    refused('truncated', 'byte %d' % (len(data) - 3))
    open(path, 'wb').write(data[:-14])                                       # inside the vertex table
    refused('truncated', 'byte')
    _independent_ply(path, verts, [[0, 1]], None, True)
    refused('below 3', 'byte')
    _independent_ply(path, verts, [[0, 1, 2], [0, 1]], None, False)
    refused('below 3', 'line 15')          # 10 header lines, 3 vertices, the second face
    _independent_ply(path, verts, [[0, 1, 2], [0, 1, 2]], None, False)
    text = open(path).read().split('\n')
    open(path, 'w').write('\n'.join(text[:-2]) + '\n')
    refused('truncated', 'line')
    head = 'ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n0 0 0\n'
    open(path, 'w').write(head)
    refused('no face element')
    open(path, 'w').write('plx\n')
    refused('line 1')


# -- 2. the float32 restatement against the fp64 one ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def random_runs():
    runs = []
    for args, counts in R.RANDOM_CASES:
        v, c, t, poses, cam = R.scene_case(*args)
        H, W, s = args[:3]
        runs.append((args, counts, cam, R.render(v, c, t, poses, H, W, s, cam),
                     R.render(v, c, t, poses, H, W, s, cam, dtype=np.float64, candidates=True), (v, c, t, poses)))
    return runs


def test_the_fp64_reference_keeps_the_recorded_share_of_unclear_samples(random_runs):
    for args, counts, cam, lo, hi, _ in random_runs:
        clear, allowed = R.classify(hi)
        covered = int((hi['winner'] >= 0).sum())
        unclear = sum(1 for k in allowed if hi['winner'][k] >= 0)
        print(args, 'covered', covered, 'unclear', unclear)
        assert (covered, unclear) == counts, (args, covered, unclear)
        assert unclear <= 0.02 * covered
        assert int(clear.sum()) + unclear == covered                         # no sample goes unchecked


def _label_error_yardstick(hi, cam, poses, stride):
    """The error of the label formula evaluated in float32 from fp64's z (the winner's depth): |fp32(...) - fp64(...)|."""
    P64 = R.pose_rows32(poses).astype(np.float64)
    B, h, w = hi['winner'].shape
    out = np.zeros((B, h, w))
    for b in range(B):
        for f in (np.float32, np.float64):
            P, z = P64[b].astype(f), hi['z'][b].astype(f)
            rx = ((np.arange(w) * stride).astype(f)[None, :] - f(cam.u)) * f(cam.inv_fx)
            ry = ((np.arange(h) * stride).astype(f)[:, None] - f(cam.v)) * f(cam.inv_fy)
            X, Y = rx * z, ry * z
            lab = np.stack([((P[4 * i] * X + P[4 * i + 1] * Y) + P[4 * i + 2] * z) + P[4 * i + 3] for i in range(3)], axis=-1)
            if f is np.float32:
                lo = lab.astype(np.float64)
        out[b] = np.abs(lo - lab).max(axis=-1)
    return out


def test_float32_restatement_agrees_with_fp64(random_runs):
    extent = float(np.linalg.norm(synth.ROOM))
    for args, counts, cam, lo, hi, (v, c, t, poses) in random_runs:
        clear, allowed = R.classify(hi)
        assert np.array_equal(lo['winner'][clear], hi['winner'][clear]), args
        assert np.array_equal(lo['labels'][..., 3][clear], hi['labels'][..., 3][clear]), args
        e = _label_error_yardstick(hi, cam, poses, args[2])
        diff = np.abs(lo['labels'][..., :3].astype(np.float64) - hi['labels'][..., :3]).max(axis=-1)
        bound = np.maximum(8.0 * e / extent, 1e-6) * extent
        assert (diff[clear] <= bound[clear]).all(), (args, (diff[clear] / bound[clear]).max())
        for key, winners in allowed.items():
            assert int(lo['winner'][key]) in winners, (args, key, int(lo['winner'][key]), winners)
        rest = ~clear
        for key in allowed:
            rest[key] = False
        assert (lo['winner'][rest] == -1).all() and (hi['winner'][rest] == -1).all()
        assert np.array_equal(lo['stats'][:, 1:], hi['stats'][:, 1:])


# -- 3. hand cases: every quantity exact in fp32 ------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hand():
    return dict((name, R.render(v, None, t, R.IDENTITY, 16, 24, 1, cam)) for name, (v, t, cam) in R.hand_cases().items())


def _covered(run):
    return set((int(x), int(y)) for y, x in zip(*np.nonzero(run['winner'][0] >= 0)))


def _alone(name):
    v, t, cam = R.hand_cases()[name]
    return [R.render(v, None, t[k:k + 1], R.IDENTITY, 16, 24, 1, cam)['winner'][0] >= 0 for k in range(len(t))]


def test_one_triangle_covers_its_top_left_samples(hand):
    assert _covered(hand['one']) == set((x, y) for x in range(24) for y in range(16) if x + y < 8)
    on = hand['one']['winner'][0] >= 0
    assert (hand['one']['z'][0][on] == 1.0).all() and (hand['one']['depth'][0][on] == 4).all()
    lab = hand['one']['labels'][0]
    assert lab[3, 2].tolist() == [2.0, 3.0, 1.0, 1.0] and lab[0, 0].tolist() == [0.0, 0.0, 1.0, 1.0]     # the vertex on a sample
    assert hand['one']['stats'][0].tolist() == [36, 1, 0, 0, 0]


def test_a_shared_edge_through_sample_points_is_covered_exactly_once(hand):
    for name in ('shared_edge', 'fan'):
        each = np.sum(_alone(name), axis=0)
        inside = np.zeros((16, 24), dtype=int)
        inside[:8, :8] = 1
        assert np.array_equal(each, inside), name
    w = hand['shared_edge']['winner'][0]
    assert all(w[k, k] == 0 for k in range(8))             # the diagonal is the upper triangle's left edge
    assert hand['fan']['winner'][0][4, 4] in (0, 1, 2, 3)


def test_sliver_duplicate_and_depth_order(hand):
    assert not _covered(hand['sliver']) and hand['sliver']['stats'][0].tolist() == [0, 1, 0, 0, 0]
    assert set(np.unique(hand['twice']['winner'])) == {-1, 0}
    for name, nearer in (('near_first', 0), ('near_last', 1)):
        assert set(np.unique(hand[name]['winner'])) == {-1, nearer}
        assert len(_covered(hand[name])) == 36
        assert (hand[name]['z'][0][hand[name]['winner'][0] >= 0] == 1.0).all()


def test_behind_the_camera_and_across_the_near_plane(hand):
    assert not _covered(hand['behind']) and hand['behind']['stats'][0].tolist() == [0, 0, 0, 0, 0]
    # one vertex behind: the polygon (0,0) (8,0) (12,2) (0,2); z = 1 / (1 + y / 2)
    one = hand['clip_one']
    assert _covered(one) == set((x, 0) for x in range(8)) | set((x, 1) for x in range(10))
    assert one['stats'][0].tolist() == [18, 1, 1, 0, 0]
    assert (one['z'][0][0, :8] == 1.0).all() and (one['z'][0][1, :10] == np.float32(1.0) / np.float32(1.5)).all()
    # two behind: the polygon (0,0) (4,0) (0,4); z = 1 / (1 + (x + y) / 4)
    two = hand['clip_two']
    assert _covered(two) == set((x, y) for x in range(4) for y in range(4) if x + y < 4)
    for x, y in _covered(two):
        assert two['z'][0][y, x] == np.float32(1.0) / np.float32(1.0 + (x + y) / 4.0)


def test_a_triangle_far_larger_than_the_image_covers_all_of_it(hand):
    assert (hand['huge']['winner'] == 0).all() and (hand['huge']['depth'] == 4).all()


def test_raw_depth_ties_go_to_even_and_the_window_masks(hand):
    tie = hand['tie']
    first, second = tie['winner'][0] == 0, tie['winner'][0] == 1
    assert first.sum() == 36 and second.any()
    assert (tie['depth'][0][first] == 0).all() and (tie['labels'][0][first] == 0).all()         # 2 / 4 = 0.5 -> 0: invalid
    assert (tie['depth'][0][second] == 2).all() and (tie['labels'][0][second][:, 3] == 1).all()  # 6 / 4 = 1.5 -> 2
    far = hand['beyond']
    beyond = far['winner'][0] == 1
    assert beyond.any() and (far['depth'][0][beyond] == 0).all() and (far['labels'][0][beyond] == 0).all()
    assert (far['labels'][0][far['winner'][0] == 0][:, 3] == 1).all()
    assert far['stats'][0, 0] == (far['winner'] >= 0).sum() > far['labels'][..., 3].sum()


# -- 4. the synthetic scene ---------------------------------------------------------------------------------------------------
def test_synthetic_scene_is_closed_and_reproducible():
    v, c, t = synth.synthetic_scene(9, 6)
    assert v.dtype == np.float32 and c.dtype == np.uint8 and t.dtype == np.int32 and len(t) == 48 * 36
    edges = collections.Counter()
    for a, b, d in t.tolist():
        for x, y in ((a, b), (b, d), (d, a)):
            edges[(min(x, y), max(x, y))] += 1
    assert set(edges.values()) == {2}
    again = synth.synthetic_scene(9, 6)
    assert all(np.array_equal(x, y) for x, y in zip((v, c, t), again))
    assert not np.array_equal(synth.synthetic_scene(10, 6)[1], c)
    assert len(np.unique(c, axis=0)) > len(c) // 2                          # texture, not one colour
    assert np.allclose(v.min(axis=0), 0) and np.allclose(v.max(axis=0), synth.ROOM)


def test_synthetic_trajectory_stays_inside_and_away_from_every_surface():
    for seed in (1, 2, 3, 4, 5, 11):
        poses = synth.synthetic_trajectory(200, seed)
        assert np.array_equal(poses, synth.synthetic_trajectory(200, seed))
        Rm = poses[:, :3, :3]
        assert np.allclose(Rm @ Rm.transpose(0, 2, 1), np.eye(3), atol=1e-12) and np.allclose(np.linalg.det(Rm), 1.0)
        centres = poses[:, :3, 3]
        boxes = synth.synthetic_scene_boxes(seed)
        lo, hi = boxes[0]
        assert (centres - lo >= 0.3).all() and (hi - centres >= 0.3).all()
        for lo, hi in boxes[1:]:
            outside = np.maximum(np.maximum(lo - centres, centres - hi), 0.0)
            assert (np.linalg.norm(outside, axis=1) >= 0.3).all()
        assert np.abs(np.diff(centres, axis=0)).max() < 0.15                # smooth


# -- 5. the exports' refusals: KFN_ERR_ARG with nothing launched, so no device is needed ---------------------------------------
CAM = DepthCamera()


def _desc(**change):
    ok = dict(B=1, V=3, N=1, H=16, W=24, stride=8, near=0.05)
    ok.update(change)
    ld = ok.pop('ld_labels', 4)
    cam = ok.pop('camera', CAM)
    return M.render_descriptor(cam, ok['B'], ok['V'], ok['N'], ok['H'], ok['W'], ok['stride'], ok['near'], ld)


def _render_call(d, **null):
    lib = _lib.load()
    p = dict(vertices=0x1000, colors=None, triangles=0x1000, poses=0x1000, zbuf=0x1000, labels=0x1000, depth=None, frames=None,
             stats=None)
    p.update(null)
    rc = lib.kfn_render(C.byref(d), p['vertices'], p['colors'], p['triangles'], p['poses'], p['zbuf'], p['labels'], p['depth'],
                        p['frames'], p['stats'], None)
    return rc, lib.kfn_last_error().decode()


def test_render_argument_checks():
    assert C.sizeof(_lib.RenderDesc) == 72
    for change, word in ((dict(stride=2), 'stride'), (dict(stride=0), 'stride'), (dict(H=20), 'multiples of the stride'),
                         (dict(W=30), 'multiples of the stride'), (dict(H=0), 'positive'), (dict(B=0), 'positive'),
                         (dict(V=0), 'positive'), (dict(N=-1), 'positive'), (dict(ld_labels=3), 'ld_labels'),
                         (dict(near=0.0), 'near'), (dict(near=-1.0), 'near'), (dict(B=70000), '65535'),
                         (dict(B=40000, H=480, W=640, stride=1), '2^31')):
        rc, msg = _render_call(_desc(**change))
        assert rc == -1 and word in msg, (change, msg)
    for field, value, word in (('scale', 0.0, 'scale'), ('raw_min', -1, 'window'), ('raw_max', 65536, 'window'), ('raw_min', 70000, 'window')):
        d = _desc()
        setattr(d, field, value)
        rc, msg = _render_call(d)
        assert rc == -1 and word in msg, (field, msg)
    d = _desc()
    d.struct_size -= 4
    rc, msg = _render_call(d)
    assert rc == -1 and 'struct_size' in msg
    for null in ('vertices', 'triangles', 'poses', 'zbuf'):
        rc, msg = _render_call(_desc(), **{null: None})
        assert rc == -1 and 'null' in msg
    assert _lib.load().kfn_render(None, *([0x1000] * 9 + [None])) == -1
    size = C.c_size_t()
    lib = _lib.load()
    assert lib.kfn_render_scratch_bytes(C.byref(_desc(B=3, H=64, W=96)), C.byref(size)) == 0 and size.value == 3 * 8 * 12 * 8
    assert lib.kfn_render_scratch_bytes(C.byref(_desc(stride=3)), C.byref(size)) == -1
    assert lib.kfn_render_scratch_bytes(C.byref(_desc()), None) == -1


def test_descriptor_constants_are_rounded_once_and_the_abi_number_stays():
    cam = DepthCamera(585.0, 583.0, 317.5, 241.25)
    d = M.render_descriptor(cam, 1, 3, 1, 480, 640, 8)
    assert d.inv_fx == np.float32(1.0 / 585.0) and d.inv_fy == np.float32(1.0 / 583.0)
    assert d.scale == np.float32(0.001) and d.near == np.float32(0.05) and (d.raw_min, d.raw_max) == (1, 65534)
    lib = _lib.load()
    assert lib.kfn_abi_version() == 13 and _lib.ABI_VERSION == 13
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ('kfn_render', 'kfn_render_scratch_bytes'):
        assert name in _lib.SYMBOLS and getattr(raw, name) is not None
    hdr = open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()
    assert '#define KFN_ABI_VERSION 13' in hdr and 'typedef struct kfn_render_desc {' in hdr
    from kfnet_amd import build
    assert build.EXTRA['kfn_render.hip'] == ['-ffp-contract=off']


# -- 6. the program's refusals, before torch touches a device -------------------------------------------------------------------
def test_render_make_argument_errors(tmp_path, capsys):
    v, c, t = synth.synthetic_scene(1, 1)
    model, bare = str(tmp_path / 'scene.ply'), str(tmp_path / 'bare.ply')
    M.write_ply(model, v, t, c)
    M.write_ply(bare, v, t)
    pose = str(tmp_path / 'p.txt')
    np.savetxt(pose, np.eye(4))
    plist = str(tmp_path / 'pose_list.txt')
    open(plist, 'w').write(pose + '\n')
    out = str(tmp_path / 'out')
    ok = ['make', '--model', model, '--poses', plist, '--output_folder', out]
    for args, word in ((['make', '--poses', plist, '--output_folder', out], '--model'),
                       (['make', '--model', model, '--output_folder', out], '--poses or --sequence'),
                       (ok + ['--sequence', str(tmp_path)], '--poses or --sequence'),
                       (['make', '--model', model, '--poses', plist], '--output_folder'),
                       (ok + ['--height', '100'], 'multiples of 8'), (ok + ['--batch', '0'], '--batch'),
                       (ok + ['--stride', '4'], '--stride'), (ok + ['--near', '0'], '--near'),
                       (ok + ['--focal_x', '-3'], 'positive'), (ok + ['--depth_u', '300'], 'depth camera'),
                       (['make', '--model', str(tmp_path / 'nowhere.ply'), '--poses', plist, '--output_folder', out], 'nowhere.ply'),
                       (['make', '--model', model, '--poses', str(tmp_path / 'none.txt'), '--output_folder', out], 'none.txt'),
                       (['make', '--model', pose, '--poses', plist, '--output_folder', out], 'not a PLY'),
                       (['make', '--model', bare, '--poses', plist, '--output_folder', out, '--frames'], 'no vertex colours')):
        assert M.main(args) == 1, args
        assert word in capsys.readouterr().err, args
    open(plist, 'w').write(pose + '\n' + str(tmp_path / 'gone.txt') + '\n')
    assert M.main(ok) == 1
    assert 'gone.txt is missing' in capsys.readouterr().err
    assert M.main([]) == 1
    assert not os.path.exists(out)                # nothing was written by a refused call
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'kfnet_amd.render', 'make', '--output_folder', out], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 1 and '--model' in r.stderr and len(r.stderr.strip().split('\n')) == 1


def test_write_png_is_what_the_library_decodes(tmp_path):
    from kfnet_amd.labels import load_depth
    rng = np.random.default_rng(5)
    depth = rng.integers(0, 65536, size=(16, 24)).astype(np.uint16)
    path = str(tmp_path / 'd.png')
    M.write_png(path, depth)
    assert np.array_equal(load_depth([path], (16, 24))[0], depth)
    with pytest.raises(ValueError):
        M.write_png(path, depth.astype(np.int32))
