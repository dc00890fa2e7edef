"""Fusion and mesh extraction, the host side: the float32 restatement against the fp64 one, extraction on
analytic fields, the table of the kernel source against the rule, and the refusals of the exports and of the program.
Nothing here needs a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fuse_ref as F
import render_ref as R
from kfnet_amd import _lib
from kfnet_amd import fuse as M
from kfnet_amd.labels import DepthCamera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_rendered = dict()


def cpu_render(v, c, t, poses, H, W, cam):
    """render_ref at stride 1: what the Renderer gives bit for bit (tests/test_gpu_render.py)."""
    key = (len(t), poses.tobytes(), H, W, tuple(sorted(cam.items())))
    if key not in _rendered:
        out = R.render(v, c, t, poses, H, W, 1, R.Camera(**cam))
        _rendered[key] = (out['depth'], out['frames'])
    return _rendered[key]


# -- 1. the table ---------------------------------------------------------------------------------------------------------------
def test_the_kernel_sources_table_is_the_one_the_rule_gives():
    src = open(os.path.join(ROOT, 'kfnet_amd', 'csrc', 'kfn_fuse.hip')).read()
    body = src[src.index('TRI_EDGES[16][6] = {'):]
    rows = re.findall(r'^\s*\{([\d, ]+)\},', body[:body.index('};')], re.M)
    assert len(rows) == 16
    counts = [int(x) for x in re.search(r'TRI_COUNT\[16\] = \{([\d, ]+)\}', src).group(1).split(',')]
    assert counts == F.TRI_COUNT.tolist() == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]
    for m, row in enumerate(rows):
        got = [int(x) for x in row.split(',')]
        want = [4 * p + q for tri in F.TABLE[m] for (p, q) in tri]
        assert got[:len(want)] == want and not any(got[len(want):]), m
    tet = re.search(r'TET\[6\]\[4\] = \{(.*?)\};', src).group(1)
    assert [tuple(int(x) for x in g.split(',')) for g in re.findall(r'\{([\d, ]+)\}', tet)] == list(F.TET)
    assert [int(x) for x in re.search(r'TET_ODD\[6\] = \{([\d, ]+)\}', src).group(1).split(',')] == list(F.TET_ODD)
    # every crossing edge of a mask is used, and only crossing edges
    for m in range(1, 15):
        used = set(e for tri in F.TABLE[m] for e in tri)
        assert used == set((p, q) for p in range(4) for q in range(p + 1, 4) if ((m >> p) ^ (m >> q)) & 1)


# -- 2. the float32 restatement against the fp64 one ------------------------------------------------------------------------------
# name -> (the sum of W in fp64: the voxel-frame pairs that pass step 7, capped in 'cap'; the pairs left unclear) of the
# 19 x 13 x 11 x 3 = 8151 pairs: chosen and recorded on the CPU
RECORDED = {
    'plain': (1201, 1), 'unregistered': (977, 0), 'no_color': (1201, 1), 'nan_pose': (801, 1), 'window': (1073, 1), 'cap': (821, 1),
}


@pytest.fixture(scope='module')
def integrate_runs():
    runs = dict()
    for name in F.INTEGRATE_CASES:
        S, depth, frames, poses = F.integrate_case(name, cpu_render)
        t0, c0 = S.empty(frames is not None)
        lo = F.integrate(t0, c0, depth, frames, poses, S)
        hi = F.integrate(t0, c0, depth, frames, poses, S, dtype=np.float64, audit=True)
        runs[name] = (S, depth, frames, poses, lo, hi)
    return runs


def test_the_cases_exercise_what_they_are_named_for(integrate_runs):
    S, depth, frames, poses, lo, hi = integrate_runs['plain']
    W = lo[0][..., 1]
    assert W.max() == 3 and (W == 0).any() and (W == 1).any()             # seen by all, by none, by some
    P = F.pose_rows32(poses)
    px, py, pz = F._lattice(S, np.float64)
    for b in range(len(P)):
        Z = (P[b][2] * (px - P[b][3]) + P[b][6] * (py - P[b][7])) + P[b][10] * (pz - P[b][11])
        assert (Z < S.near).any() and (Z > 1.0).any()                       # part of the volume behind every camera
    assert (lo[0][..., 0] < 0).any() and (lo[0][..., 0] == 1).any()
    assert (lo[1][..., 3] > 0).any() and ((lo[1][..., 3] == 0) & (W > 0)).any()
    assert integrate_runs['cap'][4][0][..., 1].max() == 2
    assert np.array_equal(integrate_runs['cap'][4][0][..., 0], lo[0][..., 0])        # the cap binds on the third frame: W alone differs
    assert integrate_runs['nan_pose'][4][0][..., 1].max() == 2
    assert integrate_runs['window'][4][0][..., 1].sum() < W.sum()
    assert not np.array_equal(integrate_runs['unregistered'][4][0], lo[0])
    assert integrate_runs['no_color'][4][1] is None and np.array_equal(integrate_runs['no_color'][4][0], lo[0])


def test_float32_integration_agrees_with_fp64_where_every_decision_is_clear(integrate_runs):
    for name in F.INTEGRATE_CASES:
        S, depth, frames, poses, lo, hi = integrate_runs[name]
        t32, t64, audit = lo[0], hi[0], hi[2]
        pairs = audit['unclear'].size
        unclear = int(audit['unclear'].sum())
        applied = int(t64[..., 1].sum())
        print(name, 'pairs', pairs, 'applied', applied, 'unclear', unclear)
        assert unclear < 0.02 * pairs
        assert pairs == 8151 and (applied, unclear) == RECORDED[name], (name, applied, unclear)
        clear = ~audit['unclear'].any(axis=0)
        assert np.array_equal(t32[..., 1][clear], t64[..., 1][clear]), name
        diff = np.abs(t32[..., 0].astype(np.float64) - t64[..., 0])
        assert (diff[clear] <= audit['bound'][clear]).all(), (name, (diff[clear] - audit['bound'][clear]).max())
        print(name, 'largest |D32 - D64| %.3g, largest bound %.3g' % (diff[clear].max(), audit['bound'].max()))
        assert audit['bound'].max() < 4e-5                     # the yardstick: some ten ulps of the 10 m coordinates over trunc = 0.5 m
        if lo[1] is not None:
            same = clear & (lo[1][..., 3] == hi[1][..., 3])
            assert same.sum() > 0.95 * clear.sum()
            assert np.abs(lo[1][..., :3][same] - hi[1][..., :3][same]).max() <= 255 * 16 * F.EPS32


def test_hand_case_every_threshold_met_exactly():
    S, depth, frames, poses, where = F.hand_case()
    for f in (np.float32, np.float64):
        tsdf, col = F.integrate(*S.empty(), depth, frames, poses, S, dtype=f)
        at = lambda a, k: a[where[k][2], where[k][1], where[k][0]].tolist()
        assert at(tsdf, 'near') == [1.0, 1.0] and at(col, 'near') == [0.0, 0.0, 0.0, 0.0]          # Z == near is taken; s = 2.5 > trunc
        assert at(tsdf, 'behind') == [1.0, 1.0] and at(col, 'behind') == [0.0, 0.0, 0.0, 0.0]
        assert at(tsdf, 'minus_trunc') == [-1.0, 1.0] and at(col, 'minus_trunc') == [200.0, 100.0, 50.0, 1.0]   # s == -trunc is taken
        assert at(tsdf, 'plus_trunc') == [1.0, 1.0] and at(col, 'plus_trunc') == [200.0, 100.0, 50.0, 1.0]      # s == trunc: painted
        assert at(tsdf, 'tie_down') == [-1.0, 1.0] and at(col, 'tie_down') == [200.0, 100.0, 50.0, 1.0]         # 8.5 -> 8
        assert at(tsdf, 'tie_up') == [-1.0, 1.0] and at(col, 'tie_up') == [10.0, 20.0, 30.0, 1.0]               # 9.5 -> 10
        assert at(tsdf, 'between') == [0.0, 0.0]                                                                # 9: the invalid pixel


# -- 3. extraction on analytic fields ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fields():
    return dict((name, (S, tsdf) + F.extract(tsdf, None, S)) for name, (S, tsdf) in F.analytic_fields().items())


def test_a_plane_between_lattice_layers(fields):
    S, tsdf, v, c, t = fields['plane']
    side = (S.dims[0] - 1) * S.voxel
    assert np.abs(v[:, 2].astype(np.float64) - F.PLANE_OFFSET).max() <= 4 * F.EPS32 * 4.0
    assert abs(F.area(v, t) - side * side) <= 1e-5 * side * side
    assert len(np.unique(t)) == len(v) and (c == 255).all()
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    assert (n[:, 2] < 0).all()                                               # D < 0 above the plane: inside -> outside is -z


def test_a_tilted_plane_not_through_lattice_points(fields):
    S, tsdf, v, c, t = fields['tilted_plane']
    nrm, off = F.TILTED_NORMAL, F.TILTED_POINT
    d = (v.astype(np.float64) - off) @ nrm / np.linalg.norm(nrm)
    assert np.abs(d).max() <= 32 * F.EPS32 * 4.0, np.abs(d).max()
    side = (S.dims[0] - 1) * S.voxel
    want = side * side * np.linalg.norm(nrm) / nrm[2]                          # the plane leaves the box through its four walls
    assert abs(F.area(v, t) - want) <= 1e-5 * want
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]).astype(np.float64)
    assert (n @ nrm >= 0).all() and (n @ nrm > 0).sum() > 0.9 * len(t)        # inside (D < 0) is where the normal comes from


def sphere_checks(S, v, t):
    F.closed_surface_checks(v, t)
    r, h = F.SPHERE_RADIUS, S.voxel
    dist = np.linalg.norm(v.astype(np.float64) - np.asarray(F.SPHERE_CENTRE), axis=1)
    bound = 3.0 * h * h / (8.0 * (r - np.sqrt(3.0) * h))
    print('sphere: %d vertices, %d triangles, largest | |v - c| - r | %.3g of %.3g' % (len(v), len(t), np.abs(dist - r).max(), bound))
    assert np.abs(dist - r).max() <= bound


def test_a_sphere_is_closed_oriented_and_close(fields):
    S, tsdf, v, c, t = fields['sphere']
    sphere_checks(S, v, t)
    exact = 4.0 / 3.0 * np.pi * F.SPHERE_RADIUS ** 3
    assert 0.97 * exact < F.signed_volume(v, t) < exact                        # chords lie inside the sphere


def test_two_disjoint_spheres(fields):
    S, tsdf, v, c, t = fields['two_spheres']
    F.closed_surface_checks(v, t, components=2)


def test_a_sphere_cut_by_an_invalid_half_space(fields):
    S, tsdf, v, c, t = fields['cut_sphere']
    uses = F.edge_uses(t)
    assert set(uses.values()) == {1}
    boundary = [e for e in uses if (e[1], e[0]) not in uses]
    assert boundary and len(boundary) < len(uses) // 4                         # one or two triangles an edge
    last_valid = np.floor(1.7 / S.voxel - 1e-9) * S.voxel
    assert v[np.unique(t)][:, 0].max() <= last_valid                            # no triangle touches an invalid point
    full = fields['sphere']
    assert 0 < len(t) < len(full[4])
    assert F.euler(len(np.unique(t)), t) == 1                                   # a disc


def test_garbage_and_edge_values_in_the_volume():
    S = F.Setup(dims=(5, 4, 3), origin=(0, 0, 0), voxel=0.5)
    tsdf = np.zeros((3, 4, 5, 2), dtype=np.float32)
    v, c, t = F.extract(tsdf, None, S)
    assert v.shape == (0, 3) and t.shape == (0, 3)                             # the empty volume
    tsdf[..., 1] = 1
    tsdf[..., 0] = 1
    tsdf[1, 1, 1, 0] = 0.0                                                     # D == 0 is outside: nothing crosses
    assert F.extract(tsdf, None, S)[2].shape == (0, 3)
    tsdf[1, 1, 1, 0] = -1.0                                                    # one inside point: a closed surface around it
    v, c, t = F.extract(tsdf, None, S)
    F.closed_surface_checks(v, t)
    assert len(v) == 14                                                         # one vertex on each of the 14 edges at the point
    tsdf[1, 1, 2, 0] = np.nan                                                  # NaN is not inside
    v2, c2, t2 = F.extract(tsdf, None, S)
    assert len(v2) == 14 and np.isfinite(v2).sum() < v2.size


# -- 4. frames of one colour ------------------------------------------------------------------------------------------------------------
def test_frames_of_one_colour_give_that_colour_at_every_vertex():
    S, depth, frames, poses = F.wall_case()
    tsdf, col = F.integrate(*S.empty(), depth, frames, poses, S)
    assert set(map(tuple, col[col[..., 3] > 0][:, :3].tolist())) == {(200.0, 100.0, 50.0)}        # averages of equal integers are exact
    assert col[..., 3].max() == 3
    v, c, t = F.extract(tsdf, col, S)
    assert len(v) > 100 and len(t) > 100 and (c == (200, 100, 50)).all()
    assert np.abs(v[:, 2] - 2.1).max() < 1e-3                                  # the wall


def test_a_vertex_is_white_only_where_an_end_of_its_edge_was_never_painted():
    S, depth, frames, poses = F.integrate_case('plain', cpu_render)
    frames = np.empty_like(frames)
    frames[...] = (200, 100, 50)
    tsdf, col = F.integrate(*S.empty(), depth, frames, poses, S)
    v, c, t = F.extract(tsdf, col, S)
    painted, white = (c == (200, 100, 50)).all(axis=1), (c == 255).all(axis=1)
    assert (painted | white).all() and painted.sum() > len(v) // 2 and white.any()       # seen only from beyond trunc: wc == 0
    col[..., :3] = (200, 100, 50)
    col[..., 3] = 1
    assert (F.extract(tsdf, col, S)[1] == (200, 100, 50)).all()


# -- 5. the exports: present, the ABI number, the build entry, the refusals -----------------------------------------------------------
CAM = DepthCamera()


def _desc(**change):
    ok = dict(dims=(8, 8, 8), origin=(0.0, 0.0, 0.0), voxel=0.05, trunc=0.2, B=1, H=16, W=24, near=0.05, max_weight=64.0,
              min_weight=1.0, camera=CAM)
    ok.update(change)
    return M.fuse_descriptor(ok['camera'], ok['dims'], ok['origin'], ok['voxel'], ok['trunc'], ok['B'], ok['H'], ok['W'],
                             ok['near'], ok['max_weight'], ok['min_weight'])


def _integrate(d, **null):
    lib = _lib.load()
    p = dict(tsdf=0x1000, color=None, depth=0x1000, frames=None, poses=0x1000)
    p.update(null)
    rc = lib.kfn_fuse_integrate(C.byref(d), p['tsdf'], p['color'], p['depth'], p['frames'], p['poses'], None)
    return rc, lib.kfn_last_error().decode()


def test_exports_abi_number_and_build_entry():
    lib = _lib.load()
    assert lib.kfn_abi_version() == 13 and _lib.ABI_VERSION == 13
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ('kfn_fuse_scratch_bytes', 'kfn_fuse_integrate', 'kfn_fuse_extract_count', 'kfn_fuse_extract'):
        assert name in _lib.SYMBOLS and getattr(raw, name) is not None
    hdr = open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()
    assert '#define KFN_ABI_VERSION 13' in hdr and 'typedef struct kfn_fuse_desc {' in hdr
    assert C.sizeof(_lib.FuseDesc) == 104
    from kfnet_amd import build
    assert build.EXTRA['kfn_fuse.hip'] == ['-ffp-contract=off']
    cam = DepthCamera(585.0, 583.0, 317.5, 241.25, depth_fx=570.0, depth_v=250.5)
    d = M.fuse_descriptor(cam, (3, 4, 5), (0.1, 0.2, 0.3), 0.02, 0.08)
    assert (d.nx, d.ny, d.nz) == (3, 4, 5) and d.ox == np.float32(0.1) and d.voxel == np.float32(0.02)
    assert (d.dfx, d.dfy, d.du, d.dv) == (570.0, 583.0, 317.5, 250.5) and (d.fx, d.fy, d.u, d.v) == (585.0, 583.0, 317.5, 241.25)
    assert d.scale == np.float32(0.001) and (d.raw_min, d.raw_max) == (1, 65534)


def test_integrate_argument_checks():
    for change, word in ((dict(dims=(0, 8, 8)), 'positive'), (dict(dims=(8, -1, 8)), 'positive'), (dict(dims=(2048, 1024, 1024)), '2^31'),
                         (dict(B=0), 'positive'), (dict(H=0), 'positive'), (dict(W=-4), 'positive'), (dict(B=70000), '65535'),
                         (dict(voxel=0.0), 'voxel'), (dict(voxel=-1.0), 'voxel'), (dict(trunc=0.0), 'trunc'), (dict(near=0.0), 'near'),
                         (dict(near=-0.5), 'near'), (dict(max_weight=0.5), 'max_weight'), (dict(origin=(np.inf, 0, 0)), 'origin'),
                         (dict(camera=DepthCamera(scale=0.0)), 'scale')):
        rc, msg = _integrate(_desc(**change))
        assert rc == -1 and word in msg, (change, msg)
    for field, value in (('raw_min', -1), ('raw_max', 65536), ('raw_min', 70000)):
        d = _desc()
        setattr(d, field, value)
        rc, msg = _integrate(d)
        assert rc == -1 and 'window' in msg, (field, msg)
    d = _desc()
    d.struct_size -= 4
    rc, msg = _integrate(d)
    assert rc == -1 and 'struct_size' in msg
    for null in ('tsdf', 'depth', 'poses'):
        rc, msg = _integrate(_desc(), **{null: None})
        assert rc == -1 and 'null' in msg
    for pair in (dict(color=0x1000), dict(frames=0x1000)):
        rc, msg = _integrate(_desc(), **pair)
        assert rc == -1 and 'both' in msg
    assert _lib.load().kfn_fuse_integrate(None, 0x1000, None, 0x1000, None, 0x1000, None) == -1
    assert _integrate(_desc(), tsdf=0x1004)[0] == -1 and _integrate(_desc(), color=0x1008, frames=0x1000)[0] == -1


def test_extract_argument_checks_and_scratch_size():
    lib = _lib.load()
    size = C.c_size_t()
    assert lib.kfn_fuse_scratch_bytes(C.byref(_desc(dims=(19, 13, 11))), C.byref(size)) == 0
    n = 19 * 13 * 11
    assert size.value == 8 * n + 16 * 3 + (n + 7) // 8 * 8                  # 2717 points: levels of 3 and 1 block
    assert lib.kfn_fuse_scratch_bytes(C.byref(_desc(dims=(128, 128, 65))), C.byref(size)) == 0
    n = 128 * 128 * 65
    assert size.value == 8 * n + 16 * (1040 + 2) + n
    assert lib.kfn_fuse_scratch_bytes(C.byref(_desc(dims=(1, 1, 1))), C.byref(size)) == 0 and size.value == 8 + 8
    assert lib.kfn_fuse_scratch_bytes(C.byref(_desc(dims=(0, 1, 1))), C.byref(size)) == -1
    assert lib.kfn_fuse_scratch_bytes(C.byref(_desc()), None) == -1

    def count(d, tsdf=0x1000, scratch=0x1000, totals=0x1000):
        return lib.kfn_fuse_extract_count(C.byref(d), tsdf, scratch, totals, None), lib.kfn_last_error().decode()

    def emit(d, tsdf=0x1000, color=None, scratch=0x1000, vertices=0x1000, colors=0x1000, triangles=0x1000, cv=4, ct=4):
        return (lib.kfn_fuse_extract(C.byref(d), tsdf, color, scratch, vertices, colors, triangles, cv, ct, None),
                lib.kfn_last_error().decode())
    for call in (count, emit):
        for change, word in ((dict(min_weight=0.5), 'min_weight'), (dict(min_weight=np.nan), 'min_weight'), (dict(voxel=0.0), 'voxel'),
                             (dict(dims=(8, 8, 0)), 'positive'), (dict(dims=(2048, 1024, 1024)), '2^31')):
            rc, msg = call(_desc(**change))
            assert rc == -1 and word in msg, (change, msg)
        d = _desc()
        d.struct_size += 4
        assert call(d)[0] == -1
    for null in ('tsdf', 'scratch', 'totals'):
        rc, msg = count(_desc(), **{null: None})
        assert rc == -1 and 'null' in msg
    for null in ('tsdf', 'scratch', 'vertices', 'triangles'):
        rc, msg = emit(_desc(), **{null: None})
        assert rc == -1 and 'null' in msg
    for cap in (dict(cv=-1), dict(ct=-1), dict(cv=1 << 31), dict(ct=1 << 40)):
        rc, msg = emit(_desc(), **cap)
        assert rc == -1 and 'capacities' in msg


# -- 6. the module's and the program's refusals, before torch touches a device ---------------------------------------------------------
def test_volume_and_box_refusals():
    for args, word in ((((0, 4, 4), (0, 0, 0), 0.1), 'empty'), (((2048, 1024, 1024), (0, 0, 0), 0.1), 'int32'),
                       (((4, 4, 4), (0, 0, 0), 0.0), 'voxel'), (((4, 4, 4), (0, 0, 0), 0.1, -1.0), 'trunc')):
        with pytest.raises(ValueError) as e:
            M.Volume(*args)
        assert word in str(e.value)
    for kw, word in ((dict(batch=0), 'batch'), (dict(max_weight=0.0), 'max_weight'), (dict(near=0.0), 'near'), (dict(image_size=(0, 4)), 'size')):
        with pytest.raises(ValueError) as e:
            M.Volume((4, 4, 4), (0, 0, 0), 0.1, **kw)
        assert word in str(e.value)
    assert M.box_lattice((0, 0, 0), (1, 0.5, 0.26), 0.25) == ((5, 3, 3), (0.0, 0.0, 0.0))
    for lo, hi in (((0, 0, 0), (1, 0, 1)), ((0, 0, 0), (1, -1, 1)), ((0, 0, np.nan), (1, 1, 1))):
        with pytest.raises(ValueError) as e:
            M.box_lattice(lo, hi, 0.1)
        assert 'empty' in str(e.value)


def test_fuse_make_argument_errors(tmp_path, capsys):
    out = str(tmp_path / 'scene.ply')
    seq = tmp_path / 'seq'
    seq.mkdir()
    ok = ['make', '--sequence', str(seq), '--output', out]
    for args, word in ((['make', '--output', out], '--sequence'), (['make', '--sequence', str(seq)], '--output'),
                       (ok + ['--batch', '0'], '--batch'), (ok + ['--every', '0'], '--every'), (ok + ['--voxel', '0'], '--voxel'),
                       (ok + ['--trunc', '-1'], '--trunc'), (ok + ['--min_weight', '0.5'], '--min_weight'),
                       (ok + ['--height', '100'], 'multiples of 8'), (ok + ['--focal_x', '-3'], 'positive'),
                       (ok, 'holds no frame-*.color.png'),
                       (['make', '--sequence', str(tmp_path / 'nowhere'), '--output', out], 'nowhere is not a folder')):
        assert M.main(args) == 1, args
        assert word in capsys.readouterr().err, args
    # a sequence that is there: the box and the volume's size are refused before a device is touched
    for k in range(2):
        for name in ('color.png', 'depth.png'):
            (seq / ('frame-%06d.%s' % (k, name))).write_bytes(b'')
        np.savetxt(str(seq / ('frame-%06d.pose.txt' % k)), np.eye(4))
    for args, word in ((ok + ['--bounds', '0', '0', '0', '1', '0', '1'], 'the box is empty'),
                       (ok + ['--bounds', '0', '0', '0', '40', '40', '40', '--voxel', '0.02'], 'do not fit int32')):
        assert M.main(args) == 1, args
        err = capsys.readouterr().err
        assert word in err and len(err.strip().split('\n')) == 1, err
    (seq / 'frame-000001.pose.txt').unlink()
    assert M.main(ok) == 1 and 'frame-000001.pose.txt is missing' in capsys.readouterr().err
    assert M.main([]) == 1
    assert not os.path.exists(out)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'kfnet_amd.fuse', 'make', '--output', out], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 1 and '--sequence' in r.stderr and len(r.stderr.strip().split('\n')) == 1
    r = subprocess.run([sys.executable, '-m', 'kfnet_amd.fuse', 'make', '--help'], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ('--sequence', '--output', '--voxel', '--trunc', '--bounds', '--min_weight', '--every', '--no_color', '--batch', '--gpu',
                 '--depth_focal_x', '--depth_v', '--focal_x'):
        assert flag in r.stdout, flag
