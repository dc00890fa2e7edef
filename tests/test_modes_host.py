"""CPU tests of the single-network programs (SCoordNet/eval.py, OFlowNet/eval.py): command lines, file
names, weight scopes, the numpy statement of both record formats, and the C surface of kfn_coord_records /
kfn_flow_records (ABI 12) with its argument checks."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from kfnet_amd import _lib, modes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def coord_records_ref(meas, transform=None):
    """numpy statement of kfn_coord_records: T.x with ((M0 x + M1 y) + M2 z) + M3 in float32, then 1/sigma."""
    m = np.asarray(meas, np.float32)
    x, y, z, s = m[..., 0], m[..., 1], m[..., 2], m[..., 3]
    if transform is None:
        out = [x, y, z]
    else:
        M = np.asarray(transform, np.float32)
        out = [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)]
    return np.stack(out + [np.float32(1) / s], -1).astype(np.float32)


def flow_records_ref(flow, sigma):
    f = np.asarray(flow, np.float32)
    s = np.asarray(sigma, np.float32).reshape(f.shape[:-1])
    return np.stack([f[..., 0], f[..., 1], np.float32(1) / s], -1)


def _run(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    e['PYTHONPATH'] = ROOT + os.pathsep + e.get('PYTHONPATH', '')
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, timeout=300)


def test_clis_parse_the_reference_flags():
    from kfnet_amd.OFlowNet import eval as oe
    from kfnet_amd.SCoordNet import eval as se
    a = se.build_parser().parse_args(['--input_folder', 'I', '--output_folder', 'O', '--model_folder', 'M', '--scene',
                                      'fire', '--synthetic', '3', '--random_weights', '--batch', '2', '--height', '64',
                                      '--width', '96', '--gpu', '1', '--pose'])
    assert (a.input_folder, a.output_folder, a.model_folder, a.scene) == ('I', 'O', 'M', 'fire')
    assert (a.synthetic, a.random_weights, a.batch, a.height, a.width, a.gpu, a.pose) == (3, True, 2, 64, 96, 1, True)
    a = oe.build_parser().parse_args(['--input_folder', 'I', '--output_folder', 'O', '--model_folder', 'M'])
    assert (a.input_folder, a.output_folder, a.model_folder) == ('I', 'O', 'M')
    assert (a.synthetic, a.random_weights, a.batch, a.height, a.width, a.gpu) == (0, False, 4, 480, 640, 0)
    with pytest.raises(SystemExit):
        oe.build_parser().parse_args(['--scene', 'fire'])      # the reference's OFlowNet command has no scene
    for mod, flags in (('kfnet_amd.SCoordNet.eval', ('--input_folder', '--output_folder', '--model_folder', '--scene',
                                                      '--pose', '--synthetic')),
                       ('kfnet_amd.OFlowNet.eval', ('--input_folder', '--output_folder', '--model_folder', '--synthetic'))):
        r = _run(['-m', mod, '--help'])
        assert r.returncode == 0, r.stdout
        for f in flags:
            assert f in r.stdout, (mod, f)


def test_scoordnet_cli_refuses_bad_scene_and_sharded_pose(tmp_path):
    r = _run(['-m', 'kfnet_amd.SCoordNet.eval', '--scene', 'nowhere', '--random_weights', '--synthetic', '2'])
    assert r.returncode == 1 and 'Invalid scene' in r.stdout
    r = _run(['-m', 'kfnet_amd.SCoordNet.eval', '--scene', 'chess', '--synthetic', '4', '--random_weights', '--pose',
              '--output_folder', str(tmp_path)], env={'WORLD_SIZE': '2', 'RANK': '0'})
    assert r.returncode == 2 and '--pose is not supported in the sharded run' in r.stdout
    assert os.listdir(str(tmp_path)) == []


def test_file_names_and_flow_list(tmp_path):
    assert modes.output_files('coord', 3, 2) == [(3, 'coord_3.npy'), (4, 'coord_4.npy')]
    assert modes.output_files('flow', 0, 3) == [(1, 'flow_1.npy'), (2, 'flow_2.npy')]     # frame 0 has no predecessor
    assert modes.output_files('flow', 5, 2) == [(5, 'flow_5.npy'), (6, 'flow_6.npy')]
    assert modes.output_files('flow', 0, 1) == []
    with pytest.raises(ValueError):
        modes.output_files('pose', 0, 1)
    path = modes.write_flow_list(str(tmp_path), 4)
    lines = open(path).read().splitlines()
    assert os.path.basename(path) == 'flow_list.txt'
    assert lines == [os.path.join(str(tmp_path.resolve()), 'flow_%d.npy' % i) for i in (1, 2, 3)]
    rec = np.arange(3 * 2 * 2 * 3, dtype=np.float32).reshape(3, 2, 2, 3)
    modes.save_records(str(tmp_path), 'flow', 0, rec)
    assert sorted(f for f in os.listdir(str(tmp_path)) if f.endswith('.npy')) == ['flow_1.npy', 'flow_2.npy']
    got = np.load(str(tmp_path / 'flow_2.npy'))
    assert got.dtype == np.float32 and np.array_equal(got, rec[2])


def test_weight_scopes():
    from kfnet_amd.engine import check_weights, network_variables
    from kfnet_amd.weights import synthetic_weights
    W = synthetic_weights(1234)
    sc = network_variables('scoordnet', (64, 96), 2)
    of = network_variables('oflownet', (64, 96), 2)
    assert sc and all(n.startswith('ScoreNet/') for n in sc)
    assert of and all(n.startswith('Temporal/') for n in of)
    # the two engines together need exactly what a full KFNet container holds
    assert sorted(sc + of) == sorted(W)
    assert 'Temporal/feat1/kernel' in of and 'Temporal/uncertainty/kernel' in of and 'Temporal/upconv0/kernel' in of
    score_only = {k: v for k, v in W.items() if k.startswith('ScoreNet/')}
    temporal_only = {k: v for k, v in W.items() if k.startswith('Temporal/')}
    check_weights(score_only, sc)
    check_weights(temporal_only, of)
    check_weights(W, sc)
    check_weights(W, of)
    with pytest.raises(KeyError):
        check_weights(temporal_only, sc)
    with pytest.raises(KeyError):
        check_weights(score_only, of)
    for names, scope in ((sc, score_only), (of, temporal_only)):
        for missing in (names[0], names[-1]):
            partial = dict(scope)
            del partial[missing]
            with pytest.raises(KeyError, match=re.escape(missing)):
                check_weights(partial, names)


def test_single_tower_graphs_hold_only_their_network():
    from kfnet_amd.engine import _single_network
    from kfnet_amd.graph import Graph
    from kfnet_amd.KFNet.KFNet import KFNet, KFNetDataSpec
    spec = KFNetDataSpec(batch_size=2, image_size=(64, 96))
    g = Graph()
    net = _single_network(g, g.placeholder((2, 64, 96, 3), 'u8'), spec, 'scoordnet')
    assert net.temp_feat_maps is None and net.scoordnet is not None
    assert [op.name for op in g.ops][0] == 'first_conv[conv1a]'
    assert all(not n.startswith('Temporal/') for n in g.params)
    g = Graph()
    net = _single_network(g, g.placeholder((2, 64, 96, 3), 'u8'), spec, 'oflownet')
    assert net.scoordnet is None and net.pair_ops
    assert [op.name for op in g.ops][0] == 'first_conv[feat1]'
    assert all(not n.startswith('ScoreNet/') for n in g.params)
    with pytest.raises(ValueError):
        KFNet(g.placeholder((2, 64, 96, 3), 'u8'), spec, towers=('kalman',))


def test_record_formats_in_numpy():
    rng = np.random.default_rng(0)
    meas = rng.normal(size=(5, 4)).astype(np.float32)
    meas[:, 3] = np.abs(meas[:, 3]) + 0.1
    T4 = np.eye(4, dtype=np.float32)
    T4[:3, 3] = (1.0, -2.0, 0.5)
    r = coord_records_ref(meas, T4)
    assert r.dtype == np.float32 and r.shape == (5, 4)
    assert np.array_equal(r[:, :3], meas[:, :3] + T4[:3, 3])
    assert np.array_equal(r[:, 3], np.float32(1) / meas[:, 3])
    assert np.array_equal(coord_records_ref(meas)[:, :3], meas[:, :3])
    flow = rng.normal(size=(5, 2)).astype(np.float32)
    sig = np.abs(rng.normal(size=(5, 1))).astype(np.float32)
    f = flow_records_ref(flow, sig)
    assert f.shape == (5, 3) and np.array_equal(f[:, :2], flow) and np.array_equal(f[:, 2], np.float32(1) / sig[:, 0])


def test_abi12_exports_the_record_entry_points_and_checks_arguments():
    assert _lib.ABI_VERSION == 13
    hdr = open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()
    assert '#define KFN_ABI_VERSION 13' in hdr
    assert 'kfn_abi_version() == 13' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    lib = _lib.load()
    assert lib.kfn_abi_version() == 13
    for name in ('kfn_coord_records', 'kfn_flow_records'):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    d16, d4 = C.c_void_p(64), C.c_void_p(68)        # never dereferenced: every call below fails its checks first
    t12 = (C.c_float * 12)()
    bad = [(None, 4, t12, d16, 10), (d16, 4, t12, None, 10), (d16, 4, None, d16, 0), (d16, 4, None, d16, -5),
           (d16, 3, None, d16, 10), (d16, 0, t12, d16, 10), (d16, 4, None, d4, 10), (C.c_void_p(66), 4, None, d16, 10)]
    for meas, ld, tr, out, P in bad:
        assert lib.kfn_coord_records(meas, ld, tr, out, P, None) == -1, (meas, ld, out, P)
    assert b'kfn_coord_records' in lib.kfn_last_error()
    bad = [(None, d4, d4, 10), (d4, None, d4, 10), (d4, d4, None, 10), (d4, d4, d4, 0), (d4, d4, d4, -1),
           (C.c_void_p(66), d4, d4, 10), (d4, d4, C.c_void_p(70), 10)]
    for flow, sig, out, P in bad:
        assert lib.kfn_flow_records(flow, sig, out, P, None) == -1, (flow, sig, out, P)
    assert b'kfn_flow_records' in lib.kfn_last_error()


def test_new_sources_have_no_build_switches():
    cond = re.compile(r'^\s*#\s*(if|ifdef|ifndef|elif)\b.*\bKFN_.*$', re.M)
    text = open(os.path.join(ROOT, 'kfnet_amd', 'csrc', 'kfn_util_ops.hip')).read()
    assert 'coord_records_kernel' in text and 'flow_records_kernel' in text
    assert not cond.findall(text)
