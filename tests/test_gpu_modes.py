"""The single-network programs on the device: kfn_coord_records / kfn_flow_records bit for bit,
SCoordNetEngine / OFlowNetEngine against KFNetEngine and the fp64 oracle, scope-only weight containers, chunk and batch
independence, and the two command lines (single process and frame-sharded)."""
import ctypes as C
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import dev, stream, sync
from kfnet_amd import _lib
from oracle import kfnet_oracle as O
from test_modes_host import coord_records_ref, flow_records_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SIZE = (64, 96)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope='module')
def gold():
    from kfnet_amd.weights import synthetic_weights
    z = np.load(os.path.join(HERE, 'golden', 'kfnet_small.npz'))
    return z, synthetic_weights(int(z['seed_w']))


@pytest.fixture(scope='module')
def seq():
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    return synthetic_sequence(9, SIZE[0], SIZE[1], seed=1), np.linalg.inv(synthetic_transform()).astype(np.float32)


def _scan_reset_records(meas, transform, h, w):
    """What kfn_kalman_scan (KFNetEngine's scan, no debug outputs) emits when every frame is a reset: meas [T,h,w,4]."""
    import torch
    lib = _lib.load()
    T = meas.shape[0]
    d = _lib.KalmanDesc(S=1, T=T, H=h, W=w, t0=0, reset_period=1, min_uncertainty=1e-5, nis_gate=0.0,
                        has_transform=int(transform is not None))
    if transform is not None:
        for i, v in enumerate(np.asarray(transform, np.float32)[:3, :4].reshape(-1)):
            d.transform[i] = float(v)
    need = C.c_size_t(0)
    _lib.check(lib.kfn_kalman_scan_scratch_bytes(C.byref(d), C.byref(need)), 'scratch bytes')
    scratch = torch.empty(max(need.value // 4, 1), device='cuda')
    flow = torch.zeros(T * h * w * 2, device='cuda')
    sig = torch.ones(T * h * w, device='cuda')
    st = torch.zeros(h * w * 4, device='cuda')
    rec = torch.zeros(T * h * w * 4, device='cuda')
    dm = dev(meas)
    _lib.check(lib.kfn_kalman_scan(C.byref(d), flow.data_ptr(), sig.data_ptr(), dm.data_ptr(), st.data_ptr(),
                                   rec.data_ptr(), None, None, scratch.data_ptr() if need.value else None, stream()), 'scan')
    sync()
    return rec.cpu().numpy().reshape(T, h, w, 4)


def _coord_records(meas_strided, ld, transform, P):
    import torch
    lib = _lib.load()
    t12 = None if transform is None else (C.c_float * 12)(*[float(v) for v in np.asarray(transform, np.float32)[:3, :4].reshape(-1)])
    dm = dev(meas_strided)
    out = torch.full((P * 4,), float('nan'), device='cuda')
    _lib.check(lib.kfn_coord_records(dm.data_ptr(), ld, t12, out.data_ptr(), P, stream()), 'kfn_coord_records')
    sync()
    return out.cpu().numpy().reshape(P, 4)


def _edge_meas(rng, T, h, w):
    m = rng.normal(scale=3.0, size=(T, h, w, 4)).astype(np.float32)
    m[..., 3] = np.abs(m[..., 3]) + 0.01
    flat = m.reshape(-1, 4)
    edge = np.array([1e-30, 1e-20, 1e-5, 2.0 ** -96, 1.0, 3.0, 7.0, 1e5, 1e20, 1e30, 3e38], np.float32)
    flat[:edge.size, 3] = edge                                   # tiny and huge sigma
    flat[edge.size:edge.size + 4, :3] = [[1e30, -1e30, 0.0], [0.0, -0.0, 1e-30], [65504.0, 1e-7, -3.5], [1e8, 1e8, 1e8]]
    return m


@pytest.mark.parametrize('use_t', [False, True])
@pytest.mark.parametrize('ld', [4, 7])
@pytest.mark.parametrize('hw', [(8, 12), (60, 80)])
def test_coord_records_equal_the_scan_on_reset_frames(seq, use_t, ld, hw):
    _, T4 = seq
    rng = np.random.default_rng(ld + 10 * use_t + hw[0])
    h, w = hw
    T = 3
    meas = _edge_meas(rng, T, h, w)
    want = _scan_reset_records(meas, T4 if use_t else None, h, w)
    P = T * h * w
    strided = np.full((P, ld), np.float32(-7.0), np.float32)
    strided[:, :4] = meas.reshape(P, 4)
    got = _coord_records(strided, ld, T4 if use_t else None, P)
    assert np.array_equal(got.view(np.uint32), want.reshape(P, 4).view(np.uint32))
    # the numpy statement: T.x exactly, 1/sigma correctly rounded where sigma and 1/sigma are normal-range operands
    ref = coord_records_ref(meas.reshape(P, 4), T4 if use_t else None)
    assert np.array_equal(got[:, :3], ref[:, :3])
    sg = meas.reshape(P, 4)[:, 3]
    normal = (sg >= np.float32(2.0 ** -96)) & (sg <= np.float32(2.0 ** 96))
    assert np.array_equal(got[normal, 3], ref[normal, 3])


def test_flow_records_are_bit_exact():
    import torch
    lib = _lib.load()
    rng = np.random.default_rng(3)
    P = 5000
    flow = rng.normal(scale=4.0, size=(P, 2)).astype(np.float32)
    sig = np.abs(rng.normal(size=P)).astype(np.float32) * 10.0 ** rng.integers(-6, 6, size=P).astype(np.float32)
    sig[:8] = [1e-40, 1e-38, 1e-30, 0.0, 1e30, 3e38, np.inf, -2.5]
    out = torch.full((P * 3,), float('nan'), device='cuda')
    df, ds = dev(flow), dev(sig)
    _lib.check(lib.kfn_flow_records(df.data_ptr(), ds.data_ptr(), out.data_ptr(), P, stream()), 'kfn_flow_records')
    sync()
    got = out.cpu().numpy().reshape(P, 3)
    with np.errstate(divide='ignore', over='ignore'):
        want = flow_records_ref(flow, sig)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize('batch', [1, 2])
def test_scoordnet_engine_equals_kfnet_with_every_frame_a_reset(gold, batch):
    from kfnet_amd.engine import KFNetEngine, SCoordNetEngine
    z, W = gold
    imgs, T4 = z['images'], z['transform']
    kf = KFNetEngine(W, image_size=SIZE, batch=batch, transform=T4, reset_period=1, max_chunk=8)
    want = kf.process(kf.upload_frames(imgs)).cpu().numpy()
    eng = SCoordNetEngine(W, image_size=SIZE, batch=batch, transform=T4, max_chunk=8)
    got = eng.process(eng.upload_frames(imgs)).cpu().numpy()
    assert got.shape == (5, 8, 12, 4)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_oflownet_engine_equals_kfnet_flow_and_the_oracle(seq):
    from kfnet_amd.engine import KFNetEngine, OFlowNetEngine
    from kfnet_amd.weights import synthetic_weights
    imgs, T4 = seq
    W = synthetic_weights(1234)
    T = imgs.shape[0]
    kf = KFNetEngine(W, image_size=SIZE, batch=4, transform=T4, reset_period=500, max_chunk=16, emit_debug=True)
    kf.process(kf.upload_frames(imgs))
    d = kf.debug(T)
    eng = OFlowNetEngine(W, image_size=SIZE, batch=4, max_chunk=16)
    rec = eng.process(eng.upload_frames(imgs)).cpu().numpy()
    e = eng.debug(T)
    assert rec.shape == (T, 8, 12, 3)
    assert np.array_equal(e['flow'][1:].view(np.uint32), d['flow'][1:].view(np.uint32))
    assert np.array_equal(e['sigma_trans'][1:].view(np.uint32), d['sigma_trans'][1:].view(np.uint32))
    assert np.array_equal(rec[1:].view(np.uint32), flow_records_ref(e['flow'], e['sigma_trans'])[1:].view(np.uint32))
    _, dbg = O.eval_sequence(imgs, W, O.get_transform(np.eye(4)), reset_period=1000, dtype=np.float64, return_debug=True)
    for t in range(1, T):
        assert np.abs(rec[t, ..., :2] - dbg[t]['flow'][0]).max() < 5e-5
        assert np.abs(e['sigma_trans'][t].reshape(-1) - dbg[t]['sigma_trans'].reshape(-1)).max() < 1e-6


def test_scope_only_containers_drive_their_engine(seq):
    from kfnet_amd.engine import OFlowNetEngine, SCoordNetEngine
    from kfnet_amd.weights import synthetic_weights
    imgs, T4 = seq
    W = synthetic_weights(1234)
    score = {k: v for k, v in W.items() if k.startswith('ScoreNet/')}
    temporal = {k: v for k, v in W.items() if k.startswith('Temporal/')}
    outs = {}
    for name, cls, kw, part in (('s', SCoordNetEngine, dict(transform=T4), score), ('o', OFlowNetEngine, {}, temporal)):
        for which, Wc in (('full', W), ('scope', part)):
            eng = cls(Wc, image_size=SIZE, batch=2, max_chunk=9, **kw)
            outs[name, which] = eng.process(eng.upload_frames(imgs)).cpu().numpy()
            assert set(p.source for p in eng.graph.params.values()) <= set(part)
        assert np.array_equal(outs[name, 'full'], outs[name, 'scope'])
    broken = dict(score)
    del broken['ScoreNet/conv4b/kernel']
    with pytest.raises(KeyError, match='ScoreNet/conv4b/kernel'):
        SCoordNetEngine(broken, image_size=SIZE, batch=2, max_chunk=4)
    broken = dict(temporal)
    del broken['Temporal/uncertainty/bias']
    with pytest.raises(KeyError, match='Temporal/uncertainty/bias'):
        OFlowNetEngine(broken, image_size=SIZE, batch=2, max_chunk=4)
    with pytest.raises(KeyError):
        OFlowNetEngine(score, image_size=SIZE, batch=2, max_chunk=4)


def _root_tensors(g):
    out = set()
    for op in g.ops:
        for _, t in g._tensor_refs(op):
            while t.base is not None:
                t = t.base
            out.add((t.name, tuple(t.shape)))
    return out


def test_engines_do_not_allocate_the_other_network():
    from kfnet_amd.engine import KFNetEngine, OFlowNetEngine, SCoordNetEngine
    from kfnet_amd.weights import synthetic_weights
    W = synthetic_weights(1234)
    s = SCoordNetEngine(W, image_size=SIZE, batch=2, max_chunk=4)
    o = OFlowNetEngine(W, image_size=SIZE, batch=2, max_chunk=4)
    k = KFNetEngine(W, image_size=SIZE, batch=2, max_chunk=4)
    assert all(n.startswith('ScoreNet/') for n in s.graph.params)
    assert all(n.startswith('Temporal/') for n in o.graph.params)
    s_names = {n for n, _ in _root_tensors(s.graph)}
    assert not any(n and (n.startswith('feat') or n in ('flow', 'uncertainty', 'conv0_T')) for n in s_names)
    o_names = {n for n, _ in _root_tensors(o.graph)}
    assert not ({'conv4a', 'conv4b', 'conv7', 'prediction'} & o_names)
    assert not any(shape == (2,) + SIZE + (64,) for _, shape in _root_tensors(o.graph))    # SCoordNet's conv1a / conv1b
    allocated = lambda e: sum(st.numel for st in e.graph.storages)
    assert allocated(s) < allocated(k) and allocated(o) < allocated(k)


@pytest.mark.parametrize('kind', ['coord', 'flow'])
def test_chunk_and_batch_independence(seq, kind):
    """Bit for bit: how a sequence is cut into process() calls (partial batches included), and a second engine primed with
    the frame before its chunk.  Across tower batch sizes the convolution routes differ (split-K and the Winograd forms are
    chosen by launch size, as for KFNetEngine), so batch 1 and batch 4 agree within the records' tolerance, not bit for bit."""
    from kfnet_amd.engine import OFlowNetEngine, SCoordNetEngine
    from kfnet_amd.weights import synthetic_weights
    imgs, T4 = seq
    W = synthetic_weights(1234)
    T = imgs.shape[0]

    def make(batch, chunk):
        if kind == 'coord':
            return SCoordNetEngine(W, image_size=SIZE, batch=batch, transform=T4, max_chunk=chunk)
        return OFlowNetEngine(W, image_size=SIZE, batch=batch, max_chunk=chunk)
    e4 = make(4, T)
    four = e4.process(e4.upload_frames(imgs)).cpu().numpy()
    # split over two process() calls of one engine (the feature ring carries over) ...
    es = make(4, 5)
    a = es.process(es.upload_frames(imgs[:5]), t0=0).cpu().numpy().copy()
    b = es.process(es.upload_frames(imgs[5:]), t0=5).cpu().numpy().copy()
    # ... and a second engine primed with the frame before its chunk (what a rank r > 0 does)
    ep = make(4, 4)
    ep.prime(ep.upload_frames(imgs[4:5])[0])
    c = ep.process(ep.upload_frames(imgs[5:]), t0=5).cpu().numpy()
    lo = 1 if kind == 'flow' else 0                # row 0 of a flow sequence has no predecessor
    for got in (np.concatenate([a, b]), np.concatenate([a, c])):
        assert np.array_equal(got[lo:].view(np.uint32), four[lo:].view(np.uint32))
    e1 = make(1, T)
    one = e1.process(e1.upload_frames(imgs)).cpu().numpy()
    ch = 3 if kind == 'coord' else 2
    assert np.abs(one[lo:, ..., :ch] - four[lo:, ..., :ch]).max() <= 1e-4
    assert (np.abs(one[lo:, ..., ch] - four[lo:, ..., ch]) / np.abs(four[lo:, ..., ch])).max() <= 1e-4


def test_full_size_runs_of_both_engines():
    from kfnet_amd.engine import KFNetEngine, OFlowNetEngine, SCoordNetEngine
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    from kfnet_amd.weights import synthetic_weights
    W = synthetic_weights(1234)
    imgs = synthetic_sequence(3, 480, 640, seed=1)
    T4 = np.linalg.inv(synthetic_transform())
    kf = KFNetEngine(W, image_size=(480, 640), batch=4, transform=T4, reset_period=1, max_chunk=3, emit_debug=True)
    krec = kf.process(kf.upload_frames(imgs)).cpu().numpy()
    s = SCoordNetEngine(W, image_size=(480, 640), batch=4, transform=T4, max_chunk=3)
    srec = s.process(s.upload_frames(imgs)).cpu().numpy()
    assert srec.shape == (3, 60, 80, 4) and np.isfinite(srec).all()
    assert np.array_equal(srec, krec)
    del s
    o = OFlowNetEngine(W, image_size=(480, 640), batch=4, max_chunk=3)
    orec = o.process(o.upload_frames(imgs)).cpu().numpy()
    d = kf.debug(3)
    assert orec.shape == (3, 60, 80, 3) and np.isfinite(orec[1:]).all()
    assert np.array_equal(orec[1:, ..., :2], d['flow'][1:])
    assert np.array_equal(orec[1:, ..., 2], np.float32(1) / d['sigma_trans'][1:, ..., 0])


# -- command lines ------------------------------------------------------------------------------------------------------
def _env(**kw):
    e = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT'):
        e.pop(k, None)
    e['PYTHONPATH'] = ROOT + os.pathsep + e.get('PYTHONPATH', '')
    e.update(kw)
    return e


def _cli(module, args, timeout=600):
    r = subprocess.run([sys.executable, '-m', module] + args, cwd=ROOT, env=_env(), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def _sharded(module, args, world=2, timeout=900):
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world),
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port()), '-m', module] + args
    r = subprocess.run(cmd, cwd=ROOT, env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


SMALL = ['--random_weights', '--height', '64', '--width', '96', '--batch', '2']


def test_scoordnet_cli_writes_records_and_poses(tmp_path):
    from kfnet_amd.engine import SCoordNetEngine
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    from kfnet_amd.weights import synthetic_weights
    out = tmp_path / 'o'
    out.mkdir()
    _cli('kfnet_amd.SCoordNet.eval', ['--scene', 'heads', '--synthetic', '6', '--output_folder', str(out), '--pose'] + SMALL)
    names = sorted(os.listdir(str(out)))
    assert names == sorted(['coord_%d.npy' % i for i in range(6)] + ['pose_%d.txt' % i for i in range(6)])
    eng = SCoordNetEngine(synthetic_weights(1234), image_size=SIZE, batch=2, transform=np.linalg.inv(synthetic_transform()),
                          max_chunk=6)
    want = eng.process(eng.upload_frames(synthetic_sequence(6, 64, 96))).cpu().numpy()
    got = np.stack([np.load(str(out / ('coord_%d.npy' % i))) for i in range(6)])
    assert got.dtype == np.float32 and np.array_equal(got, want)
    pose = np.loadtxt(str(out / 'pose_0.txt'))
    assert pose.shape == (4, 4)


def test_oflownet_cli_writes_flows_and_flow_list(tmp_path):
    from kfnet_amd.engine import OFlowNetEngine
    from kfnet_amd.synth import synthetic_sequence
    from kfnet_amd.weights import synthetic_weights
    out = tmp_path / 'o'
    out.mkdir()
    _cli('kfnet_amd.OFlowNet.eval', ['--synthetic', '7', '--output_folder', str(out)] + SMALL)
    assert sorted(os.listdir(str(out))) == sorted(['flow_%d.npy' % i for i in range(1, 7)] + ['flow_list.txt'])
    lines = open(str(out / 'flow_list.txt')).read().splitlines()
    assert lines == [os.path.join(str(out.resolve()), 'flow_%d.npy' % i) for i in range(1, 7)]
    eng = OFlowNetEngine(synthetic_weights(1234), image_size=SIZE, batch=2, max_chunk=7)
    want = eng.process(eng.upload_frames(synthetic_sequence(7, 64, 96))).cpu().numpy()
    got = np.stack([np.load(l) for l in lines])
    assert got.shape == (6, 8, 12, 3) and np.array_equal(got, want[1:])


def _write_dataset(folder, T, rng):
    from PIL import Image
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    imgs = synthetic_sequence(T, 64, 96, seed=2)
    paths, labels = [], []
    for i in range(T):
        p = os.path.join(folder, 'frame_%d.png' % i)
        Image.fromarray(imgs[i]).save(p)
        paths.append(p)
        lab = np.empty((64, 96, 4), np.float32)
        lab[..., :3] = rng.normal(scale=0.5, size=(64, 96, 3))
        lab[..., 3] = (rng.random((64, 96)) < 0.8).astype(np.float32)
        lp = os.path.join(folder, 'label_%d.bin' % i)
        lab.tofile(lp)
        labels.append(lp)
    for name, lines in (('image_list.txt', paths), ('label_list.txt', labels)):
        with open(os.path.join(folder, name), 'w') as f:
            f.write('\n'.join(lines) + '\n')
    np.savetxt(os.path.join(folder, 'transform.txt'), synthetic_transform())


def test_scoordnet_cli_dist_errors_equal_kfnet_measurement_column(tmp_path):
    inp = tmp_path / 'in'
    inp.mkdir()
    _write_dataset(str(inp), 6, np.random.default_rng(5))
    args = ['--input_folder', str(inp), '--scene', 'heads'] + SMALL
    s_out = _cli('kfnet_amd.SCoordNet.eval', args)
    k_out = _cli('kfnet_amd.KFNet.eval', args)
    s_dm = {int(m.group(1)): m.group(2) for m in re.finditer(r'^(\d+), frame \d+, d_m = ([-\d.na]+)$', s_out, re.M)}
    k_dm = {int(m.group(1)): m.group(2) for m in re.finditer(r'^(\d+), frame \d+~\d+, .*?d_m = ([-\d.na]+),', k_out, re.M)}
    assert sorted(s_dm) == list(range(6)) and sorted(k_dm) == list(range(6))
    assert s_dm == k_dm
    for name in ('Median dist error: ', 'Mean dist error: ', 'stddev error: '):
        s_line = [l for l in s_out.splitlines() if l.startswith(name)]
        k_line = [l for l in k_out.splitlines() if l.startswith(name)]
        assert len(s_line) == 1 and len(k_line) == 1
        assert s_line[0].split()[-1] == k_line[0][len(name):].split()[0]       # the measurement column


@pytest.mark.parametrize('module,kind', [('kfnet_amd.SCoordNet.eval', 'coord'), ('kfnet_amd.OFlowNet.eval', 'flow')])
def test_two_rank_run_equals_single_process(tmp_path, module, kind):
    one, two = tmp_path / 'one', tmp_path / 'two'
    one.mkdir()
    two.mkdir()
    extra = ['--scene', 'heads'] if kind == 'coord' else []
    _cli(module, ['--synthetic', '9', '--output_folder', str(one)] + extra + SMALL)
    out = _sharded(module, ['--synthetic', '9', '--output_folder', str(two)] + extra + SMALL)
    assert 'rank 0/2: frames 0~4 done' in out and 'rank 1/2: frames 5~8 done' in out
    names = sorted(f for f in os.listdir(str(one)) if f.endswith('.npy'))
    assert names == sorted(f for f in os.listdir(str(two)) if f.endswith('.npy'))
    assert len(names) == (9 if kind == 'coord' else 8)
    for n in names:
        assert np.array_equal(np.load(str(one / n)), np.load(str(two / n))), n
    if kind == 'flow':
        assert (open(str(one / 'flow_list.txt')).read().replace(str(one.resolve()), '')
                == open(str(two / 'flow_list.txt')).read().replace(str(two.resolve()), ''))
