"""-m gpu: the three test programs restore their weights straight from TF V2 checkpoints in --model_folder
(kfnet_amd/checkpoint.py; the reference's get_snapshot + RestoreFromScope, tools/io.py:185-196, KFNet/eval.py:66-68).

The checkpoints are written by tests/tf_bundle_writer.py.  A run from a checkpoint must write the same bits as a run from
the equivalent .npz container, and a corrupt tensor must stop the program before it writes anything."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytest.importorskip('google.protobuf')

import tf_bundle_writer as TW  # noqa: E402
from oracle import kfnet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W_, T = 64, 96, 5
SMALL = ['--height', str(H), '--width', str(W_), '--batch', '2']


@pytest.fixture(scope='module')
def data(tmp_path_factory):
    from PIL import Image
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    d = tmp_path_factory.mktemp('in')
    imgs = synthetic_sequence(T, H, W_, seed=6)
    paths = []
    for i in range(T):
        p = str(d / ('frame-%06d.color.png' % i))
        Image.fromarray(imgs[i]).save(p)
        paths.append(p)
    (d / 'image_list.txt').write_text('\n'.join(paths) + '\n')
    np.savetxt(str(d / 'transform.txt'), synthetic_transform())
    return str(d), imgs


def _records(folder, kind, frames):
    return np.stack([np.load(os.path.join(folder, '%s_%d.npy' % (kind, i))) for i in frames])


def _run(main, inp, model, out, extra=()):
    os.makedirs(out)
    rc = main(['--input_folder', inp, '--output_folder', out, '--model_folder', model] + list(extra) + SMALL)
    assert rc == 0
    return out


def test_kfnet_eval_restores_the_newest_checkpoint(tmp_path, data, capsys):
    """model.ckpt-100, model.ckpt-2500 (full KFNet, Adam slots, snappy index) and kfnet_weights-900.npz: the step-2500
    checkpoint wins, and its records are the bits of a run from kfnet_weights.npz holding the same weights."""
    from kfnet_amd.KFNet import eval as KE
    from kfnet_amd.weights import save_npz, synthetic_weights
    inp, imgs = data
    W_new = synthetic_weights(4321)
    model = tmp_path / 'model'
    model.mkdir()
    TW.training_checkpoint(str(model / 'model.ckpt-100'), synthetic_weights(77), step=100, adam=False)
    TW.training_checkpoint(str(model / 'model.ckpt-2500'), W_new, step=2500, compression='snappy', block_size=512)
    save_npz(str(model / 'kfnet_weights-900.npz'), synthetic_weights(900))
    npz = tmp_path / 'npz'
    npz.mkdir()
    save_npz(str(npz / 'kfnet_weights.npz'), W_new)
    capsys.readouterr()
    a = _run(KE.main, inp, str(model), str(tmp_path / 'a'), ['--scene', 'heads'])
    log = capsys.readouterr().out
    assert 'model.ckpt-2500 (step 2500): %d variables restored, %d ignored' % (len(W_new), 2 * len(W_new) + 3) in log
    b = _run(KE.main, inp, str(npz), str(tmp_path / 'b'), ['--scene', 'heads'])
    got, want = _records(a, 'coord', range(T)), _records(b, 'coord', range(T))
    assert got.shape == (T, H // 8, W_ // 8, 4)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    T4 = KE.get_transform(os.path.join(inp, 'transform.txt'))
    ref = O.eval_sequence(imgs, W_new, T4, reset_period=500, dtype=np.float64)
    dc = float(np.abs(got[..., :3] - ref[..., :3]).max())
    dr = float((np.abs(got[..., 3] - ref[..., 3]) / np.abs(ref[..., 3])).max())
    assert dc <= 1e-4 and dr <= 1e-4, (dc, dr)


@pytest.mark.parametrize('program,scope,kind', [('SCoordNet', 'ScoreNet', 'coord'), ('OFlowNet', 'Temporal', 'flow')])
def test_single_network_programs_restore_their_scope(tmp_path, data, program, scope, kind):
    """SCoordNet eval from a ScoreNet-only checkpoint, OFlowNet eval from a Temporal-only one: the same bits as the
    program fed the equivalent scope-only .npz."""
    import importlib
    from kfnet_amd.weights import save_npz, synthetic_weights
    main = importlib.import_module('kfnet_amd.%s.eval' % program).main
    inp, _ = data
    Ws = {k: v for k, v in synthetic_weights(55).items() if k.startswith(scope + '/')}
    model, npz = tmp_path / 'model', tmp_path / 'npz'
    model.mkdir()
    npz.mkdir()
    TW.training_checkpoint(str(model / 'model.ckpt-30'), Ws, step=30, num_shards=2)
    save_npz(str(npz / 'kfnet_weights-30.npz'), Ws)
    extra = ['--scene', 'heads'] if kind == 'coord' else []
    a = _run(main, inp, str(model), str(tmp_path / 'a'), extra)
    b = _run(main, inp, str(npz), str(tmp_path / 'b'), extra)
    frames = range(T) if kind == 'coord' else range(1, T)
    got, want = _records(a, kind, frames), _records(b, kind, frames)
    assert np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_a_corrupt_tensor_stops_the_program(tmp_path, data):
    """One flipped byte in a tensor the program loads: non-zero exit, the variable named, no output written."""
    from kfnet_amd.weights import synthetic_weights
    inp, _ = data
    Ws = {k: v for k, v in synthetic_weights(56).items() if k.startswith('Temporal/')}
    model = tmp_path / 'model'
    model.mkdir()
    prefix = str(model / 'model.ckpt-8')
    ents = TW.training_checkpoint(prefix, Ws, step=8)
    e = ents['Temporal/conv3b/kernel']
    with open(prefix + '.data-00000-of-00001', 'r+b') as f:
        f.seek(e.offset + 1000)
        b = f.read(1)
        f.seek(e.offset + 1000)
        f.write(bytes([b[0] ^ 0x10]))
    out = tmp_path / 'out'
    out.mkdir()
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        env.pop(k, None)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    r = subprocess.run([sys.executable, '-m', 'kfnet_amd.OFlowNet.eval', '--input_folder', inp, '--output_folder',
                        str(out), '--model_folder', str(model)] + SMALL, cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode != 0
    assert 'Temporal/conv3b/kernel' in r.stderr and 'CRC-32C mismatch' in r.stderr, r.stderr[-2000:]
    assert os.listdir(str(out)) == []
