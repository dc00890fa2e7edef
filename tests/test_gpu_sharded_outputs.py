"""-m gpu: the frame-sharded eval runs print and write what a single process does -- label metrics and camera poses
included (kfnet_amd.modes.ChunkOutputs / report_sharded / run_shard / run_shard_cyclic, dist.gather_frames).

Every case runs the command line twice, one after the other: first as one process (the reference), then under
torch.distributed.run with its ranks sharing this GPU over gloo.  Both poses and metrics are per frame and deterministic,
so the comparison is exact: rank 0's metric lines, summary and pose count (stdout of rank 0 alone, --local-ranks-filter 0)
equal the single process's as an ordered list of strings, and every pose_<i>.txt and coord_<i>.npy file is byte-identical."""
import os
import re
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ['--random_weights', '--height', '64', '--width', '96']
FRAMES = 1002

KFNET_LINE = re.compile(r'^\d+, frame \d+~\d+, l_m = ')
SCOORD_LINE = re.compile(r'^\d+, frame \d+, d_m = ')
SUMMARY = ('Median dist error: ', 'Mean dist error: ', 'stddev error: ')


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _write_dataset(folder, T):
    """T frames at 64x96 (as tests/test_gpu_modes.py): PNGs, raw float32 [64,96,4] labels, transform.txt."""
    from PIL import Image
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    rng = np.random.default_rng(11)
    imgs = synthetic_sequence(T, 64, 96, seed=2)
    for i in range(T):
        Image.fromarray(imgs[i]).save(os.path.join(folder, 'frame_%d.png' % i))
        lab = np.empty((64, 96, 4), np.float32)
        lab[..., :3] = rng.normal(scale=0.5, size=(64, 96, 3))
        lab[..., 3] = (rng.random((64, 96)) < 0.8).astype(np.float32)
        lab.tofile(os.path.join(folder, 'label_%d.bin' % i))
    np.savetxt(os.path.join(folder, 'transform.txt'), synthetic_transform())


@pytest.fixture(scope='module')
def frames_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp('frames')
    _write_dataset(str(d), FRAMES)
    return str(d)


def _input_folder(tmp_path, frames_dir, T, labels=True):
    """An input folder listing the first T frames of the shared dataset."""
    inp = tmp_path / 'in'
    inp.mkdir()
    shutil.copy(os.path.join(frames_dir, 'transform.txt'), str(inp / 'transform.txt'))
    lists = [('image_list.txt', 'frame_%d.png')] + ([('label_list.txt', 'label_%d.bin')] if labels else [])
    for name, pattern in lists:
        with open(str(inp / name), 'w') as f:
            f.write(''.join(os.path.join(frames_dir, pattern % i) + '\n' for i in range(T)))
    return str(inp)


def _env():
    e = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT'):
        e.pop(k, None)
    e['PYTHONPATH'] = ROOT + os.pathsep + e.get('PYTHONPATH', '')
    e['KFN_DIST_BACKEND'] = 'gloo'
    return e


def _single(module, args, timeout=600):
    r = subprocess.run([sys.executable, '-m', module] + args, cwd=ROOT, env=_env(), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def _sharded_run(module, args, world, timeout=900, rank0_only=True):
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world),
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port())]
    cmd += (['--local-ranks-filter', '0'] if rank0_only else []) + ['-m', module] + args
    return subprocess.run(cmd, cwd=ROOT, env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                          timeout=timeout)


def _sharded(module, args, world, timeout=900):
    r = _sharded_run(module, args, world, timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def _report(stdout, line_re):
    """The lines a run prints behind its records, in order: per-frame metric lines, the summary, the pose count."""
    return [l for l in stdout.splitlines() if line_re.match(l) or l.startswith(SUMMARY) or l.startswith('poses: ')]


def _same_files(one, two, T):
    for i in range(T):
        for name in ('coord_%d.npy' % i, 'pose_%d.txt' % i):
            with open(os.path.join(one, name), 'rb') as a, open(os.path.join(two, name), 'rb') as b:
                assert a.read() == b.read(), name
    assert sorted(os.listdir(one)) == sorted(os.listdir(two))


def _compare(tmp_path, module, inp, T, world, extra, line_re=KFNET_LINE):
    one, two = tmp_path / 'one', tmp_path / 'two'
    one.mkdir()
    two.mkdir()
    args = ['--input_folder', inp, '--pose'] + extra + SMALL
    want = _report(_single(module, args + ['--output_folder', str(one)]), line_re)
    got_out = _sharded(module, args + ['--output_folder', str(two)], world)
    got = _report(got_out, line_re)
    n_lines = len([l for l in want if line_re.match(l)])
    assert n_lines == T and len(want) == T + 4, want[-6:]
    assert got == want
    _same_files(str(one), str(two), T)
    return got_out, want


@pytest.mark.parametrize('T', [1000, 1002])
def test_kfnet_contiguous_two_ranks_stairs(tmp_path, frames_dir, T):
    """1000: the reset and the metrics sequence start at frame 500 fall on the rank boundary.  The records need no hand-off
    there, but frame 500's l_t / l_kf / nis are computed from the incoming state, so rank 1 receives it all the same
    (dist.handoff_period).  1002: frame 500 is rank 0's last; its pair (501, 500) reads a label of rank 1, and rank 1's
    first pair (500, 501) one of rank 0."""
    inp = _input_folder(tmp_path, frames_dir, T)
    out, want = _compare(tmp_path, 'kfnet_amd.KFNet.eval', inp, T, 2, ['--scene', 'stairs'])
    half = T // 2 + T % 2
    assert 'rank 0/2: frames 0~%d done' % (half - 1) in out
    assert any(l.startswith('500, frame 501~500, ') for l in want)
    assert any(l.startswith('501, frame 500~501, ') for l in want)
    assert want[-1].startswith('poses: ') and want[-1].endswith(' of %d frames solved' % T)


def test_kfnet_contiguous_three_ranks_nis(tmp_path, frames_dir):
    """520 frames on 3 ranks (174, 173, 173): the reset at 500 falls inside the last rank's chunk."""
    inp = _input_folder(tmp_path, frames_dir, 520)
    _compare(tmp_path, 'kfnet_amd.KFNet.eval', inp, 520, 3, ['--scene', 'stairs', '--NIS'])


def test_kfnet_cyclic_four_ranks(tmp_path, frames_dir):
    """100 frames in blocks of 16 dealt over 4 ranks: a block's first pair reads the label of the block before, which
    another rank owns."""
    inp = _input_folder(tmp_path, frames_dir, 100)
    out, _ = _compare(tmp_path, 'kfnet_amd.KFNet.eval', inp, 100, 4,
                      ['--scene', 'heads', '--sharding', 'cyclic', '--block', '16'])
    assert 'rank 0/4: 2 blocks of 16 frames done (block-cyclic)' in out


def test_scoordnet_two_ranks(tmp_path, frames_dir):
    inp = _input_folder(tmp_path, frames_dir, 41)
    _compare(tmp_path, 'kfnet_amd.SCoordNet.eval', inp, 41, 2, ['--scene', 'chess'], line_re=SCOORD_LINE)


def test_kfnet_empty_chunk(tmp_path, frames_dir):
    """3 frames on 4 ranks: rank 3 owns none, builds its engine, joins the gather and exits 0."""
    inp = _input_folder(tmp_path, frames_dir, 3)
    out, _ = _compare(tmp_path, 'kfnet_amd.KFNet.eval', inp, 3, 4, ['--scene', 'chess'])
    assert 'rank 0/4: frames 0~0 done' in out


def test_kfnet_poses_without_labels(tmp_path, frames_dir):
    """--pose alone (no label_list.txt): pose files and the pose count, nothing else."""
    inp = _input_folder(tmp_path, frames_dir, 30, labels=False)
    one, two = tmp_path / 'one', tmp_path / 'two'
    one.mkdir()
    two.mkdir()
    args = ['--input_folder', inp, '--pose', '--scene', 'fire'] + SMALL
    want = _report(_single('kfnet_amd.KFNet.eval', args + ['--output_folder', str(one)]), KFNET_LINE)
    got = _report(_sharded('kfnet_amd.KFNet.eval', args + ['--output_folder', str(two)], 2), KFNET_LINE)
    assert len(want) == 1 and want[0].startswith('poses: ') and got == want
    _same_files(str(one), str(two), 30)


def test_short_label_list_fails_every_rank(tmp_path, frames_dir):
    inp = _input_folder(tmp_path, frames_dir, 6)
    lines = open(os.path.join(inp, 'label_list.txt')).read().splitlines()
    with open(os.path.join(inp, 'label_list.txt'), 'w') as f:
        f.write('\n'.join(lines[:-1]) + '\n')
    out = tmp_path / 'out'
    out.mkdir()
    r = _sharded_run('kfnet_amd.KFNet.eval', ['--input_folder', inp, '--output_folder', str(out), '--scene', 'chess',
                                              '--pose'] + SMALL, 2, timeout=300, rank0_only=False)
    assert r.returncode != 0
    assert 'lists 5 labels for 6 images' in r.stderr
    assert os.listdir(str(out)) == []


def test_missing_label_file_ends_the_run(tmp_path, frames_dir):
    """A label of rank 1's range is gone: rank 1 raises while rank 0 waits in the gather; torch.distributed.run stops the
    group and the run ends non-zero instead of hanging."""
    T = 40
    inp = _input_folder(tmp_path, frames_dir, T)
    lab = tmp_path / 'gone.bin'
    with open(os.path.join(inp, 'label_list.txt')) as f:
        lines = f.read().splitlines()
    lines[30] = str(lab)       # frame 30 of rank 1's [20, 40): a file that does not exist
    with open(os.path.join(inp, 'label_list.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    out = tmp_path / 'out'
    out.mkdir()
    r = _sharded_run('kfnet_amd.KFNet.eval', ['--input_folder', inp, '--output_folder', str(out), '--scene', 'chess']
                     + SMALL, 2, timeout=300, rank0_only=False)
    assert r.returncode != 0
    assert 'gone.bin' in r.stderr
