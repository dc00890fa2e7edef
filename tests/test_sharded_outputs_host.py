"""CPU tests of what the frame-sharded eval runs print besides their records (no GPU): dist.gather_frames over a gloo world
with an empty rank, the summary lines built from gathered results, the label rows a chunk reads from its neighbours, and
the input checks every rank makes before any engine or collective."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from kfnet_amd.dist import chunk_bounds, gather_frames
from kfnet_amd.KFNet import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _frame_metrics(i):
    """A metrics dict of frame i with values that do not sum exactly in fp64 (so that the summary depends on order)."""
    rng = np.random.default_rng(i)
    return dict(i=i, pair=(i - 1, i), l_m=0.1, l_t=0.2, l_kf=0.3, a_m=0.4, a_t=0.5, a_kf=0.6,
                d_m=float(rng.random() * 37.1), d_t=float(rng.random() * 1e-3), d_kf=float(rng.random() * 1e5), nis=0.7)


def _gather_worker(rank, world, port, T, out_dir):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        lo, hi = chunk_bounds(T, world, rank)
        # a rank reports its frames in any order; the result is ordered by frame index
        items = [(i, (_frame_metrics(i), i % 3)) for i in reversed(range(lo, hi))]
        got = gather_frames(dist, items)
        # a second use: every rank joins it again, the empty one included
        again = gather_frames(dist, [(i, i * i) for i in range(lo, hi)])
        if rank != 0:
            assert got is None and again is None
            return
        with open(os.path.join(out_dir, 'result.txt'), 'w') as f:
            assert [m['i'] for m, _ in got] == list(range(T))
            assert [st for _, st in got] == [i % 3 for i in range(T)]
            assert again == [i * i for i in range(T)]
            one = [_frame_metrics(i) for i in range(T)]
            assert [m for m, _ in got] == one
            assert M.summary_lines([m for m, _ in got]) == M.summary_lines(one)
            assert M.summary_lines([m for m, _ in got], ('d_m',)) == M.summary_lines(one, ('d_m',))
            f.write('ok\n')
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('T,world', [(7, 3), (2, 3)])
def test_gather_frames_orders_results_of_every_rank_on_rank_0(tmp_path, T, world):
    """(7, 3): chunks of 3, 2, 2 frames; (2, 3): the last rank owns no frame and still joins both gathers."""
    if T < world:
        assert chunk_bounds(T, world, world - 1)[0] == chunk_bounds(T, world, world - 1)[1]
    mp.spawn(_gather_worker, args=(world, _free_port(), T, str(tmp_path)), nprocs=world, join=True)
    assert open(str(tmp_path / 'result.txt')).read() == 'ok\n'


def _duplicate_worker(rank, world, port, out_dir):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        try:
            gather_frames(dist, [(5, rank)])
            outcome = 'returned'
        except ValueError as e:
            outcome = 'ValueError: %s' % e
        with open(os.path.join(out_dir, 'rank%d.txt' % rank), 'w') as f:
            f.write(outcome)
    finally:
        dist.destroy_process_group()


def test_gather_frames_refuses_a_frame_reported_twice(tmp_path):
    mp.spawn(_duplicate_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert 'frame 5 was reported by more than one rank' in open(str(tmp_path / 'rank0.txt')).read()
    assert open(str(tmp_path / 'rank1.txt')).read() == 'returned'


def test_summary_lines_are_what_print_writes(capsys):
    ms = [_frame_metrics(i) for i in range(11)]
    for name, fn in (('Median dist error: ', np.median), ('Mean dist error: ', np.mean), ('stddev error: ', np.std)):
        print(name, fn([m['d_m'] for m in ms]), fn([m['d_t'] for m in ms]), fn([m['d_kf'] for m in ms]))
    assert capsys.readouterr().out.splitlines() == M.summary_lines(ms)
    for name, fn in (('Median dist error: ', np.median), ('Mean dist error: ', np.mean), ('stddev error: ', np.std)):
        print(name, fn([m['d_m'] for m in ms]))
    assert capsys.readouterr().out.splitlines() == M.summary_lines(ms, ('d_m',))


@pytest.mark.parametrize('T,world,seq', [(1002, 2, 500), (1000, 2, 500), (520, 3, 500), (3, 4, 500), (100, 4, 1000)])
def test_label_rows_of_a_chunk_equal_those_of_the_whole_sequence(T, world, seq):
    """Every frame's label pair resolves to the same two label grids whether the frame is evaluated in one chunk of the
    whole sequence or in its rank's chunk -- whose pairs may reach a label a neighbour owns (frame lo-1, and s+1 at a
    sequence start s that ends a chunk)."""
    grids = np.arange(T, dtype=np.float32)[:, None, None, None] * np.ones((1, 2, 3, 4), np.float32)
    pairs = M.pair_schedule(0, T, T, seq)
    rows, local = M.label_rows(0, pairs, T, lambda i: grids[i])
    want = rows[local]
    reached = set()
    for r in range(world):
        lo, hi = chunk_bounds(T, world, r)
        if hi == lo:
            continue
        p = M.pair_schedule(lo, hi - lo, T, seq)
        assert np.array_equal(p, pairs[lo:hi])
        rows, local = M.label_rows(lo, p, T, lambda i: grids[i])
        assert rows.shape[0] <= hi - lo + 2
        assert np.array_equal(rows[local], want[lo:hi])
        reached |= {int(i) for i in p.ravel() if not lo <= i < hi}
    if (T, world) == (1002, 2):
        assert reached == {500, 501}       # (501, 500) on rank 0, (500, 501) on rank 1


def test_handoff_period_follows_the_engine():
    """A KFNetEngine with label metrics sets handoff_period = 0: a chunk that starts on a reset frame receives the state
    too, because that frame's l_t / l_kf / nis are computed from it.  Engines without the attribute keep their reset
    period."""
    from types import SimpleNamespace
    from kfnet_amd.dist import handoff_period, handoff_plan
    assert handoff_period(SimpleNamespace(reset_period=500)) == 500
    assert handoff_period(SimpleNamespace(reset_period=1)) == 1
    metrics_eng = SimpleNamespace(reset_period=500, handoff_period=0)
    assert handoff_period(metrics_eng) == 0
    assert handoff_plan(500, 500, 1, 2, 500) == (False, False)
    assert handoff_plan(0, 500, 0, 2, handoff_period(metrics_eng)) == (False, True)
    assert handoff_plan(500, 500, 1, 2, handoff_period(metrics_eng)) == (True, False)


def _run(args, env=None):
    e = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT'):
        e.pop(k, None)
    e.update(env or {})
    e['PYTHONPATH'] = ROOT + os.pathsep + e.get('PYTHONPATH', '')
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, timeout=300)


def _short_label_list(folder, T=4):
    for i in range(T):
        open(os.path.join(folder, 'frame_%d.png' % i), 'wb').close()
        open(os.path.join(folder, 'label_%d.bin' % i), 'wb').close()
    with open(os.path.join(folder, 'image_list.txt'), 'w') as f:
        f.write(''.join(os.path.join(folder, 'frame_%d.png\n' % i) for i in range(T)))
    with open(os.path.join(folder, 'label_list.txt'), 'w') as f:
        f.write(''.join(os.path.join(folder, 'label_%d.bin\n' % i) for i in range(T - 1)))


@pytest.mark.parametrize('module', ['kfnet_amd.KFNet.eval', 'kfnet_amd.SCoordNet.eval'])
@pytest.mark.parametrize('rank', ['0', '1'])
def test_every_rank_refuses_a_short_label_list_before_any_collective(tmp_path, module, rank):
    """A torch.distributed.run-style environment whose rendezvous nobody serves: a rank that went on to an engine or a
    collective would fail differently (no GPU here) or wait for its peer until the time limit.  --pose is accepted in the
    sharded run; the bad folder is what fails, with status 1, on every rank."""
    inp, out = tmp_path / 'in', tmp_path / 'out'
    inp.mkdir()
    out.mkdir()
    _short_label_list(str(inp))
    r = _run(['-m', module, '--scene', 'chess', '--input_folder', str(inp), '--output_folder', str(out), '--pose',
              '--random_weights', '--height', '64', '--width', '96'],
             env={'WORLD_SIZE': '2', 'RANK': rank, 'LOCAL_RANK': rank, 'MASTER_ADDR': '127.0.0.1',
                  'MASTER_PORT': str(_free_port())})
    assert r.returncode == 1, r.stdout[-3000:]
    assert 'lists 3 labels for 4 images' in r.stdout
    assert 'not supported in the sharded run' not in r.stdout
    assert os.listdir(str(out)) == []


@pytest.mark.parametrize('module', ['kfnet_amd.KFNet.eval', 'kfnet_amd.SCoordNet.eval'])
def test_labels_in_a_sharded_run_need_torch_distributed_run(tmp_path, module):
    """WORLD_SIZE=2 but no rendezvous (MASTER_PORT unset): rank 0 could not gather the per-frame metrics, so the run is
    refused with status 2 before it loads weights or writes a file -- as --pose is (tests/test_pnp_host.py,
    tests/test_modes_host.py)."""
    inp, out = tmp_path / 'in', tmp_path / 'out'
    inp.mkdir()
    out.mkdir()
    _short_label_list(str(inp))
    with open(str(inp / 'label_list.txt'), 'a') as f:
        f.write(os.path.join(str(inp), 'label_3.bin\n'))
    r = _run(['-m', module, '--scene', 'chess', '--input_folder', str(inp), '--output_folder', str(out),
              '--random_weights', '--height', '64', '--width', '96'], env={'WORLD_SIZE': '2', 'RANK': '0'})
    assert r.returncode == 2, r.stdout[-3000:]
    assert 'label_list.txt is not supported in the sharded run without torch.distributed.run' in r.stdout
    assert os.listdir(str(out)) == []
