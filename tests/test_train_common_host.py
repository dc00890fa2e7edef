"""CPU tests of what the three trainers and the three training programs share (kfnet_amd/train_common.py, train_cli.py,
staging.stage_labels; DESIGN.md 6b "Shared host pieces"): the parameter store on CPU tensors, the parsers against the defaults
recorded before the flags were declared once, the loop with a fake trainer, the label staging and the snapshot reader."""
import os

import numpy as np
import pytest
import torch

from kfnet_amd import staging, train_cli
from kfnet_amd.train_common import LazyStats, ParamStore, read_snapshot, snapshot_paths

SPECS = [('S/a/kernel', (3, 3, 2, 5)), ('S/a/bias', (5,)), ('S/b/kernel', (1, 1, 5, 3)), ('S/b/bias', (3,))]


def _arrays(seed, prefix=''):
    rng = np.random.default_rng(seed)
    return {prefix + n: rng.normal(size=shape).astype(np.float32) for n, shape in SPECS}


# -- the store -------------------------------------------------------------------------------------------------------------------
def test_slots_follow_the_specs_at_multiples_of_four_floats():
    st = ParamStore(SPECS)
    assert list(st.slots) == [n for n, _ in SPECS]
    assert [st.slots[n] for n, _ in SPECS] == [(0, 90, (3, 3, 2, 5)), (92, 5, (5,)), (100, 15, (1, 1, 5, 3)), (116, 3, (3,))]
    assert st.num_floats == 120 and all(off % 4 == 0 for off, _, _ in st.slots.values())
    for buf in (st.params, st.grads, st.m, st.v):
        assert buf.shape == (120,) and buf.dtype == torch.float32 and buf.device.type == 'cpu' and not buf.any()
    assert (st.global_step, st.adam_t) == (0, 0)


@pytest.mark.parametrize('prefix', ['', 'adam_m/'])
def test_fill_then_read_back_is_the_identity(prefix):
    st = ParamStore(SPECS)
    A = _arrays(1, prefix)
    st._fill(st.grads, A, prefix)
    got = st._named(st.grads, prefix)
    assert sorted(got) == sorted(A)
    for k in A:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], A[k])
    assert not st.grads[90:92].any() and not st.grads[97:100].any()        # the padding between slots stays zero
    st._packs_stale = False
    st.set_weights(_arrays(2))
    assert st._packs_stale and all(np.array_equal(v, _arrays(2)[k]) for k, v in st.weights().items())
    assert all(np.array_equal(v, A[prefix + k]) for k, v in st.gradients().items())


def test_fill_names_the_missing_key_and_the_wrong_shape():
    st = ParamStore(SPECS)
    A = _arrays(3, 'adam_v/')
    del A['adam_v/S/b/kernel']
    with pytest.raises(KeyError) as e:
        st._fill(st.v, A, 'adam_v/')
    assert e.value.args[0] == 'weights lack adam_v/S/b/kernel'
    A = _arrays(3)
    A['S/a/bias'] = np.zeros((1, 5), np.float32)
    with pytest.raises(ValueError) as e:
        st.set_weights(A)
    assert str(e.value) == 'S/a/bias has shape (1, 5), expected (5,)'


def test_state_round_trip_and_the_slots_alone():
    a, b = ParamStore(SPECS), ParamStore(SPECS)
    a._fill(a.m, _arrays(4))
    a._fill(a.v, _arrays(5))
    a.global_step, a.adam_t = 12, 11
    st = a.state()
    assert sorted(st) == sorted(['global_step', 'adam_t'] + [p + n for p in ('adam_m/', 'adam_v/') for n, _ in SPECS])
    assert st['global_step'].dtype == np.int64 and st['adam_t'].dtype == np.int64 and st['adam_m/S/a/bias'].dtype == np.float32
    b.load_state(st)
    assert torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and (b.global_step, b.adam_t) == (12, 11)
    c = ParamStore(SPECS)
    c.load_slots(st)                       # the slots of this state, the counters stay
    assert torch.equal(a.m, c.m) and torch.equal(a.v, c.v) and (c.global_step, c.adam_t) == (0, 0)
    c.zero_slots()                         # what a state lacking the scope's slots leads to
    assert not c.m.any() and not c.v.any()
    with pytest.raises(KeyError):
        ParamStore([('T/x/kernel', (2,))]).load_slots(st)


def test_save_writes_the_two_files_of_a_snapshot(tmp_path):
    a = ParamStore(SPECS)
    a.set_weights(_arrays(6))
    a.global_step = a.adam_t = 3
    wp, sp = a.save(str(tmp_path / 'new'))
    assert (wp, sp) == snapshot_paths(str(tmp_path / 'new'), 3)
    with np.load(wp) as z:
        assert sorted(z.files) == sorted(n for n, _ in SPECS) and np.array_equal(z['S/b/bias'], _arrays(6)['S/b/bias'])
    with np.load(sp) as z:
        assert int(z['global_step']) == 3 and len(z.files) == 2 + 2 * len(SPECS)
    assert os.path.basename(a.save(str(tmp_path), 8)[0]) == 'kfnet_weights-8.npz'


def test_lazy_stats_read_back_once_and_only_when_asked():
    class Dev(object):
        reads = 0

        def cpu(self):
            Dev.reads += 1
            return torch.tensor([2.0, 5.0])

    class Stats(LazyStats):
        KEYS = ('loss', 'lr')

        def _decode(self, s):
            return dict(loss=float(s[0]), lr=self._lr)
    s = Stats(Dev(), 0.5)
    assert s.keys() == ['loss', 'lr'] and Dev.reads == 0
    assert dict(s) == dict(loss=2.0, lr=0.5) and s['loss'] == 2.0 and Dev.reads == 1


# -- the parsers: vars(build_parser().parse_args([])) as the programs gave it before the shared flags were declared once ---------
CAMERA = dict(focal_x=525.0, focal_y=525.0, u=320.0, v=240.0, depth_focal_x=None, depth_focal_y=None, depth_u=None, depth_v=None)
STAGE1 = dict(CAMERA, augment=False, augment_seed=None, base_lr=0.0001, batch=4, depth=False, display=10, fp16=False, gamma=0.5,
              gpu=0, height=480, input_folder='', loss_clip=None, loss_scale=None, max_steps=None, model_folder='', reproj=None,
              reset_step=-1, scene='', seed=0, shuffle=False, smooth_weight=50.0, snapshot=5000, stepvalue=None, synthetic=0,
              weight_decay=0.0001, width=640)
STAGE2 = dict(CAMERA, augment=False, base_lr=0.0001, depth=False, display=10, fp16=False, gamma=0.5, gpu=0, height=480,
              input_folder='', loss_clip=None, max_steps=None, model_folder='', pairs=4, reset_step=-1, seed=0,
              sequence_length=1000, shuffle=False, snapshot=5000, stepvalue=100000, synthetic=0, weight_decay=0.0001, width=640)
STAGE3 = dict(STAGE1, reproj=False, reproj_weights=None, fix_flownet=False, joint=False, groups=1, oflownet='', scoordnet='',
              sequence_length=None)


def test_parsers_hold_the_recorded_flags_and_defaults(capsys):
    from kfnet_amd.KFNet.train import build_parser as stage3
    from kfnet_amd.OFlowNet.train import build_parser as stage2
    from kfnet_amd.SCoordNet.train import build_parser as stage1
    assert vars(stage1().parse_args([])) == STAGE1
    assert vars(stage2().parse_args([])) == STAGE2
    assert vars(stage3().parse_args([])) == STAGE3
    for flags in (['--scene', 'fire'], ['--reproj'], ['--batch', '2'], ['--smooth_weight', '1'], ['--augment_seed', '1'],
                  ['--loss_scale', '2']):
        with pytest.raises(SystemExit):
            stage2().parse_args(flags)
    assert stage1().parse_args(['--reproj', '5']).reproj == 5.0 and stage1().parse_args(['--reproj']).reproj == 50.0
    assert stage3().parse_args(['--reproj']).reproj is True
    with pytest.raises(SystemExit):
        stage3().parse_args(['--reproj', '5'])                  # stage 3's takes no number
    capsys.readouterr()
    # the help texts that differ per program
    assert 'refused: not built for pairs' in stage2().format_help() and 'refused' not in stage1().format_help()
    assert 'brightness, contrast, rotation' in stage3().format_help()


def test_shared_checks_give_each_programs_own_line():
    import argparse
    a = argparse.Namespace(model_folder='', display=1, snapshot=1, batch=0, pairs=1, stepvalue=0, groups=1)
    assert train_cli.check_flags(a, ('display', 'snapshot', 'batch')) == '--model_folder is required: the snapshots go there'
    a.model_folder = 'm'
    assert train_cli.check_flags(a, ('display', 'snapshot', 'batch')) == '--display, --snapshot and --batch must be >= 1'
    assert (train_cli.check_flags(a, ('display', 'snapshot', 'pairs', 'stepvalue')) ==
            '--display, --snapshot, --pairs and --stepvalue must be >= 1')
    assert train_cli.check_flags(a, ('display', 'snapshot', 'groups')) is None
    a.snapshot = 0
    assert train_cli.check_flags(a, ('display', 'snapshot', 'groups')) == '--display, --snapshot and --groups must be >= 1'


# -- the loop --------------------------------------------------------------------------------------------------------------------
class _Stats(object):
    converted = []

    def __init__(self, step):
        self.step = step

    def keys(self):
        _Stats.converted.append(self.step)
        return ['loss']

    def __getitem__(self, k):
        return float(self.step)


class _Trainer(object):
    def __init__(self, step):
        self.global_step, self.calls = step, []

    def set_poses(self, poses):
        self.calls.append(('poses', poses))

    def step(self, frames, labels, **kw):
        self.calls.append(('step', frames, labels, kw))
        self.global_step += 1
        return _Stats(self.global_step)

    def save(self, folder, step):
        self.calls.append(('save', step))
        return '%s/w-%d' % (folder, step), '%s/s-%d' % (folder, step)


def _run(tr, monkeypatch, capsys, poses=None):
    synced = []
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda: synced.append(True))
    _Stats.converted = []
    asked = []

    def batch(step):
        asked.append(step)
        return [step, step + 1], 'f%d' % step, 'l%d' % step, poses, dict(augment=step)

    def line(stats, s, indices, duration):
        assert type(stats) is dict and duration >= 0.0
        return 'line %d %s %s' % (s, indices, stats['loss'])
    assert train_cli.loop(tr, 7, 2, 3, 'M', batch, line) == 0
    return asked, synced, capsys.readouterr().out.splitlines()


def test_loop_displays_snapshots_and_reads_stats_only_on_display_steps(monkeypatch, capsys):
    tr = _Trainer(0)
    asked, synced, out = _run(tr, monkeypatch, capsys)
    assert asked == list(range(7)) and synced == [True] and tr.global_step == 7
    assert _Stats.converted == [2, 4, 6, 7]
    assert out == ['line 2 [1, 2] 2.0', 'snapshot: M/w-3, M/s-3', 'line 4 [3, 4] 4.0', 'line 6 [5, 6] 6.0',
                   'snapshot: M/w-6, M/s-6', 'line 7 [6, 7] 7.0', 'snapshot: M/w-7, M/s-7']
    assert [c for c in tr.calls if c[0] == 'save'] == [('save', 3), ('save', 6), ('save', 7)]
    assert tr.calls[0] == ('step', 'f0', 'l0', dict(augment=0)) and not any(c[0] == 'poses' for c in tr.calls)
    # poses, where the batch has them, go to the trainer in front of every step
    tr = _Trainer(5)
    asked, _, out = _run(tr, monkeypatch, capsys, poses='P')
    assert asked == [5, 6] and [c[0] for c in tr.calls] == ['poses', 'step', 'save', 'poses', 'step', 'save']
    assert out == ['line 6 [5, 6] 6.0', 'snapshot: M/w-6, M/s-6', 'line 7 [6, 7] 7.0', 'snapshot: M/w-7, M/s-7']


def test_loop_from_the_last_step_does_nothing(monkeypatch, capsys):
    tr = _Trainer(7)
    asked, synced, out = _run(tr, monkeypatch, capsys)
    assert asked == [] and tr.calls == [] and out == [] and _Stats.converted == [] and synced == [True]


# -- the labels --------------------------------------------------------------------------------------------------------------------
def test_stage_labels_picks_the_stride_and_reuses_the_buffer():
    B, size, grid = 2, (16, 24), (2, 3)
    rng = np.random.default_rng(7)
    full, small = rng.normal(size=(B, 16, 24, 4)).astype(np.float32), rng.normal(size=(B, 2, 3, 4)).astype(np.float64)
    buf, stride = staging.stage_labels(None, full, B, size, grid, 'cpu')
    assert stride == 8 and buf.dtype == torch.float32 and np.array_equal(buf.numpy(), full)
    again, stride = staging.stage_labels(buf, torch.from_numpy(2 * full), B, size, grid, 'cpu')
    assert again is buf and stride == 8 and np.array_equal(buf.numpy(), 2 * full)
    other, stride = staging.stage_labels(buf, small, B, size, grid, 'cpu')              # numpy of another dtype is converted
    assert other is not buf and stride == 1 and other.dtype == torch.float32 and np.array_equal(other.numpy(), small.astype(np.float32))
    assert staging.stage_labels(other, torch.from_numpy(small), B, size, grid, 'cpu')[0] is other
    with pytest.raises(ValueError) as e:
        staging.stage_labels(other, small[:1], B, size, grid, 'cpu')
    assert str(e.value) == 'labels must be float32 [2,16,24,4] or grid-sized [2,2,3,4], got (1, 2, 3, 4)'


# -- the snapshot reader -------------------------------------------------------------------------------------------------------------
def test_snapshot_reader_and_its_stage_3_face(tmp_path, capsys):
    from kfnet_amd.train_kfnet import restore
    from kfnet_amd.weights import initial_weights, save_npz
    M = str(tmp_path / 'model')
    os.makedirs(M)
    wp, sp = snapshot_paths(M, 7)
    W = initial_weights(1, scopes=('ScoreNet', 'Temporal'))
    save_npz(wp, W)
    np.savez(snapshot_paths(M, 9)[1], global_step=np.int64(9))                    # a state file with a HIGHER step is ignored
    got, state, step = restore(M, verbose=False)
    assert step == 7 and state is None and sorted(got) == sorted(W) and capsys.readouterr().out == ''
    got, state, step = read_snapshot(M, ('ScoreNet', 'Temporal'))
    out = capsys.readouterr().out.splitlines()
    assert step == 7 and state is None and len(out) == 2 and out[0].startswith('Restore from %s (step 7)' % wp)
    assert out[1] == 'no kfnet_train_state-7.npz: the Adam slots start at zero'
    np.savez(sp, global_step=np.int64(7), adam_t=np.int64(6))
    got, state, step = restore(M)
    out = capsys.readouterr().out.splitlines()
    assert int(state['adam_t']) == 6 and out[1] == 'Adam slots restored from %s' % sp and len(out) == 2
    assert read_snapshot(str(tmp_path / 'none'), ('ScoreNet',)) == (None, None, 0) and read_snapshot('', ('ScoreNet',)) == (None, None, 0)
    assert restore(str(tmp_path / 'none'), verbose=False) == ({}, None, 0)
    # --scoordnet: ScoreNet/* of another folder's newest snapshot replaces the model folder's; an empty folder is an error
    A = str(tmp_path / 'stage1')
    os.makedirs(A)
    S1 = initial_weights(2)
    save_npz(snapshot_paths(A, 3)[0], S1)
    got, state, step = restore(M, scoordnet=A, verbose=False)
    assert step == 7 and int(state['global_step']) == 7
    assert np.array_equal(got['ScoreNet/conv1a/kernel'], S1['ScoreNet/conv1a/kernel'])
    assert np.array_equal(got['Temporal/feat1/kernel'], W['Temporal/feat1/kernel'])
    empty = str(tmp_path / 'empty')
    os.makedirs(empty)
    for missing in (empty, str(tmp_path / 'absent')):
        with pytest.raises(ValueError) as e:
            restore(M, scoordnet=missing, verbose=False)
        assert str(e.value) == 'no kfnet_weights*.npz or model.ckpt-*.index in %s' % missing
