"""Host side of joint stage 3 (kfnet_amd/train_kfnet.py with train_flownet, kfnet_amd/KFNet/train.py --joint):
the two formulas kfn_filter_backward_joint adds, restated in float32 (tests/joint_train_ref.py), against fp64 autograd and
central finite differences; the pair table and the unique-index scatter of OFlowNetTrainer's shared-frames layout; the new
export's refusals; the command line's; and train-state files of the older kinds."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import joint_train_ref as JR
import kf_train_ref as KR
from kfnet_amd import _lib
from kfnet_amd.train_common import ParamStore
from kfnet_amd.train_flow import check_pair_index
from kfnet_amd.train_kfnet import pair_table, split_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 5, 7
EPS = 1e-5


def frame_inputs(seed, reach=4.0):
    """KF_{t-1}, a flow with every warped position at least 0.01 from an integer, sigma_trans, and the two incoming gradients."""
    rng = np.random.default_rng(seed)
    prev = rng.normal(size=(H, W, 4)).astype(np.float32)
    prev[..., 3] = 10.0 ** rng.uniform(-2, 0, size=(H, W))
    whole = rng.integers(-int(reach), int(reach), size=(H, W, 2))
    flow = (whole + rng.uniform(0.01, 0.99, size=(H, W, 2))).astype(np.float32)
    st = (10.0 ** rng.uniform(-3, -1, size=(H, W))).astype(np.float32)
    g_x = rng.normal(size=(H, W, 3)).astype(np.float32)
    d_lvar = rng.normal(size=(H, W)).astype(np.float32)
    return prev, flow, st, g_x, d_lvar


def autograd(prev, flow, st, g_x, d_lvar, dtype=torch.float64):
    fl, s = JR.tensor(flow, dtype, True), JR.tensor(st, dtype, True)
    obj = JR.warp_objective(JR.tensor(prev, dtype), fl, s, JR.tensor(g_x, dtype), JR.tensor(d_lvar, dtype))
    gf, gs = torch.autograd.grad(obj, [fl, s])
    return gf.to(torch.float64).numpy(), gs.to(torch.float64).numpy()


# -- the formulas ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_restated_formulas_against_fp64_autograd_and_central_differences(seed):
    prev, flow, st, g_x, d_lvar = frame_inputs(seed)
    frac = flow - np.floor(flow)
    assert frac.min() >= 0.009 and frac.max() <= 0.991
    assert np.abs(flow).max() <= 4.0 and ((np.arange(W)[None, :, None] + flow[..., 0:1]) < 0).any()     # samples leave the grid
    df, ds, s_l = JR.flow_sigma_grads(prev, flow, st, g_x, d_lvar)
    assert np.all(s_l * s_l > 100 * KR.EPS2) or np.all(np.abs(s_l * s_l / KR.EPS2 - 1) > 1e-3)
    f64, s64 = autograd(prev, flow, st, g_x, d_lvar)
    f32, s32 = autograd(prev, flow, st, g_x, d_lvar, torch.float32)
    # the project's rule: no further from fp64 than 8 times torch's own fp32 autograd, floor 1e-6
    for name, got, want, w32 in (('d_flow', df, f64, f32), ('d_sigma_trans', ds, s64, s32)):
        e, e32 = JR.FR.rel_err(got, want), JR.FR.rel_err(w32, want)
        print('%s seed %d: e restatement %.3e, e torch-fp32 %.3e' % (name, seed, e, e32))
        assert e <= max(8.0 * e32, 1e-6), (name, e, e32)
    # central differences of the fp64 objective: the positions are 0.01 from a floor step, the probe moves them by 1e-6
    eps = 1e-6
    args = [JR.tensor(a, torch.float64) for a in (prev, flow, st, g_x, d_lvar)]

    def objective(flow_, st_):
        return JR.warp_objective(args[0], flow_, st_, args[3], args[4]).item()
    rng = np.random.default_rng(seed)
    for _ in range(12):
        r, c, k = int(rng.integers(H)), int(rng.integers(W)), int(rng.integers(2))
        hi, lo = args[1].clone(), args[1].clone()
        hi[r, c, k] += eps
        lo[r, c, k] -= eps
        fd = (objective(hi, args[2]) - objective(lo, args[2])) / (2 * eps)
        assert abs(fd - f64[r, c, k]) <= 1e-6 * max(1.0, np.abs(f64).max()), (r, c, k, fd, f64[r, c, k])
        assert abs(df[r, c, k] - fd) <= 1e-4 * np.abs(f64).max()
        hi, lo = args[2].clone(), args[2].clone()
        hi[r, c] += eps * st[r, c]
        lo[r, c] -= eps * st[r, c]
        fd = (objective(args[1], hi) - objective(args[1], lo)) / (2 * eps * st[r, c])
        assert abs(fd - s64[r, c]) <= 1e-6 * max(1.0, np.abs(s64).max())
        assert abs(ds[r, c] - fd) <= 1e-4 * np.abs(s64).max()


def test_hand_cases_of_the_restatement():
    prev, flow, st, g_x, d_lvar = frame_inputs(5)
    # column 0 sampled 1.5 cells to the left, row H-1 sampled 2.25 below: both corners of that axis clamp to one cell
    flow[:, 0, 0] = -1.5
    flow[H - 1, :, 1] = 2.25
    st[1, :] = 3e-6                        # sigma_trans^2 <= eps^2
    st[2, 0] = np.float32(EPS)             # the gate is strict: float(1e-5)^2 rounds to at most float(1e-10)
    df, ds, s_l = JR.flow_sigma_grads(prev, flow, st, g_x, d_lvar)
    assert np.all(df[:, 0, 0] == 0.0) and np.all(df[H - 1, :, 1] == 0.0)
    ix0, ix1, iy0, iy1 = JR.taps(flow, H, W)[:4]
    assert np.all(ix0[:, 0] == ix1[:, 0]) and np.all(iy0[H - 1] == iy1[H - 1])
    # (a sample that leaves the grid along the other axis has weights w_0 = -w_1 there: the sampler returns 0, and so do these)
    outside = (ix0 == ix1) | (iy0 == iy1)
    assert np.array_equal(df[..., 0] == 0.0, outside) and np.array_equal(df[..., 1] == 0.0, outside)
    assert 4 <= (~outside).sum() < outside.size
    assert np.all(ds[1] == 0.0) and np.all(ds[3:] != 0.0)
    assert np.float32(EPS) * np.float32(EPS) <= np.float32(KR.EPS2) and ds[2, 0] == 0.0
    f64, s64 = autograd(prev, flow, st, g_x, d_lvar)
    tiny = 1e-12 * np.abs(f64).max()                     # autograd sums the four corners' terms: they cancel to rounding
    assert np.all(np.abs(f64[:, 0, 0]) <= tiny) and np.all(np.abs(f64[H - 1, :, 1]) <= tiny) and np.all(s64[1] == 0.0)
    # s_l^2 <= eps^2: whatever the previous sigma holds below the floor, it adds nothing to d_flow
    low = prev.copy()
    low[..., 3] = 1e-7
    other = low.copy()
    other[..., 3] = np.random.default_rng(6).uniform(1e-8, 5e-6, size=(H, W))
    a, _, sa = JR.flow_sigma_grads(low, flow, st, g_x, d_lvar)
    b, _, sb = JR.flow_sigma_grads(other, flow, st, g_x, d_lvar)
    assert np.all(np.abs(sa) < EPS) and np.all(np.abs(sb) < EPS) and not np.array_equal(sa, sb)
    assert np.array_equal(a, b) and np.any(a != 0.0)
    c, _, _ = JR.flow_sigma_grads(prev, flow, st, g_x, d_lvar)
    assert not np.array_equal(a, c)                      # above the floor it does
    # frame 0 of a group: autograd of the whole filter leaves its flow and sigma_trans without gradient
    rng = np.random.default_rng(7)
    pred = rng.normal(size=(1, 3, H, W, 4))
    fl = rng.uniform(-2, 2, size=(1, 3, H, W, 2))
    s = 10.0 ** rng.uniform(-2, -1, size=(1, 3, H, W))
    g = rng.normal(size=(2, 1, 3, H, W, 4))
    _, gf, gs = JR.backward_grads(pred, fl, s, g[0], g[1])
    assert not gf[:, 0].any() and not gs[:, 0].any() and gf[:, 1:].any() and gs[:, 1:].any()


def test_joint_filter_with_constant_flow_is_the_fixed_reference():
    rng = np.random.default_rng(8)
    meas = rng.normal(size=(2, 4, H, W, 4))
    meas[..., 3] = 10.0 ** rng.uniform(-2, 0, size=(2, 4, H, W))
    fl = rng.uniform(-4, 4, size=(2, 4, H, W, 2))
    s = 10.0 ** rng.uniform(-3, -1, size=(2, 4, H, W))
    want = KR.filter_forward(torch.from_numpy(meas), fl, s)
    got = JR.filter_forward(torch.from_numpy(meas), torch.from_numpy(fl), torch.from_numpy(s))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# -- the shared-frames layout ----------------------------------------------------------------------------------------------------
def test_pair_table_for_two_groups_of_four():
    a, b = pair_table(2, 4)
    assert a.tolist() == [0, 1, 2, 4, 5, 6] and b.tolist() == [1, 2, 3, 5, 6, 7]
    ra, rb = JR.pair_table(2, 4)
    assert np.array_equal(a, ra) and np.array_equal(b, rb)
    assert pair_table(1, 2)[0].tolist() == [0] and pair_table(1, 2)[1].tolist() == [1]
    assert len(set(a.tolist())) == len(a) and len(set(b.tolist())) == len(b)      # no frame twice within a list
    assert not set(b.tolist()) & {0, 4}                                          # a group's first frame ends no pair
    check_pair_index((a, b), 6, 8)
    for bad in ((a, b[:-1]), (a, np.array([1, 2, 3, 5, 6, 8])), (np.array([0, 1, 2, 4, 5, 5]), b), (a - 1, b)):
        with pytest.raises(ValueError):
            check_pair_index(bad, 6, 8)


def test_unique_index_scatter_and_add_against_autograd_on_integers():
    """d_feat: zero, d_fb to rows b_idx, d_fa added at rows a_idx -- the transpose of the two gathers.  On integers every sum is
    exact, so the result equals autograd's whatever its order."""
    a, b = pair_table(2, 4)
    rng = np.random.default_rng(9)
    feat = torch.from_numpy(rng.integers(-8, 9, size=(8, 6, 32)).astype(np.float32)).requires_grad_(True)
    d_fa = torch.from_numpy(rng.integers(-8, 9, size=(6, 6, 32)).astype(np.float32))
    d_fb = torch.from_numpy(rng.integers(-8, 9, size=(6, 6, 32)).astype(np.float32))
    ai, bi = torch.from_numpy(a), torch.from_numpy(b)
    f_a, f_b = torch.index_select(feat, 0, ai), torch.index_select(feat, 0, bi)
    want, = torch.autograd.grad((f_a * d_fa).sum() + (f_b * d_fb).sum(), [feat])
    g = torch.full((8, 6, 32), 7.0)
    g.zero_()
    g.index_copy_(0, bi, d_fb)
    g.index_add_(0, ai, d_fa)
    assert torch.equal(g, want)
    assert torch.equal(g[0], d_fa[0]) and torch.equal(g[3], d_fb[2]) and torch.equal(g[1], d_fb[0] + d_fa[1])


def test_trainers_refuse_bad_arguments_without_a_device():
    from kfnet_amd.train_flow import OFlowNetTrainer
    with pytest.raises(ValueError):
        OFlowNetTrainer({}, image_size=(60, 96), pairs=3, frames=4, pair_index=pair_table(1, 4))
    with pytest.raises(ValueError):
        OFlowNetTrainer({}, image_size=(64, 96), pairs=0, frames=4, pair_index=pair_table(1, 4))


# -- the export --------------------------------------------------------------------------------------------------------------------
def test_new_export_is_declared_bound_and_checks_its_arguments_without_a_device():
    header = open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()
    lib = _lib.load()
    assert lib.kfn_abi_version() == 13 and '#define KFN_ABI_VERSION 13' in header
    name = 'kfn_filter_backward_joint'
    assert re.search(r'\bint %s\(' % name, header) and name in _lib.SYMBOLS and hasattr(lib, name)
    decl = re.search(r'int %s\((.*?)\);' % name, header, re.S).group(1)
    assert len(decl.split(',')) == len(_lib.SYMBOLS[name][1]) == 14
    assert 'KFNet/KFNet.py:361-403' in header and 'tools/util.py:36-94' in header
    ARG = -1
    store = np.zeros(64 + 4, np.float32)
    buf = store.ctypes.data + (-store.ctypes.data) % 16
    bd = _lib.FilterBackwardDesc(S=1, T=4, H=5, W=7, ld_dpred=16, radius=4, min_uncertainty=1e-5)

    def call(d=bd, **kw):
        a = dict(flow=buf, st=buf, meas=buf, temp=buf, kf=buf, d_temp=buf, d_kf=buf, dpred=buf, d_flow=buf, d_st=buf, stats=buf,
                 scratch=buf)
        a.update(kw)
        return lib.kfn_filter_backward_joint(C.byref(d), a['flow'], a['st'], a['meas'], a['temp'], a['kf'], a['d_temp'], a['d_kf'],
                                             a['dpred'], a['d_flow'], a['d_st'], a['stats'], a['scratch'], None)
    for k in ('flow', 'st', 'meas', 'temp', 'kf', 'd_temp', 'd_kf', 'dpred', 'd_flow', 'd_st', 'stats', 'scratch'):
        assert call(**{k: None}) == ARG and b'null' in lib.kfn_last_error(), k
    assert call(d_flow=buf + 4) == ARG and b'misaligned' in lib.kfn_last_error()
    assert call(flow=buf + 4) == ARG and call(d_kf=buf + 8) == ARG and call(scratch=buf + 8) == ARG
    bad = _lib.FilterBackwardDesc(S=1, T=4, H=5, W=7, ld_dpred=16, radius=3, min_uncertainty=1e-5)
    assert call(bad) == ARG and b'radius' in lib.kfn_last_error()
    bad = _lib.FilterBackwardDesc(S=1, T=4, H=5, W=7, ld_dpred=16, radius=65, min_uncertainty=1e-5)
    assert call(bad) == ARG and b'radius' in lib.kfn_last_error()
    bad = _lib.FilterBackwardDesc(S=1, T=4, H=5, W=7, ld_dpred=16, radius=4, min_uncertainty=1e-5)
    bad.struct_size = 8
    assert call(bad) == ARG and b'struct_size' in lib.kfn_last_error()
    bad = _lib.FilterBackwardDesc(S=1, T=4, H=1, W=7, ld_dpred=16, radius=4, min_uncertainty=1e-5)
    assert call(bad) == ARG and b'shape' in lib.kfn_last_error()
    bad = _lib.FilterBackwardDesc(S=1, T=4, H=5, W=7, ld_dpred=3, radius=4, min_uncertainty=1e-5)
    assert call(bad) == ARG


# -- the command line ----------------------------------------------------------------------------------------------------------------
def _cli(*args):
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    # a refusal must come before any device is touched: hide them all, so that touching one would be a traceback instead
    env['HIP_VISIBLE_DEVICES'] = env['CUDA_VISIBLE_DEVICES'] = ''
    return subprocess.run([sys.executable, '-m', 'kfnet_amd.KFNet.train'] + list(args), cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def test_command_line_refusals_exit_with_status_1_before_any_device(tmp_path):
    r = _cli('--help')
    assert r.returncode == 0 and '--joint' in r.stdout and '--fix_flownet' in r.stdout
    base = ['--scene', 'fire', '--model_folder', str(tmp_path), '--synthetic', '8', '--height', '64', '--width', '96']
    cases = ((base, ('training OFlowNet is not built', '--joint', '--fix_flownet')),
             (base + ['--joint', '--fix_flownet'], ('--joint', '--fix_flownet')),
             (base + ['--joint', '--augment'], ('--augment',)),
             (base[:-1] + ['100', '--joint'], ('multiples of 8',)),
             (base[:5] + ['3'] + base[6:] + ['--joint'], ('no group',)))
    for args, words in cases:
        r = _cli(*args)
        assert r.returncode == 1 and 'Traceback' not in r.stderr and r.stdout == '', (args, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, (args, r.stderr)
        for word in words:
            assert word in r.stderr, (args, word, r.stderr)
    assert os.listdir(str(tmp_path)) == []
    from kfnet_amd.KFNet.train import build_parser
    a = build_parser().parse_args(['--joint'])
    assert a.joint and not a.fix_flownet
    assert not build_parser().parse_args(['--fix_flownet']).joint


def test_graph_api_keeps_refusing_to_train_oflownet():
    from kfnet_amd.KFNet.KFNet import KFNet
    with pytest.raises(NotImplementedError):
        KFNet(None, None, train_oflownet=True)


# -- state files ---------------------------------------------------------------------------------------------------------------------
class _FlatTrainer(ParamStore):
    """What load_state touches of a trainer: the parameter store both trainers are, on CPU tensors, its Adam slots holding 9."""

    def __init__(self, names):
        ParamStore.__init__(self, [(n, (3,)) for n in names])
        self.m.fill_(9.0)
        self.v.fill_(9.0)


def _state(names, step):
    st = dict(global_step=np.int64(step), adam_t=np.int64(step))
    for n in names:
        st['adam_m/' + n] = np.full(3, 1.0, np.float32)
        st['adam_v/' + n] = np.full(3, 2.0, np.float32)
    return st


def test_state_files_of_the_older_kinds_load_with_the_stated_line(capsys):
    from kfnet_amd.train_kfnet import KFNetTrainer
    sc_names, ft_names = ['ScoreNet/conv1a/kernel', 'ScoreNet/conv1a/bias'], ['Temporal/feat1/kernel']
    assert split_state(_state(sc_names, 5)) == {'ScoreNet': True, 'Temporal': False}
    assert split_state(_state(ft_names, 5)) == {'ScoreNet': False, 'Temporal': True}
    assert split_state(_state(sc_names + ft_names, 5)) == {'ScoreNet': True, 'Temporal': True}
    for held, lacking, names in (('ScoreNet', 'Temporal', sc_names), ('Temporal', 'ScoreNet', ft_names), (None, None, sc_names + ft_names)):
        tr = KFNetTrainer.__new__(KFNetTrainer)
        tr.train_flownet, tr.sc, tr.ft = True, _FlatTrainer(sc_names), _FlatTrainer(ft_names)
        tr.load_state(_state(names, 7))
        out = capsys.readouterr().out
        assert tr.global_step == 7 and tr.adam_t == 7
        for scope, t in (('ScoreNet', tr.sc), ('Temporal', tr.ft)):
            if scope == lacking:
                assert not t.m.any() and not t.v.any()
                assert 'the train state holds no Adam slots of %s/*: they start at zero' % scope in out
            else:
                assert t.m[:3].tolist() == [1.0] * 3 and t.v[:3].tolist() == [2.0] * 3
                assert scope + '/*' not in out
    # the fixed path reads its own scope and ignores the other's slots
    tr = KFNetTrainer.__new__(KFNetTrainer)
    tr.train_flownet = False

    class Fixed(_FlatTrainer):
        def load_state(self, st):
            self._fill(self.m, st, 'adam_m/')
            self.global_step = int(st['global_step'])
    tr.sc = Fixed(sc_names)
    tr.load_state(_state(sc_names + ft_names, 3))
    assert tr.global_step == 3 and tr.sc.m[:3].tolist() == [1.0] * 3 and capsys.readouterr().out == ''
