"""CPU tests (no GPU): which kernel route every convolution of a graph ends on, as a snapshot.

One line per ConvOp of `g.ops` after Graph.resolve_routes() and Graph.assign_layouts(): class, packers, routing
options as found in the op's __dict__, workspace, the bytes of desc(), kernel name, workgroups, executed FLOPs and
the tensor layouts.  tests/golden/routes.json holds the lines recorded on the commit BEFORE kfnet_amd/routing.py
existed (`python tests/test_routes_host.py --record FILE` run against that checkout, where the route fix-ups after
concat re-binding were the ops' own resolve() methods); it is never re-recorded from the tree under test.  A routing
change that is meant re-records it from its own parent and says which lines moved.

The one difference the snapshot allows: routing options of a class an op has LEFT.  The recorded commit kept a stale
`k_split` / `f42` in the __dict__ of an op that set_epilogue had moved to the direct kernel; here they must be gone
(OPTIONS_OF below), and the private split-K workspace of such an op must have left g.storages.
"""
import json
import os
import sys

import pytest

if __name__ == '__main__':      # the recorder runs against another checkout: its root is the working directory
    sys.path.insert(0, os.getcwd())

from kfnet_amd import _lib
from kfnet_amd.cnn_wrapper.network import Network
from kfnet_amd.graph import ConvOp, Graph, variable_scope
from kfnet_amd.KFNet.KFNet import KFNet, KFNetDataSpec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'routes.json')
FIELDS = ('name', 'class', 'kernel_pack', 'bias_pack', 'k_split', 'eight_wave', 'f42', 'workspace', 'workspace_numel',
          'desc', 'kernel_name', 'workgroups', 'mfma_flops', 'x_layout', 'y_layout')
# the routing options each class owns; every other class must carry none of them
OPTIONS_OF = {'WinogradF43ConvOp': ('k_split', 'eight_wave'), 'WinogradS2ConvOp': ('k_split', 'eight_wave', 'f42')}


def _resolve(g):
    g.resolve_routes()


def snapshot(g, resolve=_resolve):
    resolve(g)
    g.assign_layouts()
    lib = _lib.load()
    lines = []
    for op in g.ops:
        if not isinstance(op, ConvOp):
            continue
        ws = getattr(op, 'workspace', None)
        kind = None if ws is None else ('shared' if ws is g.winograd_ws else 'private')
        wgs = op.launch_workgroups() if hasattr(op, 'launch_workgroups') else op.workgroups(lib)
        lines.append([op.name, type(op).__name__, op.kernel.pack.__name__,
                      None if op.bias is None else op.bias.pack.__name__,
                      op.__dict__.get('k_split'), op.__dict__.get('eight_wave'), op.__dict__.get('f42'),
                      kind, None if ws is None else ws.numel, bytes(op.desc()).hex(), op.kernel_name(lib), wgs,
                      op.mfma_flops(), op.x.layout, op.y.layout])
    return lines


def orphaned_storages(g):
    """Buffers of g.storages that no op reaches: neither a tensor's nor a workspace's."""
    held = {id(g.winograd_ws)}
    for op in g.ops:
        held.update(id(t.root_storage) for _, t in Graph._tensor_refs(op))
        if getattr(op, 'workspace', None) is not None:
            held.add(id(op.workspace))
    return [s for s in g.storages if id(s) not in held]


# ---- the product graphs ------------------------------------------------------------------------------------
def _kfnet(B=2, H=480, W=640, **graph_options):
    g = Graph()
    for k, v in graph_options.items():
        assert hasattr(g, k), k
        setattr(g, k, v)
    img = g.placeholder((B, H, W, 3), 'u8')
    st = g.placeholder((1, -(-H // 8), -(-W // 8), 4))
    net = KFNet(img, KFNetDataSpec(batch_size=B, image_size=(H, W)))
    net.GetKFCoordRecursive(st.channels(0, 3), st.channels(3, 1))
    return g


SWITCHES = [dict(winograd_f43_eight_wave=False), dict(winograd_s2_f42=False),
            dict(winograd_s2_eight_wave=False, winograd_s2_f42=False), dict(winograd_s2_eight_wave=False, winograd_s2_f42=True),
            dict(winograd_f43_min_channels=0), dict(winograd_f43_max_k_split=1), dict(winograd_f43_min_workgroups=0),
            dict(winograd_s2_max_k_split=1), dict(winograd_fused=False), dict(winograd_fused=False, winograd_min_channels=0),
            dict(winograd_s2_min_channels=0), dict(window_fc=False), dict(activation_layout_c16=False),
            dict(lds_bytes_per_cu=65536), dict(factor_cost_volume=False), dict(fuse_cost_volume=False),
            dict(fuse_oflow_window=False)]
KFNET_CASES = ([dict(B=b) for b in (1, 2, 4, 20, 32)] + [dict(B=8, H=64, W=96)]
               + [dict(B=2, H=540, W=960, conv_operands='f16'),
                  dict(B=2, H=540, W=960, conv_operands='f16', conv64_rows_f16=False, f16_activation_scopes=()),
                  dict(B=2, conv_operands='f16x3')]
               + [dict(B=b, **sw) for sw in SWITCHES for b in (1, 4, 20)])


def _case_id(case):
    return ','.join('%s=%s' % (k, case[k]) for k in sorted(case))


# ---- the fallbacks the product graphs never take: small networks, re-bound through concat -------------------------
class _Cat(Network):
    """One 3x3 layer 'a' whose output a concat with a 2-channel tensor re-binds to a window of pixel stride Cout + 2."""

    def __init__(self, inputs, filters, stride):
        self.filters, self.stride = filters, stride
        Network.__init__(self, inputs, is_training=False)

    def setup(self):
        self.feed('input').conv(3, self.filters, self.stride, name='a')
        self.feed('a', 'side').concat(3, name='cat')


def _cat_graph(shape, filters, stride, **graph_options):
    g = Graph()
    for k, v in graph_options.items():
        assert hasattr(g, k), k
        setattr(g, k, v)
    n, h, w, _ = shape
    x = g.placeholder(shape, name='input')
    side = g.placeholder((n, -(-h // stride), -(-w // stride), 2), name='side')
    net = _Cat({'input': x, 'side': side}, filters, stride)
    return g, net.ops[0]


# (id, input shape, filters, stride, graph options, class / options before resolve_routes, class / options after)
FALLBACKS = [
    ('f43_to_fused', (32, 64, 96, 64), 64, 1, {}, ('WinogradF43ConvOp', dict(k_split=1)), ('WinogradFusedConvOp', {})),
    # (a single frame has 12 workgroups: below winograd_f43_min_workgroups the chooser would not pick F(4x4) at all)
    ('f43_splitk_to_fused', (1, 64, 96, 64), 64, 1, dict(winograd_f43_min_workgroups=0),
     ('WinogradF43ConvOp', dict(split=True)), ('WinogradFusedConvOp', {})),
    # (32 workgroups and no fused F(2x2) form to compete with on a 4-pixel-wide map: split-K here too)
    ('f43_to_direct', (32, 32, 4, 64), 64, 1, {}, ('WinogradF43ConvOp', dict(split=True)), ('ConvOp', {})),
    # (192 workgroups of the F(4,2) form: the chooser takes it from winograd_s2_f42_min_workgroups = 1024 up)
    ('s2_f42_to_eight_wave', (32, 64, 96, 64), 128, 2, dict(winograd_s2_f42_min_workgroups=1),
     ('WinogradS2ConvOp', dict(f42=True)), ('WinogradS2ConvOp', dict(f42=False, eight_wave=True, k_split=1))),
    ('s2_splitk_to_unsplit', (1, 64, 96, 64), 128, 2, {},
     ('WinogradS2ConvOp', dict(f42=False, eight_wave=True, split=True)), ('WinogradS2ConvOp', dict(f42=False, eight_wave=True, k_split=1))),
]


class _Two(Network):
    def __init__(self, inputs, filters, stride):
        self.filters, self.stride = filters, stride
        Network.__init__(self, inputs, is_training=False)

    def setup(self):
        self.feed('input').conv(3, self.filters, 1, name='a').conv(3, self.filters, self.stride, name='b')


def _epilogue_graph(shape, filters, stride, dtype='f32', **graph_options):
    g = Graph()
    for k, v in graph_options.items():
        assert hasattr(g, k), k
        setattr(g, k, v)
    x = g.placeholder(shape, dtype=dtype, name='input')
    with variable_scope('S'):
        net = _Two({'input': x}, filters, stride)
    return g, net, [op for op in net.ops if op.name == 'b'][0]


# (id, input shape, channels, stride of 'b', graph options, class / options of 'b' before set_epilogue, class after)
EPILOGUES = [
    ('two_kernel_winograd', (2, 16, 16, 128), 128, 1, dict(winograd_fused=False), ('WinogradConvOp', {}), 'ConvOp'),
    ('fused_f2x2', (2, 16, 16, 32), 32, 1, {}, ('WinogradFusedConvOp', {}), 'ConvOp'),
    ('f43', (32, 64, 96, 64), 64, 1, {}, ('WinogradF43ConvOp', dict(k_split=1)), 'ConvOp'),
    ('f43_splitk', (1, 64, 96, 64), 64, 1, dict(winograd_f43_min_workgroups=0), ('WinogradF43ConvOp', dict(split=True)), 'ConvOp'),
    ('s2_f42', (32, 64, 96, 128), 128, 2, dict(winograd_s2_f42_min_workgroups=1), ('WinogradS2ConvOp', dict(f42=True)), 'ConvOp'),
    ('s2_eight_wave_splitk', (1, 64, 96, 128), 128, 2, {}, ('WinogradS2ConvOp', dict(eight_wave=True, split=True)), 'ConvOp'),
    # the window matrix runs through the direct kernel's 1x1 path, which carries the epilogues: it stays
    ('window_matrix', (8, 2, 2, 32), 32, 1, {}, ('WindowFcConvOp', {}), 'WindowFcConvOp'),
    ('conv64_rows_f16', (2, 64, 96, 64), 64, 1, dict(conv_operands='f16', f16_activation_scopes=('S',)), ('Conv64RowsF16Op', {}), 'ConvOp'),
]


def _is(op, want):
    kind, options = want
    have = dict(op.__dict__, split=op.__dict__.get('k_split', 1) > 1)      # split: into how many runs is the cost model's business
    return type(op).__name__ == kind and all(have.get(k) == v for k, v in options.items())


def all_snapshots(resolve=_resolve):
    """case id -> lines, every case of this file."""
    out = {}
    for case in KFNET_CASES:
        out['kfnet:' + _case_id(case)] = snapshot(_kfnet(**case), resolve)
    for cid, shape, filters, stride, opts, before, after in FALLBACKS:
        g, op = _cat_graph(shape, filters, stride, **opts)
        assert _is(op, before) and op.y.ld == filters + 2, (cid, type(op).__name__, op.__dict__)
        out['fallback:' + cid] = snapshot(g, resolve)
        assert _is(op, after), (cid, type(op).__name__, op.__dict__)
    for cid, shape, filters, stride, opts, before, after in EPILOGUES:
        g, net, op = _epilogue_graph(shape, filters, stride, dtype='f16' if cid == 'conv64_rows_f16' else 'f32', **opts)
        assert _is(op, before), (cid, type(op).__name__, op.__dict__)
        net.set_epilogue('b', _lib.EPI_EXP_CH3)
        assert type(op).__name__ == after and op.epilogue == _lib.EPI_EXP_CH3, (cid, type(op).__name__)
        out['epilogue:' + cid] = snapshot(g, resolve)
    return out


# ---- the fixture: a table of distinct lines + per case the indices into it ----------------------------------------
def _write_golden(path, snaps):
    table, index, cases = [], {}, {}
    for cid, lines in snaps.items():
        cases[cid] = [index.setdefault(json.dumps(ln), len(index)) for ln in lines]
    table = [json.loads(k) for k in sorted(index, key=index.get)]
    with open(path, 'w') as f:
        json.dump({'fields': list(FIELDS), 'lines': table, 'cases': cases}, f, separators=(',', ':'))
        f.write('\n')


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert gold['fields'] == list(FIELDS)
    return {cid: [gold['lines'][i] for i in idx] for cid, idx in gold['cases'].items()}


@pytest.fixture(scope='module')
def snaps():
    return all_snapshots()


def _without_left_options(line):
    """The line with the options its class does not own blanked (what the recorded commit left behind in __dict__)."""
    rec = dict(zip(FIELDS, line))
    for opt in ('k_split', 'eight_wave', 'f42'):
        if opt not in OPTIONS_OF.get(rec['class'], ()):
            rec[opt] = None
    return rec


def test_every_case_is_recorded(golden, snaps):
    assert sorted(golden) == sorted(snaps)
    assert os.path.getsize(GOLDEN) <= 283504        # tests/golden/kfnet_full.npz, the largest fixture before this one


@pytest.mark.parametrize('kind', ['kfnet', 'fallback', 'epilogue'])
def test_routes_match_the_recorded_ones(golden, snaps, kind):
    checked = 0
    for cid in sorted(snaps):
        if not cid.startswith(kind + ':'):
            continue
        got, want = snaps[cid], golden[cid]
        assert [ln[0] for ln in got] == [ln[0] for ln in want], cid
        for g_line, w_line in zip(got, want):
            assert dict(zip(FIELDS, g_line)) == _without_left_options(w_line), cid
            checked += 1
    assert checked > 0


def test_an_op_that_left_a_route_keeps_nothing_of_it():
    """After every re-route (set_epilogue, the fix-ups after concat re-binding): no routing option of the class the op left,
    and a private split-K workspace is gone from g.storages, not merely from the op."""
    for cid, shape, filters, stride, opts, before, after in FALLBACKS:
        g, op = _cat_graph(shape, filters, stride, **opts)
        had_ws = op.__dict__.get('workspace')
        assert (had_ws is not None) == bool(before[1].get('split')), cid
        g.resolve_routes()
        assert not orphaned_storages(g), cid
        assert had_ws is None or had_ws not in g.storages, cid
        for opt in ('k_split', 'eight_wave', 'f42'):
            assert (opt in op.__dict__) == (opt in OPTIONS_OF.get(type(op).__name__, ())), (cid, opt)
        assert op.__dict__.get('k_split', 1) == 1 and getattr(op, 'workspace', None) is None, cid
    for cid, shape, filters, stride, opts, before, after in EPILOGUES:
        g, net, op = _epilogue_graph(shape, filters, stride, dtype='f16' if cid == 'conv64_rows_f16' else 'f32', **opts)
        had_ws = op.__dict__.get('workspace')
        assert (had_ws is not None) == (before[0] == 'WinogradConvOp' or bool(before[1].get('split'))), cid
        net.set_epilogue('b', _lib.EPI_EXP_CH3)
        g.resolve_routes()
        assert not orphaned_storages(g), cid
        assert had_ws is None or had_ws is g.winograd_ws or had_ws not in g.storages, cid
        for opt in ('k_split', 'eight_wave', 'f42'):
            assert opt not in op.__dict__, (cid, opt)
        assert getattr(op, 'workspace', None) is None, cid


def test_a_packed_op_refuses_another_route_once_with_both_kernel_names():
    g, net, op = _epilogue_graph((32, 64, 96, 64), 64, 1)
    op.kernel.storage = object()         # what Graph.load_weights leaves: the weights are on the device in the F(4x4) layout
    with pytest.raises(RuntimeError) as err:
        net.set_epilogue('b', _lib.EPI_EXP_CH3)
    assert 'b' in str(err.value) and 'wino4b_kernel' in str(err.value) and 'conv_mfma_kernel' in str(err.value)
    assert type(op).__name__ == 'WinogradF43ConvOp' and op.epilogue == _lib.EPI_NONE


if __name__ == '__main__':
    def _own_resolve(g):        # the recorded commit: every op fixed its own route up (what its Graph.finalize did)
        for op in g.ops:
            if hasattr(op, 'resolve'):
                op.resolve()
    assert sys.argv[1] == '--record' and not hasattr(Graph, 'resolve_routes'), 'record on the commit before routing.py only'
    _write_golden(sys.argv[2], all_snapshots(_own_resolve))
