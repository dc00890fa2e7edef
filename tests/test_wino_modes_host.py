"""Host checks of the Winograd kernels' case table (tests/wino_modes.py): pair coverage, reproducibility, generation time, that
the table reaches the branches it is for (dword-store epilogues, the decoding of the workgroup order), the exactness premises of
the fp16-operand cases, and the test's own transform matrices."""
import time

import numpy as np

from oracle import kfnet_oracle as O
from tests import wino_modes as WM

PAIRS, ALLOWED, CASES = 2057, 1642, 170      # of the table as committed (SEED 23); EXTRA adds 19 cases


def test_table_covers_every_allowed_pair_and_is_quick_to_make():
    t0 = time.perf_counter()
    cases = WM.TABLE.generate(WM.SEED)
    dt = time.perf_counter() - t0
    allowed = WM.TABLE.allowed_pairs()
    covered = set()
    for c in cases:
        assert WM.TABLE.valid(c._asdict()), c
        covered |= WM.TABLE.pairs_of(c)
    missing = [p for p in allowed if p not in covered]
    assert not missing, missing[:10]
    dword = sum(WM.store_path(c) == 'dword' for c in cases)
    print('%d of %d pairs allowed, %d cases (%d on a dword-store path) + %d extra, generated in %.2f s'
          % (len(allowed), len(WM.TABLE.all_pairs()), len(cases), dword, len(WM.EXTRA), dt))
    assert (len(WM.TABLE.all_pairs()), len(allowed), len(cases)) == (PAIRS, ALLOWED, CASES)
    assert cases == WM.table()                      # reproducible from its seed
    assert dt < 5.0, 'the table slows collection: %.1f s' % dt
    assert all(WM.TABLE.valid(c._asdict()) for c in WM.EXTRA)
    # every level of every factor is usable at all
    assert {q for p in allowed for q in p} == {(n, l) for n in WM.NAMES for l in WM.FACTORS[n]}


def test_rules_allow_and_refuse_what_the_launchers_do():
    ok = set(WM.TABLE.allowed_pairs())

    def pair(fa, la, fb, lb):
        return tuple(sorted([(fa, la), (fb, lb)], key=lambda t: WM.NAMES.index(t[0])))
    # kfn_conv2d_winograd_fused's routing
    assert pair('kernel', 'w3p', 'cout', 36) in ok and pair('kernel', 'w3p', 'cout', 100) not in ok
    assert pair('kernel', 'w3', 'cin', 48) not in ok and pair('kernel', 'w3h', 'cin', 32) not in ok and pair('kernel', 'w3h', 'cin', 128) in ok
    assert pair('kernel', 'w3', 'cout', 100) not in ok and pair('kernel', 'w2', 'cout', 384) in ok
    # the dword epilogues: seven kernels, and k_split = 1 of the stride-2 split-K entry point (it IS s2_launch)
    for k in WM.KERNELS:
        has = k in WM.DWORD_KERNELS or k == 's2bk'
        assert (pair('kernel', k, 'yview', 'off') in ok) == has and (pair('kernel', k, 'yview', 'ld') in ok) == has, k
        assert (pair('kernel', k, 'cout', 130) in ok) == (has and k != 'w3p'), k
    assert pair('yview', 'off', 'ksplit', 1) in ok and pair('yview', 'off', 'ksplit', 2) not in ok
    # 8-byte aligned x: wino4_setup only; channel-blocked tensors: wino4b_kernel and wino_s2c_kernel, dense, Cout % 16
    assert pair('kernel', 'f43a', 'xview', 'x8') in ok and pair('kernel', 's2c', 'xview', 'x8') not in ok and pair('kernel', 'w2', 'xview', 'x8') not in ok
    assert pair('kernel', 'f43b', 'layout', 'c16both') in ok and pair('kernel', 'f43bk', 'layout', 'c16in') not in ok
    assert pair('xview', 'pad', 'layout', 'c16in') not in ok and pair('xview', 'pad', 'layout', 'c16out') in ok
    assert pair('cout', 100, 'layout', 'c16out') not in ok and pair('cout', 100, 'layout', 'c16in') in ok
    # split-K: k_split <= Cin / 16, no empty run of super-steps
    assert pair('cin', 16, 'ksplit', 2) not in ok and pair('cin', 64, 'ksplit', 3) not in ok and pair('cin', 48, 'ksplit', 3) in ok
    assert pair('cin', 128, 'ksplit', 3) in ok and pair('kernel', 's2b', 'ksplit', 1) not in ok and pair('kernel', 's2bk', 'ksplit', 0) not in ok


def test_n_group_rules():
    """wino4_setup: AUTO = 4 | 2 | 1 groups, a request that does not divide tiles_n falls back to 1; s2_launch and launch_wino_s2c:
    AUTO = 2 when tiles_n is even, else all, and the fallback is all."""
    ng = WM.n_group
    assert [ng('f43b', t, 'auto') for t in (1, 2, 3, 4, 6, 8)] == [1, 2, 1, 4, 2, 4]
    assert [ng('s2a', t, 'auto') for t in (1, 2, 3, 4)] == [1, 2, 3, 2] and [ng('s2c', t, 'auto') for t in (1, 2, 3, 4)] == [1, 2, 3, 2]
    assert ng('f43a', 6, 'g3') == 3 and ng('f43a', 6, 'g4') == 1 and ng('f43a', 3, 'g2') == 1 and ng('f43a', 2, 'g3') == 1
    assert ng('s2b', 3, 'g3') == 3 and ng('s2b', 3, 'g2') == 3 and ng('s2bk', 1, 'g2') == 1 and ng('s2c', 3, 'g4') == 3
    assert ng('s2ah', 3, 'm') == 1 and ng('f43bk', 6, 'n') == 6 and ng('w3', 3, 'n') == 3 and ng('w3h', 3, 'g2') == 1
    assert ng('w2', 12, 'n') is None and ng('w3p', 1, 'n') is None


def test_table_reaches_the_order_decoding_of_every_kernel():
    cs = [c for _, c in WM.cases()]
    for k in WM.GROUP_KERNELS:
        gs = [WM.geometry(c) for c in cs if c.kernel == k]
        assert any(1 < g['n_group'] < g['tiles_n'] for g in gs), k
        assert any(g['tiles_n'] >= 3 for g in gs), k
        assert any(g['fallback'] for g in gs), k
    for k in WM.FAST_KERNELS:
        got = {c.order for c in cs if c.kernel == k and WM.geometry(c)['tiles_n'] >= 3}
        assert {'m', 'n'} <= got, (k, got)


def test_table_reaches_every_dword_store_epilogue():
    cs = [c for _, c in WM.cases()]
    for k in WM.DWORD_KERNELS:
        mine = [c for c in cs if c.kernel == k and WM.store_path(c) == 'dword']
        assert any(c.cout % 4 for c in mine), k
        assert any(c.yview == 'ld' for c in mine) and any(c.yview == 'off' for c in mine), k
        assert any(WM.geometry(c)['straddle'] for c in mine), k
        assert any(WM.geometry(c)['ho'] % 2 and WM.geometry(c)['wo'] % 2 for c in mine), k
        assert all(WM.store_path(c) == 'wide' for c in cs if c.kernel == k and c.yview == 'pad' and c.cout % 4 == 0)
    assert not [c for c in cs if WM.store_path(c) == 'dword' and not WM._dword_ok(c.kernel, c.ksplit)]


def test_fp16_cases_multiply_exact_operands():
    """The premise of holding the fp16-operand kernels to their fp32 siblings' bound: on the gridded inputs the packed U is
    exactly representable in fp16 and normal, V = B^T d B is exact in fp32 (so the kernel's fp32 transform, in any order,
    yields it), and rounding V to fp16 does change values -- the rounding mode is exercised."""
    from kfnet_amd.graph import pack_winograd_fused_kernel, pack_winograd_s2_kernel
    seen = set()
    changed = total = 0
    for i, c in WM.cases():
        if not WM.KERNELS[c.kernel][3]:
            continue
        fam = WM.FAMILY[c.kernel]
        x, w, _ = WM.make_inputs(i, c)
        u32 = WM.unpack_u(fam, (pack_winograd_fused_kernel if fam == 'f23' else pack_winograd_s2_kernel)(w), c.cin, c.cout)
        u16 = WM.packed_f16(c, w)
        exact = WM.transformed_weights(fam, w)
        for a, b, e in zip(*[(t,) if fam == 'f23' else t for t in (u16, u32, exact)]):
            assert np.array_equal(a, b) and np.array_equal(a, e), (i, c)
            nz = np.abs(a[a != 0])
            assert nz.min() >= 2.0 ** -14, (i, c, nz.min())       # normal in fp16
        v = WM.input_transform(fam, x)
        for a in ((v,) if fam == 'f23' else v):
            assert np.array_equal(a, a.astype(np.float32).astype(np.float64)), (i, c)
            assert np.abs(a).max() <= 16 * WM.X_MAX
            changed += int((WM.round_f16(a) != a).sum())
            total += a.size
        seen.add(c.kernel)
    print('fp16 rounding changes %d of %d V values (%.1f %%)' % (changed, total, 100.0 * changed / total))
    assert seen == {'w3h', 's2ah'} and changed > total // 100


def test_winograd_way_reference_equals_the_direct_one():
    """The test's own B^T, G, A^T: on fp32 cases of the two families the fp16 reference is written for, the fp64 direct
    convolution and the fp64 Winograd-way one (unrounded V and U) agree to 1e-12 relative."""
    done = {}
    for i, c in WM.cases():
        fam = WM.FAMILY[c.kernel]
        if fam not in ('f23', 's2') or WM.KERNELS[c.kernel][3] or done.get((fam, c.img)):
            continue
        done[(fam, c.img)] = True
        x, w, b = WM.make_inputs(i, c)
        g = WM.geometry(c)
        ref = WM.reference(c, x, w, b)
        alt = WM.wino_reference(fam, x, WM.transformed_weights(fam, w), b, bool(c.relu), (g['ho'], g['wo']))
        assert ref.shape == alt.shape
        assert np.abs(ref - alt).max() <= 1e-12 * np.abs(ref).max(), (i, c)
    assert len(done) == 8          # every image of both families


def test_persistent_list_satisfies_the_launchers_rule():
    for cu in (256, 304, 64):
        cs = WM.persistent_cases(cu)
        assert [c.order for _, c in cs] == list(WM.ORDERS)
        assert {c.relu for _, c in cs} == {0, 1} and {c.bias for _, c in cs} == {0, 1} and {c.layout for _, c in cs} == set(WM.LAYOUTS)
        for _, c in cs:
            assert WM.TABLE.valid(dict(c._asdict(), img=(2, 40, 48)))      # (the rules know the table's images only)
            assert c.cin in (32, 64) and c.cout in (384, 512) and c.img[1:] == (40, 48)
            assert WM.s2c_persistent(c.img[0], 40, 48, c.cin, c.cout, cu)
        ns = sorted({c.img[0] for _, c in cs if c.cout == 512})
        assert len(ns) == 2 and ns[1] == ns[0] + 3 and not WM.s2c_persistent(ns[0] - 1, 40, 48, 32, 512, cu)
        if cu == 256:
            assert ns[0] == 51
