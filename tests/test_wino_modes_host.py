"""Host checks of the Winograd kernels' case table (tests/wino_modes.py): pair coverage, reproducibility, generation time, that
the table reaches the branches it is for (dword-store epilogues, the decoding of the workgroup order), the exactness premises of
the fp16-operand cases, and the test's own transform matrices; then the table against the launchers' own launch plan
(kfn_winograd_launch_plan): every case, every refusal, and that the library's three readings of a plan agree."""
import collections
import time

import numpy as np

from kfnet_amd import _lib
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
    # 8-byte aligned x: the F(4x4,3x3) launcher only; channel-blocked tensors: wino4b_kernel and wino_s2c_kernel, dense, Cout % 16
    assert pair('kernel', 'f43a', 'xview', 'x8') in ok and pair('kernel', 's2c', 'xview', 'x8') not in ok and pair('kernel', 'w2', 'xview', 'x8') not in ok
    assert pair('kernel', 'f43b', 'layout', 'c16both') in ok and pair('kernel', 'f43bk', 'layout', 'c16in') not in ok
    assert pair('xview', 'pad', 'layout', 'c16in') not in ok and pair('xview', 'pad', 'layout', 'c16out') in ok
    assert pair('cout', 100, 'layout', 'c16out') not in ok and pair('cout', 100, 'layout', 'c16in') in ok
    # split-K: k_split <= Cin / 16, no empty run of super-steps
    assert pair('cin', 16, 'ksplit', 2) not in ok and pair('cin', 64, 'ksplit', 3) not in ok and pair('cin', 48, 'ksplit', 3) in ok
    assert pair('cin', 128, 'ksplit', 3) in ok and pair('kernel', 's2b', 'ksplit', 1) not in ok and pair('kernel', 's2bk', 'ksplit', 0) not in ok


def test_n_group_rules():
    """wino_f43_plan: AUTO = 4 | 2 | 1 groups, a request that does not divide tiles_n falls back to 1; wino_s2_plan and wino_s2c_plan:
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


# ---- the table against the launchers' own plan (kfn_winograd_launch_plan: the function every launcher launches from) ----------
K = _lib
PLAN_KERNEL = {'w3p': K.WINO_KERNEL_WINO3_PAIR, 'w3': K.WINO_KERNEL_WINO3, 'w3h': K.WINO_KERNEL_WINO3_F16, 'f43a': K.WINO_KERNEL_WINO4,
               'f43b': K.WINO_KERNEL_WINO4B, 'f43bk': K.WINO_KERNEL_WINO4B, 's2a': K.WINO_KERNEL_S2, 's2ah': K.WINO_KERNEL_S2_F16,
               's2b': K.WINO_KERNEL_S2B, 's2bk': K.WINO_KERNEL_S2B, 's2c': K.WINO_KERNEL_S2C}
THREADS = {'w2': 64, 'w3p': 128, 'w3': 256, 'w3h': 256, 'f43a': 256, 'f43b': 512, 'f43bk': 512, 's2a': 256, 's2ah': 256, 's2b': 512,
           's2bk': 512, 's2c': 512}


def _fields(c):
    """The descriptor gpu_util.run_winograd sends for case c, and the low bits of the output address (its buffers come
    from the allocator 16-byte aligned; the window starts y_off floats in).  The layouts are set after the fact, so that a
    blocked tensor that is NOT dense -- which run_winograd cannot build -- can be described too."""
    from tests.gpu_util import winograd_fields
    kind = WM.KERNELS[c.kernel][1]
    xl, yl = WM.LAYOUTS[c.layout]
    fields, _, y_off = winograd_fields(kind, tuple(c.img) + (c.cin,), c.cout, **dict(WM.launch_args(c), x_layout='nhwc', y_layout='nhwc'))
    fields.update(x_layout=_lib.LAYOUT_C16 if xl == 'c16' else 0, y_layout=_lib.LAYOUT_C16 if yl == 'c16' else 0)
    return fields, (4 * y_off) % 16


def _plan(c, cu=256):
    fields, low = _fields(c)
    return _lib.winograd_launch_plan(_lib.ConvDesc(**fields), c.ksplit if WM.KERNELS[c.kernel][4] else c.ksplit and -1, cu, low)


def test_the_launchers_plan_agrees_with_the_table():
    """Every case of the table, and the persistent list on 256 CUs: the kernel, the grid, n_group and the store path the table
    states for it are what the launcher's plan of the descriptor the GPU test sends says."""
    checked = 0
    for i, c in WM.cases() + WM.persistent_cases(256):
        p, g = _plan(c), WM.geometry(c)
        assert p is not None, (i, c, _lib.load().kfn_last_error())
        wide = WM.store_path(c) == 'wide'
        want = PLAN_KERNEL.get(c.kernel) or (K.WINO_KERNEL_WINO2_WIDE if wide else K.WINO_KERNEL_WINO2_DWORD)
        if i >= 2000:
            want = K.WINO_KERNEL_S2C_PERSISTENT
        bh, bw, _ = WM.BLOCK[WM.FAMILY[c.kernel]]
        ks = max(c.ksplit, 1)
        assert (p.kernel, p.threads, p.tiles_m, p.tiles_n, p.wide_store, p.tiles_per_block, p.channels_per_group, p.k_split) == \
            (want, THREADS[c.kernel], g['tiles_m'], g['tiles_n'], int(wide), bh * bw, WM.KERNELS[c.kernel][5], ks), (i, c)
        assert p.workgroups == (256 if i >= 2000 else g['tiles_m'] * g['tiles_n'] * ks), (i, c)
        assert p.ss_per_split == -(-(c.cin // (32 if c.kernel in ('w3', 'w3h') else 16)) // ks), (i, c)
        if g['n_group'] is not None:
            assert p.n_group == g['n_group'], (i, c)
        checked += 1
    assert checked == CASES + len(WM.EXTRA) + 6
    # the persistent rule itself, on other chips and on the table's own F(4,2) cases
    for cu in (64, 256, 304):
        for i, c in WM.cases() + WM.persistent_cases(cu):
            if c.kernel == 's2c':
                persistent = WM.s2c_persistent(c.img[0], c.img[1], c.img[2], c.cin, c.cout, cu)
                assert (_plan(c, cu).kernel == K.WINO_KERNEL_S2C_PERSISTENT) == persistent == (i >= 2000), (cu, i, c)


# What a refused combination of a rule means for the launcher.  'refused': the plan fails.  'elsewhere': the fused entry point
# takes the layer on another of its kernels.  None: not a statement about the launcher -- the images are the table's choice per
# family; a split asked of s2a / s2b IS the s2bk launch and no split asked of f43bk / s2bk IS the f43b / s2b launch; an input
# 8 bytes past a 16-byte boundary is a fact about a pointer, which the F(4,2) plan (ldx % 2 == 0 is all it asks) cannot see.
def _expected(names, combo):
    k = combo.get('kernel')
    if names == ('kernel', 'img'):
        return None
    if names in (('kernel', 'cout'), ('kernel', 'cin')):
        return 'refused' if k == 'w3h' else 'elsewhere'
    if names == ('kernel', 'xview'):
        return None if k == 's2c' else 'refused'
    if names == ('kernel', 'ksplit'):
        return 'refused' if combo['ksplit'] > 0 and k not in ('s2a', 's2b') and not WM.KERNELS[k][4] else None
    return 'refused'


def test_the_plan_refuses_what_the_rules_refuse():
    """Every combination of levels a rule of the table refuses, put into a case that breaks no other rule: the launcher's plan
    refuses that descriptor (or, for the fused entry point's routing, names another kernel)."""
    import itertools
    lib = _lib.load()
    cases = [c for _, c in WM.cases()]
    seen = collections.Counter()
    for names, fn in WM.RULES:
        for levels in itertools.product(*[WM.FACTORS[n] for n in names]):
            if fn(*levels):
                continue
            combo = dict(zip(names, levels))
            want = _expected(names, combo)
            if want is None:
                seen[names, 'no statement'] += 1
                continue
            for base in cases:
                c = base._replace(**combo)
                d = c._asdict()
                if all(f(*[d[n] for n in ns]) for ns, f in WM.RULES if ns != names):
                    break
            else:
                seen[names, 'no case breaks this rule alone'] += 1
                continue
            p = _plan(c)
            if want == 'refused':
                assert p is None and lib.kfn_last_error(), (names, combo, c)
            else:
                assert p is not None and p.kernel != PLAN_KERNEL[c.kernel], (names, combo, c)
            seen[names, want] += 1
    print(sorted(seen.items()))
    # (a combination that cannot stand alone breaks a second rule by itself, e.g. a split asked of f43a with Cout % 4 != 0)
    for names, _ in WM.RULES:
        assert names == ('kernel', 'img') or seen[names, 'refused'] + seen[names, 'elsewhere'] > 0, names
    assert sum(n for (_, what), n in seen.items() if what in ('refused', 'elsewhere')) >= 100


def test_supported_lds_bytes_and_launch_plan_never_disagree():
    """kfn_winograd_*_supported, kfn_winograd_lds_bytes and kfn_winograd_launch_plan are three readings of one plan: over the
    forms, both strides, both operand types, Cin, Cout and ragged / straddling / too-small images they give one answer."""
    import ctypes as C
    import itertools
    lib = _lib.load()
    images = ((1, 32, 32), (2, 29, 12), (3, 30, 34), (2, 40, 48), (2, 7, 9), (5, 20, 24))
    taken = collections.Counter()
    for form, stride, op, cin, cout, (n, h, w), pad in itertools.product(range(6), (1, 2), (0, 1), (16, 32, 48, 64), (36, 64, 128, 130),
                                                                        images, (0, 8, 6)):
        d = _lib.ConvDesc(N=n, H=h, W=w, Cin=cin, ldx=cin, Cout=cout, cout_pad=-(-cout // 32) * 32, ldy=cout + pad, kh=3, kw=3,
                          stride=stride, wino_form=form, operand_dtype=op)
        family = 's2' if stride == 2 else ('f43' if form in (2, 3) else 'fused')
        sup = getattr(lib, 'kfn_winograd_%s_supported' % family)(C.byref(d))
        nb = C.c_int(-1)
        rc = lib.kfn_winograd_lds_bytes(C.byref(d), C.byref(nb))
        p = _lib.winograd_launch_plan(d)
        assert (sup == 1) == (rc == 0) == (p is not None), (form, stride, op, cin, cout, n, h, w, pad, sup, rc)
        if p is not None:
            assert nb.value == p.lds_bytes > 0 and p.workgroups == p.tiles_m * p.tiles_n > 0
            taken[p.kernel] += 1
        taken[family, p is not None] += 1
    assert all(taken[k] for k in range(1, 12)), taken          # every kernel but the persistent one (no image here fills 256 CUs twice)
    assert all(taken[f, ok] for f in ('fused', 'f43', 's2') for ok in (True, False)), taken


def test_lds_bytes_follows_the_launcher_past_the_two_wave_forms_byte_range():
    """Where kfn_winograd_lds_bytes had drifted from the launcher: a 64-channel layer whose two input images take exactly 2^30
    bytes.  The two-wave form needs them BELOW 1 GiB (bits 30 and 31 of its patch offsets are marks), so the launcher runs
    wino2_kernel with WINO2_LDS_BYTES = 32768; the LDS query, a separate copy of the routing rule without its byte ranges, answered
    wino3_pair_kernel's 4 * VBUF.  Descriptors only, nothing is allocated.

    The layer as first written down -- N=1, H=W=2048, Cin=ldx=32, Cout=ldy=64 -- is one no kernel of the entry point takes:
    with ldy = 64 two OUTPUT images are 2 * 2048 * 2048 * 64 * 4 = 2^31 bytes, and every form needs them below 2 GiB
    ("tensor too large for 32-bit buffer addressing"; the old query answered 71 KB of LDS for it all the same).  Plan and query
    must both refuse it.  With Cout = ldy = 60 -- cout_pad still 64, two output images 1.875 GiB -- the input-side condition is
    the only one that fails, and both must name wino2_kernel."""
    import ctypes as C
    lib = _lib.load()
    base = dict(N=1, H=2048, W=2048, Cin=32, ldx=32, cout_pad=64, kh=3, kw=3, stride=1, wino_form=0)
    assert 2 * 2048 * 2048 * 32 * 4 == 1 << 30
    nb = C.c_int(-1)
    d = _lib.ConvDesc(Cout=64, ldy=64, **base)
    assert _lib.winograd_launch_plan(d) is None and b'too large' in lib.kfn_last_error()
    assert lib.kfn_winograd_lds_bytes(C.byref(d), C.byref(nb)) < 0 and lib.kfn_winograd_fused_supported(C.byref(d)) == 0
    d = _lib.ConvDesc(Cout=60, ldy=60, **base)
    p = _lib.winograd_launch_plan(d)
    assert p is not None and p.kernel == K.WINO_KERNEL_WINO2_WIDE and p.lds_bytes == 32768 and p.threads == 64
    assert lib.kfn_winograd_lds_bytes(C.byref(d), C.byref(nb)) == 0 and nb.value == 32768
    # one row less and the two-wave form takes it: the boundary is the launcher's
    p = _lib.winograd_launch_plan(_lib.ConvDesc(**dict(base, H=2047, Cout=60, ldy=60)))
    assert p is not None and p.kernel == K.WINO_KERNEL_WINO3_PAIR and p.lds_bytes > 32768
