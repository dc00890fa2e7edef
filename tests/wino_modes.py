"""Case table of the Winograd kernels' mode cross-test (tests/test_gpu_wino_modes.py; checked on the host by
tests/test_wino_modes_host.py).

The minimal-filtering entry points (csrc/kfn_wino2.hip, kfn_wino3.hip, kfn_wino4.hip, kfn_wino_s2.hip, kfn_wino_s2c.hip) are
steered by many descriptor fields at once: the form, the workgroup order, ReLU, bias, channel windows on either side, the
layout, split-K -- and, silently, by Cout % 4, ldy % 4 and the alignment of y, which pick between the 16-byte and the
dword store epilogue.  As in tests/conv_modes.py every field is a FACTOR with a few LEVELS, RULES restate what the
launchers accept (their launch plans: wino_fused_plan, wino_f43_plan, wino_s2_plan, wino_s2c_plan, which state the two split-K
entry points too; nothing else -- tests/test_wino_modes_host.py holds the table against them through kfn_winograd_launch_plan),
and conv_modes.Table draws cases until every pair of
levels that the rules allow together occurs in one.  EXTRA adds what pairs alone do not guarantee (see there).  Nothing
below touches the GPU."""
import collections

import numpy as np

from oracle import kfnet_oracle as O
from tests.conv_modes import Table

# kernel level -> (family, run_winograd kind, wino_form, fp16 operands, split-K entry point, output channels per workgroup)
KERNELS = collections.OrderedDict([
    ('w2', ('f23', 'fused', 1, False, False, 32)),      # wino2_kernel, KFN_WINO_FORM_ONE_WAVE
    ('w3p', ('f23', 'fused', 0, False, False, 64)),     # wino3_pair_kernel: cout_pad == 64
    ('w3', ('f23', 'fused', 0, False, False, 128)),     # wino3_kernel<false>: Cout >= 128, Cin % 32 == 0
    ('w3h', ('f23', 'fused', 0, True, False, 128)),     # wino3_kernel<true>: fp16 operands, Cin % 64 == 0
    ('f43a', ('f43', 'f43', 2, False, False, 64)),      # wino4_kernel
    ('f43b', ('f43', 'f43', 3, False, False, 64)),      # wino4b_kernel
    ('f43bk', ('f43', 'f43', 3, False, True, 64)),      # wino4b_kernel through kfn_conv2d_winograd_f43_splitk
    ('s2a', ('s2', 's2', 0, False, False, 128)),        # wino_s2_kernel<false>
    ('s2ah', ('s2', 's2', 0, True, False, 128)),        # wino_s2_kernel<true>
    ('s2b', ('s2', 's2', 4, False, False, 128)),        # wino_s2b_kernel
    ('s2bk', ('s2', 's2', 4, False, True, 128)),        # wino_s2b_kernel through kfn_conv2d_winograd_s2_splitk
    ('s2c', ('f42', 's2', 5, False, False, 128)),       # wino_s2c_kernel (the table's images never fill the chip twice)
])
FAMILY = {k: v[0] for k, v in KERNELS.items()}
TOL_KIND = {'f23': 'f23', 'f43': 'f43', 's2': 'f22s2', 'f42': 'f42s2'}       # conv_tol.A
STRIDE = {'f23': 1, 'f43': 1, 's2': 2, 'f42': 2}
# tile block of a workgroup in output tiles (rows, columns) and the output pixels of a tile
BLOCK = {'f23': (4, 8, 2), 'f43': (8, 4, 4), 's2': (4, 8, 2), 'f42': (4, 4, 4)}
# the kernels with a dword-store epilogue beside the 16-byte one (wide_store = 0); s2bk with k_split = 1 IS the s2b launch
DWORD_KERNELS = ('w2', 'w3p', 'w3', 'w3h', 's2a', 's2ah', 's2b')
GROUP_KERNELS = ('f43a', 'f43b', 'f43bk', 's2a', 's2ah', 's2b', 's2bk', 's2c')   # decode KFN_WINO_ORDER_GROUPS(n)
FAST_KERNELS = ('w3', 'w3h')                                                     # M fastest / N fastest only (w3p: one group)

# (N, H, W) per family: whole blocks, ragged blocks, a block straddling two images, fewer tile columns than a block holds
IMAGES = {
    'f23': ((1, 8, 8), (2, 7, 9), (3, 14, 33), (5, 10, 6)),
    'f43': ((2, 32, 16), (1, 29, 12), (3, 29, 35), (2, 36, 40)),
    's2': ((1, 16, 16), (2, 14, 18), (3, 30, 34), (5, 20, 24)),
    'f42': ((1, 32, 32), (2, 40, 48), (3, 32, 40), (1, 32, 72)),
}
ORDERS = collections.OrderedDict([('auto', 0), ('m', 1), ('n', 2), ('g2', 18), ('g3', 19), ('g4', 20)])   # KFN_WINO_ORDER_*
LAYOUTS = {'nhwc': ('nhwc', 'nhwc'), 'c16in': ('c16', 'nhwc'), 'c16out': ('nhwc', 'c16'), 'c16both': ('c16', 'c16')}

FACTORS = collections.OrderedDict([
    ('kernel', tuple(KERNELS)),
    ('img', tuple(i for f in ('f23', 'f43', 's2', 'f42') for i in IMAGES[f])),
    ('cin', (16, 32, 48, 64, 128)),                    # one, odd and many super-steps
    ('cout', (6, 8, 36, 50, 64, 100, 128, 130, 160, 256, 384)),
    ('order', tuple(ORDERS)),
    ('relu', (0, 1)),
    ('bias', (1, 0)),
    ('xview', ('dense', 'pad', 'x8')),
    ('yview', ('dense', 'pad', 'ld', 'off')),
    ('layout', tuple(LAYOUTS)),
    ('ksplit', (0, 1, 2, 3)),
])
NAMES = tuple(FACTORS)
Case = collections.namedtuple('Case', NAMES)
SEED = 23


def view_strides(c):
    """(ldx, x_off, ldy, y_off) in floats.  xview pad: 32 bytes before the window; x8: 8 bytes (F(4x4,3x3) only).  yview pad: the
    window starts 16 bytes in (the 16-byte stores run); ld: ldy % 4 == 2; off: the base is 4 bytes past a 16-byte boundary."""
    ldx, x_off = {'dense': (c.cin, 0), 'pad': (c.cin + 16, 8), 'x8': (c.cin + 6, 2)}[c.xview]
    ldy, y_off = {'dense': (c.cout, 0), 'pad': (c.cout + 8, 4), 'ld': (c.cout + 6, 0), 'off': (c.cout + 8, 1)}[c.yview]
    return ldx, x_off, ldy, y_off


def _split_ok(cin, ks):
    n_super = cin // 16
    return ks <= n_super and (ks - 1) * -(-n_super // ks) < n_super          # no empty run of super-steps


def _dword_ok(kernel, ks):
    return kernel in DWORD_KERNELS or (kernel == 's2bk' and ks == 1)


def launch_args(c):
    """The keyword arguments of gpu_util.run_winograd / winograd_fields for case c (everything but the data and the split)."""
    _, _, form, f16, _, _ = KERNELS[c.kernel]
    ldx, x_off, ldy, y_off = view_strides(c)
    xl, yl = LAYOUTS[c.layout]
    return dict(relu=bool(c.relu), form=form, ldx_pad=ldx - c.cin, ldy_pad=ldy - c.cout, x_layout=xl, y_layout=yl,
                order=ORDERS[c.order], x_off=x_off, y_off=y_off, f16=f16)


RULES = (
    (('kernel', 'img'), lambda k, i: i in IMAGES[FAMILY[k]]),
    (('kernel', 'cout'), lambda k, co: (32 < co <= 64) if k == 'w3p' else (co >= 128 if k in ('w3', 'w3h') else True)),
    (('kernel', 'cin'), lambda k, ci: ci % 64 == 0 if k == 'w3h' else (ci % 32 == 0 if k == 'w3' else True)),
    (('kernel', 'xview'), lambda k, v: v != 'x8' or FAMILY[k] == 'f43'),
    (('kernel', 'layout'), lambda k, l: l == 'nhwc' or k in ('f43b', 's2c')),
    (('kernel', 'ksplit'), lambda k, s: (s > 0) == KERNELS[k][4]),
    (('cin', 'ksplit'), lambda ci, s: s == 0 or _split_ok(ci, s)),
    (('kernel', 'ksplit', 'cout'), lambda k, s, co: co % 4 == 0 or _dword_ok(k, s)),
    (('kernel', 'ksplit', 'yview'), lambda k, s, v: v not in ('ld', 'off') or _dword_ok(k, s)),
    (('layout', 'xview'), lambda l, v: LAYOUTS[l][0] == 'nhwc' or v == 'dense'),      # a blocked tensor is dense
    (('layout', 'yview'), lambda l, v: LAYOUTS[l][1] == 'nhwc' or v == 'dense'),
    (('layout', 'cout'), lambda l, co: LAYOUTS[l][1] == 'nhwc' or co % 16 == 0),
)
TABLE = Table(FACTORS, RULES, Case, constrained_first=True)


def store_path(c):
    """'dword' where the launcher clears wide_store (Cout % 4, ldy % 4 or y not 16-byte aligned), else 'wide'."""
    _, _, ldy, y_off = view_strides(c)
    return 'dword' if (c.cout % 4 or ldy % 4 or y_off % 4) else 'wide'


def geometry(c):
    """What the launcher derives from the shape: output size, tiles per image, the grid (tiles_m, tiles_n), whether some
    tile block holds rows of two images, and n_group as the launcher resolves c.order."""
    fam = FAMILY[c.kernel]
    n, h, w = c.img
    s = STRIDE[fam]
    ho, wo = -(-h // s), -(-w // s)
    bh, bw, px = BLOCK[fam]
    th, tw = -(-ho // px), -(-wo // px)
    tiles_m = -(-tw // bw) * -(-(n * th) // bh)
    cout_pad = -(-c.cout // 32) * 32
    tiles_n = -(-cout_pad // KERNELS[c.kernel][5])
    straddle = n > 1 and th % bh != 0
    return dict(ho=ho, wo=wo, th=th, tw=tw, tiles_m=tiles_m, tiles_n=tiles_n, straddle=straddle,
                n_group=n_group(c.kernel, tiles_n, c.order), fallback=falls_back(c.kernel, tiles_n, c.order))


def _requested(kernel, tiles_n, order):
    """The n_group the order asks for, before the launcher checks that it divides tiles_n."""
    fam = FAMILY[kernel]
    if order == 'auto':
        if fam == 'f43':
            return 4 if tiles_n % 4 == 0 else (2 if tiles_n % 2 == 0 else 1)
        return 2 if tiles_n % 2 == 0 else tiles_n          # S2_DEFAULT_N_FAST
    return {'m': 1, 'n': tiles_n}.get(order) or int(order[1:])


def falls_back(kernel, tiles_n, order):
    if kernel not in GROUP_KERNELS:
        return False
    r = _requested(kernel, tiles_n, order)
    return r > tiles_n or tiles_n % r != 0


def n_group(kernel, tiles_n, order):
    """wino_f43_plan / wino_s2_plan / wino_s2c_plan: channel groups of one tile block that are adjacent in the grid.  w3 / w3h
    know M fastest (1) and N fastest (tiles_n) only, every other value being their default, M fastest; w2 and w3p (one
    group) ignore the field: None."""
    if kernel in FAST_KERNELS:
        return tiles_n if order == 'n' else 1
    if kernel not in GROUP_KERNELS:
        return None
    if falls_back(kernel, tiles_n, order):
        return 1 if FAMILY[kernel] == 'f43' else tiles_n
    return _requested(kernel, tiles_n, order)


# What the pairs alone do not guarantee, stated as cases: (a) per kernel that decodes an order, a request that is honoured with
# 1 < n_group < tiles_n and one that falls back, both on tiles_n >= 3 -- triples (kernel, Cout, order); on the 128-channel kernels
# the first needs tiles_n >= 4, i.e. Cout = 512, which is no level (384 gives three groups: GROUPS(2) falls back); (b) every
# dword-store kernel on a block that straddles two images AND on odd output sizes -- triples (kernel, image, store path).
def _extra():
    out = []
    for j, k in enumerate(GROUP_KERNELS + FAST_KERNELS):
        fam = FAMILY[k]
        cin = 64 if KERNELS[k][3] or k == 'w3' else 32
        ks = 2 if KERNELS[k][4] else 0
        picks = {'f43': ((384, 'g3'), (384, 'g4')), 'f23': ((384, 'm'), (384, 'n'))}.get(fam, ((512, 'g2'), (384, 'g2')))
        for t, (co, order) in enumerate(picks):
            out.append(Case(kernel=k, img=IMAGES[fam][1 + t], cin=cin, cout=co, order=order, relu=(j + t) % 2, bias=(j + t + 1) % 2,
                            xview=('pad', 'dense')[t], yview=('pad', 'dense')[(j + t) % 2], layout='nhwc', ksplit=ks))
    straddling = {'f23': ((3, 14, 33), (2, 7, 9)), 's2': ((5, 20, 24), (2, 14, 18))}   # (a block on two images, odd Ho and Wo)
    for j, k in enumerate(DWORD_KERNELS):
        fam = FAMILY[k]
        cin = 64 if k in ('w3', 'w3h', 's2ah') else 48
        co = {'w3p': (50, 36), 'w3': (130, 160), 'w3h': (130, 160)}.get(k, (130, 100))
        for t, img in enumerate(straddling[fam]):
            out.append(Case(kernel=k, img=img, cin=cin, cout=co[t], order=('n', 'm')[(j + t) % 2], relu=(j + t) % 2, bias=t,
                            xview=('dense', 'pad')[t], yview=('dense', 'ld', 'off')[(j + t) % 3] if co[t] % 4 else ('ld', 'off')[j % 2],
                            layout='nhwc', ksplit=0))
    return tuple(out)


EXTRA = _extra()
_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = TABLE.generate(SEED)
    return _TABLE


def cases():
    """(index, case) of everything that is run: the table, then EXTRA from index 1000."""
    return list(enumerate(table())) + [(1000 + j, c) for j, c in enumerate(EXTRA)]


def case_id(i, c):
    return '%03d-%s-%dx%dx%d-ci%d-co%d-%s-r%d-b%d-x%s-y%s-%s-k%d' % (
        (i, c.kernel) + tuple(c.img) + (c.cin, c.cout, c.order, c.relu, c.bias, c.xview, c.yview, c.layout, c.ksplit))


# ---- the persistent F(4,2) kernel: outside the table, its images depend on the device's CU count -------------------------------------
PERSIST_MAX_SS = 64


def s2c_persistent(n, h, w, cin, cout, cu):
    """wino_s2c_plan's rule for wino_s2c_pkernel: 2 <= Cin/16 <= 64 and at least two workgroups per CU."""
    tiles_m = -(-(w // 8) // 4) * -(-(n * (h // 8)) // 4)
    tiles_n = -(-(-(-cout // 32) * 32) // 128)
    return 2 <= cin // 16 <= PERSIST_MAX_SS and tiles_m * tiles_n >= 2 * cu


def persistent_cases(cu):
    """Six (index, case) on images (N, 40, 48), N the smallest batch for which Cout = 512 runs the persistent kernel and N + 3
    (a ragged last round); Cout = 384 gets the smallest N of its own.  Every order level once; ReLU, bias, layouts spread."""
    def n_min(cout):
        n = 1
        while not s2c_persistent(n, 40, 48, 32, cout, cu):
            n += 1
        return n
    spec = (('auto', 64, 512, 0, 1, 1, 'nhwc', 'dense', 'pad'), ('m', 32, 384, 3, 0, 1, 'c16in', 'dense', 'pad'),
            ('n', 32, 512, 3, 1, 0, 'c16out', 'pad', 'dense'), ('g2', 32, 512, 0, 0, 0, 'c16both', 'dense', 'dense'),
            ('g3', 32, 384, 0, 1, 0, 'nhwc', 'pad', 'dense'), ('g4', 64, 512, 3, 0, 1, 'nhwc', 'dense', 'pad'))
    out = []
    for j, (order, cin, cout, dn, relu, bias, layout, xv, yv) in enumerate(spec):
        out.append((2000 + j, Case(kernel='s2c', img=(n_min(cout) + dn, 40, 48), cin=cin, cout=cout, order=order, relu=relu,
                                   bias=bias, xview=xv, yview=yv, layout=layout, ksplit=0)))
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
X_GRID, X_MAX, W_MAX = 2.0 ** -10, 4.0, 0.1875


def make_inputs(i, c):
    """x [N,H,W,Cin], w [3,3,Cin,Cout], b or None -- fp32, seeded from the case's index.  x ~ N(0,1) (post-ReLU for every second
    case), w ~ N(0,1) sqrt(2 / (9 Cin)), b ~ N(0,1).  fp16-operand kernels: x and w on the 2^-10 grid, |x| <= 4, |w| <= 0.1875 --
    the packed U is then exact in fp16, B^T d B is exact in fp32 (test_wino_modes_host.py checks both), so the kernel and
    wino_reference() multiply identical operands."""
    n, h, wd = c.img
    rng = np.random.default_rng([SEED, i])
    x = rng.normal(size=(n, h, wd, c.cin))
    if i % 2:
        x = np.maximum(x, 0.0)
    w = rng.normal(size=(3, 3, c.cin, c.cout)) * np.sqrt(2.0 / (9 * c.cin))
    b = rng.normal(size=c.cout) if c.bias else None
    if KERNELS[c.kernel][3]:
        x = np.clip(np.round(x / X_GRID) * X_GRID, -X_MAX, X_MAX)
        w = np.clip(np.round(w / X_GRID) * X_GRID, -W_MAX, W_MAX)
    f = np.float32
    return x.astype(f), w.astype(f), (b.astype(f) if b is not None else None)


# ---- references ---------------------------------------------------------------------------------------------------------------------
# F(2x2,3x3)
BT23 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
G23 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
AT23 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)
# F(2,2) as kfn_wino_s2.hip runs it: index 2 of V is d1 - d2, its output coefficient -1 is folded into the weights
BT22 = np.array([[1, -1, 0], [0, 1, 0], [0, 1, -1]], np.float64)
G22 = np.array([[1, 0], [1, 1], [0, -1]], np.float64)
AT22 = np.array([[1, 1, 0], [0, 1, 1]], np.float64)


def transformed_weights(fam, w):
    """The transformed kernel in fp64, unrounded.  'f23': U [4,4,Cin,Cout].  's2': (U00 [3,3,Cin,Cout], U01 [3,Cin,Cout],
    U10 [3,Cin,Cout], U11 [Cin,Cout]) of the four polyphase filters."""
    w = np.asarray(w, np.float64)
    if fam == 'f23':
        return np.einsum('ai,ijco,bj->abco', G23, w, G23)
    assert fam == 's2'
    return (np.einsum('xa,abio,nb->xnio', G22, w[0::2, 0::2], G22), np.einsum('xa,aio->xio', G22, w[0::2, 1]),
            np.einsum('nb,bio->nio', G22, w[1, 0::2]), w[1, 1])


def unpack_u(fam, packed, cin, cout):
    """pack_winograd_fused_kernel / pack_winograd_s2_kernel's [Cin/8][16][cout_pad][8] (any dtype) back to the shapes of
    transformed_weights(), in fp64."""
    u = np.asarray(packed).astype(np.float64).transpose(1, 2, 0, 3).reshape(16, -1, cin)[:, :cout, :].transpose(0, 2, 1)   # [16][Cin][Cout]
    if fam == 'f23':
        return u.reshape(4, 4, cin, cout)
    return u[0:9].reshape(3, 3, cin, cout), u[9:12], u[12:15], u[15]


def input_transform(fam, x):
    """V in fp64: 'f23' [N,Th,Tw,4,4,Cin]; 's2' the four parts (V00 [N,Th,Tw,3,3,Cin], V01 [..,3 xi,2 n,Cin], V10 [..,2 m,3 nu,Cin],
    V11 [..,2,2,Cin])."""
    x = np.asarray(x, np.float64)
    n, h, w, ci = x.shape
    if fam == 'f23':
        th, tw = (h + 1) // 2, (w + 1) // 2
        xp = np.zeros((n, 2 * th + 2, 2 * tw + 2, ci))
        xp[:, 1:1 + h, 1:1 + w] = x
        d = np.stack([np.stack([xp[:, r:r + 2 * th:2, c:c + 2 * tw:2] for c in range(4)], axis=3) for r in range(4)], axis=3)
        return np.einsum('ar,ntxrcC,bc->ntxabC', BT23, d, BT23)
    assert fam == 's2' and h % 2 == 0 and w % 2 == 0
    ho, wo = h // 2, w // 2
    th, tw = (ho + 1) // 2, (wo + 1) // 2
    xp = np.zeros((n, 4 * th + 4, 4 * tw + 4, ci))
    xp[:, :h, :w] = x
    ph = [[xp[:, p::2, q::2] for q in range(2)] for p in range(2)]          # x_pq[i][j] = x[2i + p][2j + q]

    def patch(a, rows, cols):
        return np.stack([np.stack([a[:, r:r + 2 * th:2, c:c + 2 * tw:2] for c in range(cols)], axis=3) for r in range(rows)], axis=3)
    return (np.einsum('ar,ntxrcC,bc->ntxabC', BT22, patch(ph[0][0], 3, 3), BT22),
            np.einsum('ar,ntxrcC->ntxacC', BT22, patch(ph[0][1], 3, 2)),
            np.einsum('bc,ntxrcC->ntxrbC', BT22, patch(ph[1][0], 2, 3)), patch(ph[1][1], 2, 2))


def wino_reference(fam, x, u, b, relu, out_hw, round_v=None):
    """The convolution the Winograd way in fp64: V = B^T d B (through `round_v` when given), times `u` (transformed_weights() or
    unpack_u()), summed over the input channels, A^T M A, bias, ReLU.  out_hw: (Ho, Wo)."""
    v = input_transform(fam, x)
    rnd = round_v or (lambda a: a)
    if fam == 'f23':
        m = np.einsum('ntxabC,abCo->ntxabo', rnd(v), u)
        y = np.einsum('ia,ntxabo,jb->ntixjo', AT23, m, AT23)
    else:
        v00, v01, v10, v11 = [rnd(a) for a in v]
        u00, u01, u10, u11 = u
        y = (np.einsum('ia,ntxabo,jb->ntixjo', AT22, np.einsum('ntxabC,abCo->ntxabo', v00, u00), AT22) +
             np.einsum('ia,ntxajo->ntixjo', AT22, np.einsum('ntxajC,aCo->ntxajo', v01, u01)) +
             np.einsum('jb,ntxibo->ntixjo', AT22, np.einsum('ntxibC,bCo->ntxibo', v10, u10)) +
             np.einsum('ntxijC,Co->ntixjo', v11, u11))
    n, th, _, tw, _, co = y.shape
    y = y.reshape(n, 2 * th, 2 * tw, co)[:, :out_hw[0], :out_hw[1]]
    if b is not None:
        y = y + np.asarray(b, np.float64)
    return np.maximum(y, 0.0) if relu else y


def round_f16(a):
    return a.astype(np.float16).astype(np.float64)


def packed_f16(c, w):
    """The fp16 U the device gets for an fp16-operand case, decoded to transformed_weights()' shapes."""
    from kfnet_amd.graph import as_f16, pack_winograd_fused_kernel, pack_winograd_s2_kernel
    fam = FAMILY[c.kernel]
    pack = pack_winograd_fused_kernel if fam == 'f23' else pack_winograd_s2_kernel
    return unpack_u(fam, as_f16(pack)(w), c.cin, c.cout)


def reference(c, x, w, b):
    """fp64 reference of a case: oracle.conv2d_same with bias and ReLU; for the fp16-operand kernels the Winograd way with V
    rounded to fp16 once (RNE) and the fp16 U the device gets."""
    fam = FAMILY[c.kernel]
    if KERNELS[c.kernel][3]:
        g = geometry(c)
        return wino_reference(fam, x, packed_f16(c, w), b, bool(c.relu), (g['ho'], g['wo']), round_f16)
    b64 = b.astype(np.float64) if b is not None else None
    return O.conv2d_same(x.astype(np.float64), w.astype(np.float64), b64, STRIDE[fam], bool(c.relu))
