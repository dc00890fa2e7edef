"""Case table of the direct convolution's mode cross-test (tests/test_gpu_conv_modes.py; checked on the host by
tests/test_conv_modes_host.py).

kfn_conv2d_nhwc (csrc/kfn_conv.hip, conv_mfma_kernel) is steered by many descriptor fields at once; the op tests exercise
each of them mostly alone.  Here every field is a FACTOR with a few LEVELS, RULES restate what the launcher accepts (its
validate(), its dispatch and pick_config(); nothing else), and a seeded greedy generator draws cases until every pair of
levels that the rules allow together occurs in at least one case.  The generator itself (class Table) knows nothing of this
table: tests/wino_modes.py hands it another.  Nothing below touches the GPU."""
import collections

import numpy as np

from oracle import kfnet_oracle as O

EPI_NONE, EPI_L2NORM, EPI_EXP_CH3, EPI_EXP_1E2 = 0, 1, 2, 3      # KFN_EPI_*
EPI_NAME = {EPI_NONE: 'none', EPI_L2NORM: 'l2norm', EPI_EXP_CH3: 'exp_ch3', EPI_EXP_1E2: 'exp_1e2'}
EPI_COUT = {EPI_L2NORM: 32, EPI_EXP_CH3: 4, EPI_EXP_1E2: 1}       # channels of the three heads
EPI_CONFIGS = (0, 4, 6)            # auto, 128x32, 256x32: pick_config() forces every other choice to 128x32
X16_CONFIGS = (0, 2, 3, 4, 6)      # auto + the four fp16-input / fp32-output instantiations
N16_CONFIGS = (10, 11)             # the 16-column tiles: fp32 operands only

# image sets (N, H, W).  256 rows = a whole number of every tile height except 160 and 192; 442 rows = a ragged last tile
# for every height.  Transposed: M = 4 N H W rows in parity-class order -- (2,5,7) puts the class boundaries at rows 70,
# 140, 210 (inside 128-, 160- and 256-row tiles), (2,13,17) at 442, 884, 1326.
IMAGES = ((7, 1, 1), (6, 2, 2), (2, 5, 7), (1, 16, 16), (2, 13, 17))
IMAGES_S2_EVEN = ((2, 6, 8), (1, 16, 16), (2, 14, 18))
IMAGES_FOR = {
    's1': IMAGES, '1x1': IMAGES, 'tr': IMAGES,
    's2e': IMAGES_S2_EVEN,                                              # even H, W: SAME pad (0, 1)
    's2o': tuple(i for i in IMAGES if i[1] % 2 == 1 and i[2] % 2 == 1),  # odd H, W: SAME pad (1, 1)
}
MODE = {  # kernel size, stride, transposed
    's1': (3, 1, False), 's2e': (3, 2, False), 's2o': (3, 2, False), '1x1': (1, 1, False), 'tr': (3, 2, True)}

FACTORS = collections.OrderedDict([
    ('mode', ('s1', 's2e', 's2o', '1x1', 'tr')),
    ('img', IMAGES + tuple(i for i in IMAGES_S2_EVEN if i not in IMAGES)),
    ('cin', (16, 48, 64, 128)),
    ('cout', (1, 4, 16, 20, 32, 33, 64, 100, 160)),
    ('config', tuple(range(12))),                    # KFN_CFG_AUTO and the eleven fp32 tile configs
    ('operands', ('f32', 'f16', 'f16x3')),
    ('relu', (0, 1)),
    ('bias', (1, 0)),
    ('view', ('dense', 'in', 'out', 'both')),
    ('epi', (EPI_NONE, EPI_L2NORM, EPI_EXP_CH3, EPI_EXP_1E2)),
    ('x16', (0, 1)),                                 # fp16 input tensor, fp32 output
])
NAMES = tuple(FACTORS)
Case = collections.namedtuple('Case', NAMES)

SEED = 15
CANDIDATES = 48        # completions drawn per step; the one covering most uncovered pairs is kept


def view_strides(cin, cout, view):
    """(ldx, x_off, ldy, y_off) of a view level."""
    win, wout = view in ('in', 'both'), view in ('out', 'both')
    return (cin + 32 if win else cin, 16 if win else 0, cout + 24 if wout else cout, 8 if wout else 0)


# What the launcher accepts, one rule per line: (fields it reads, predicate).  A rule is applied as soon as all its fields
# are known, so the same list prunes the searches below and judges whole cases.
RULES = (
    (('mode', 'img'), lambda m, i: i in IMAGES_FOR[m]),
    (('operands', 'cin'), lambda o, c: o == 'f32' or c % 32 == 0),           # fp16 MFMA: 32 channels per k-step
    (('operands', 'mode'), lambda o, m: o != 'f16x3' or m != 'tr'),          # f16x3: forward only
    (('operands', 'config'), lambda o, c: o == 'f32' or c not in N16_CONFIGS),
    (('x16', 'mode'), lambda x, m: not x or m != 'tr'),                      # fp16 activations: forward only
    (('x16', 'operands'), lambda x, o: not x or o == 'f16'),
    (('x16', 'config'), lambda x, c: not x or c in X16_CONFIGS),
    (('x16', 'cin', 'view'), lambda x, c, v: not x or view_strides(c, 0, v)[0] % 8 == 0),
    (('epi', 'mode'), lambda e, m: e == EPI_NONE or m != 'tr'),              # head epilogues: forward only
    (('epi', 'cout'), lambda e, c: e == EPI_NONE or c == EPI_COUT[e]),
    (('epi', 'config'), lambda e, c: e == EPI_NONE or c in EPI_CONFIGS),
)


class Table:
    """The generator, for any table of factors and rules (tests/wino_modes.py builds its own from it): FACTORS an ordered
    dict factor -> levels, RULES a list of (fields, predicate) as above."""

    def __init__(self, factors, rules, case_type=None, constrained_first=False):
        self.factors = factors
        self.constrained_first = constrained_first      # complete() sets the factors that most rules name first (less backtracking)
        self.rules = tuple(rules)
        self.names = tuple(factors)
        self.Case = case_type or collections.namedtuple('Case', self.names)
        # the rules that name a factor: when that factor is the last one set, only these can newly fail
        self._naming = {n: tuple(r for r in self.rules if n in r[0]) for n in self.names}

    def valid(self, partial):
        """`partial`: dict factor -> level (any subset).  False as soon as a rule whose fields are all present fails."""
        for fields, pred in self.rules:
            if all(f in partial for f in fields) and not pred(*[partial[f] for f in fields]):
                return False
        return True

    def _still_valid(self, cur, name):
        """valid(cur) for a `cur` that was valid before `name` was set."""
        for fields, pred in self._naming[name]:
            try:
                args = [cur[f] for f in fields]
            except KeyError:
                continue
            if not pred(*args):
                return False
        return True

    def complete(self, partial, rng=None, constrained_first=None):
        """A valid full case extending `partial` (levels in random order when `rng` is given), or None if there is none."""
        todo = [n for n in self.names if n not in partial]
        if rng is not None:
            todo = [todo[i] for i in rng.permutation(len(todo))]
        if self.constrained_first if constrained_first is None else constrained_first:
            todo.sort(key=lambda n: -len(self._naming[n]))      # stable: the drawn order among equals

        def rec(k, cur):
            if k == len(todo):
                return dict(cur)
            levels = self.factors[todo[k]]
            order = rng.permutation(len(levels)) if rng is not None else range(len(levels))
            for j in order:
                cur[todo[k]] = levels[j]
                if self._still_valid(cur, todo[k]):
                    got = rec(k + 1, cur)
                    if got is not None:
                        return got
                del cur[todo[k]]
            return None

        if not self.valid(partial):
            return None
        return rec(0, dict(partial))

    def all_pairs(self):
        """Every ((factor, level), (factor, level)) of two different factors, factors in table order."""
        names = self.names
        out = []
        for a in range(len(names)):
            for b in range(a + 1, len(names)):
                for la in self.factors[names[a]]:
                    for lb in self.factors[names[b]]:
                        out.append(((names[a], la), (names[b], lb)))
        return out

    def allowed_pairs(self):
        """The pairs that some valid case contains (exhaustive search per pair, pruned by the rules; whether a completion
        exists does not depend on the order in which the search sets the factors)."""
        return [p for p in self.all_pairs() if self.complete({p[0][0]: p[0][1], p[1][0]: p[1][1]}, None, True) is not None]

    def pairs_of(self, case):
        names = self.names
        d = case._asdict() if hasattr(case, '_asdict') else case
        return {((names[a], d[names[a]]), (names[b], d[names[b]]))
                for a in range(len(names)) for b in range(a + 1, len(names))}

    def generate(self, seed):
        """Seeded greedy all-pairs table: while a pair is uncovered, draw random valid completions of it and keep the one
        that covers the most pairs still uncovered."""
        rng = np.random.default_rng(seed)
        open_pairs = self.allowed_pairs()
        uncovered = set(open_pairs)
        cases = []
        for p in open_pairs:
            if p not in uncovered:
                continue
            best, gain = None, 0
            for _ in range(CANDIDATES):
                c = self.complete({p[0][0]: p[0][1], p[1][0]: p[1][1]}, rng)
                g = len(self.pairs_of(c) & uncovered)
                if g > gain:
                    best, gain = c, g
            cases.append(self.Case(**best))
            uncovered -= self.pairs_of(best)
        assert not uncovered
        return cases


DIRECT = Table(FACTORS, RULES, Case)
valid, complete, all_pairs, allowed_pairs, pairs_of = (DIRECT.valid, DIRECT.complete, DIRECT.all_pairs, DIRECT.allowed_pairs,
                                                       DIRECT.pairs_of)


def generate(seed=SEED):
    return DIRECT.generate(seed)


# Outside the table: an explicit config that pick_config() forces to 128x32 beside a head epilogue -- (index, the config-4
# case, the other config); the two results must agree bit for bit.
FORCED = tuple((1000 + 2 * e, Case(mode='s1', img=(2, 13, 17), cin=48, cout=EPI_COUT[e], config=4, operands='f32', relu=1,
                                   bias=1, view='both', epi=e, x16=0), cfg)
               for e, cfg in ((EPI_L2NORM, 2), (EPI_EXP_CH3, 7), (EPI_EXP_1E2, 10)))

_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = generate()
    return _TABLE


def cases():
    """(index, case) of everything that is run: the table, then FORCED's config-4 cases."""
    return list(enumerate(table())) + [(i, c) for i, c, _ in FORCED]


def case_id(i, c):
    return '%03d-%s-%dx%dx%d-ci%d-co%d-cfg%d-%s%s-r%d-b%d-%s-%s' % (
        (i, c.mode) + tuple(c.img) + (c.cin, c.cout, c.config, c.operands, '-x16' if c.x16 else '', c.relu, c.bias, c.view,
                                      EPI_NAME[c.epi]))


def zero_pixel(c):
    """L2NORM cases: (image, output row, output column) of the pixel whose receptive field is zeroed, or None where no
    all-zero output can be made (a bias without ReLU: the pixel's outputs are then the bias itself)."""
    if c.epi != EPI_L2NORM or (c.bias and not c.relu):
        return None
    k, s, _ = MODE[c.mode]
    n, h, w = c.img
    return (n - 1, -(-h // s) // 2, -(-w // s) // 2)


def zero_mask(c, x):
    """[N,Ho,Wo] bool: the output pixels of an L2NORM case that are zero by construction -- zero_pixel() and, on images
    smaller than the zeroed neighbourhood, whichever other pixels see nothing but zeros.  All False without zero_pixel()."""
    k, s, _ = MODE[c.mode]
    seen = O.conv2d_same(np.abs(x.astype(np.float64)), np.ones((k, k, c.cin, 1)), None, s, False)[..., 0]
    if zero_pixel(c) is None:
        return np.zeros(seen.shape, dtype=bool)
    assert seen[zero_pixel(c)] == 0.0
    return seen == 0.0


def make_inputs(i, c):
    """x [N,H,W,Cin], w (TF layout; [k,k,Cout,Cin] when transposed), b or None -- fp32, seeded from the case's index.
    x ~ N(0,1) (post-ReLU for every second case), w ~ N(0,1)/sqrt(K), b ~ N(0,1).  L2NORM cases with a zero_pixel(): the
    3x3 neighbourhood (the receptive field) of that pixel is zero and b = -|b| / 16 <= 0, so that with ReLU (or without
    bias) its 32 outputs are all zero before the normalisation.  (The 1/16: with b = -|N(0,1)| ReLU would silence three
    quarters of the channels of EVERY pixel and leave norms far below 1 all over the map -- the L2NORM allowance is
    stated for ||v|| >= 1 -- while -|b| / 16 keeps about half of the channels alive, as without a bias.)"""
    k, s, tr = MODE[c.mode]
    n, h, wd = c.img
    rng = np.random.default_rng([SEED, i])
    x = rng.normal(size=(n, h, wd, c.cin))
    if i % 2:
        x = np.maximum(x, 0.0)
    K = k * k * c.cin
    w = rng.normal(size=(k, k, c.cout, c.cin) if tr else (k, k, c.cin, c.cout)) / np.sqrt(K)
    b = rng.normal(size=c.cout) if c.bias else None
    zp = zero_pixel(c)
    if zp is not None:
        _, pt, _ = O.same_pad(h, k, s)
        _, pl, _ = O.same_pad(wd, k, s)
        r0, c0 = zp[1] * s - pt, zp[2] * s - pl
        x[zp[0], max(r0, 0):max(r0 + k, 0), max(c0, 0):max(c0 + k, 0), :] = 0.0
        if b is not None:
            b = -np.abs(b) / 16.0
    f = np.float32
    return x.astype(f), w.astype(f), (b.astype(f) if b is not None else None)


def rounded_operands(c, x, w):
    """The operands the kernel's products are exact for, in fp64: fp16-rounded for fp16 operands (and an fp16 input
    tensor), unrounded for fp32 and for f16x3 (whose hi + lo split carries 22 significand bits)."""
    if c.operands == 'f16':
        return x.astype(np.float16).astype(np.float64), w.astype(np.float16).astype(np.float64)
    return x.astype(np.float64), w.astype(np.float64)


def reference(c, x, w, b):
    """fp64 convolution (bias, ReLU) WITHOUT the head epilogue, on rounded_operands()."""
    k, s, tr = MODE[c.mode]
    xr, wr = rounded_operands(c, x, w)
    b64 = b.astype(np.float64) if b is not None else None
    return (O.conv2d_transpose_same if tr else O.conv2d_same)(xr, wr, b64, s, bool(c.relu))


def apply_epilogue(epi, v):
    """The head operation on the fp64 pre-epilogue values."""
    if epi == EPI_L2NORM:
        return O.l2_normalize(v)
    if epi == EPI_EXP_CH3:
        out = v.copy()
        out[..., 3] = np.exp(v[..., 3])
        return out
    if epi == EPI_EXP_1E2:
        return np.exp(v) * 1e-2
    return v
