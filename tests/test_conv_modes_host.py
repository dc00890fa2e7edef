"""Host checks of the direct convolution's case table (tests/conv_modes.py): pair coverage, reproducibility, and the
premise of the L2NORM tolerance (no accidental near-zero pixel in the fp64 reference)."""
import numpy as np

from tests import conv_modes as CM


def test_rules_allow_and_refuse_what_the_launcher_does():
    ok = {p for p in CM.allowed_pairs()}
    def pair(fa, la, fb, lb):
        a, b = sorted([(fa, la), (fb, lb)], key=lambda t: CM.NAMES.index(t[0]))
        return (a, b)
    # spot checks against kfn_conv.hip: validate(), dispatch_cfg(), pick_config(), the fp16-input switch
    assert pair('mode', 'tr', 'operands', 'f16') in ok and pair('mode', 'tr', 'config', 10) in ok
    assert pair('mode', 'tr', 'operands', 'f16x3') not in ok and pair('mode', 'tr', 'x16', 1) not in ok
    assert pair('mode', 'tr', 'epi', CM.EPI_L2NORM) not in ok
    assert pair('cin', 48, 'operands', 'f16') not in ok and pair('cin', 16, 'x16', 1) not in ok   # the second only through f16
    assert pair('cout', 33, 'epi', CM.EPI_L2NORM) not in ok and pair('cout', 32, 'epi', CM.EPI_L2NORM) in ok
    assert pair('config', 6, 'epi', CM.EPI_EXP_1E2) in ok and pair('config', 2, 'epi', CM.EPI_EXP_1E2) not in ok
    assert pair('config', 11, 'operands', 'f16x3') not in ok and pair('config', 5, 'operands', 'f16x3') in ok
    assert pair('config', 7, 'x16', 1) not in ok and pair('epi', CM.EPI_EXP_CH3, 'x16', 1) in ok
    assert pair('mode', 's2e', 'img', (7, 1, 1)) not in ok and pair('mode', 's2o', 'img', (2, 13, 17)) in ok
    # every level of every factor is usable at all
    used = {q for p in ok for q in p}
    assert used == {(n, l) for n in CM.NAMES for l in CM.FACTORS[n]}


def test_table_covers_every_allowed_pair():
    cases = CM.table()
    assert all(CM.valid(c._asdict()) for c in cases)
    covered = set()
    for c in cases:
        covered |= CM.pairs_of(c)
    missing = [p for p in CM.allowed_pairs() if p not in covered]
    assert not missing, missing[:10]
    # the largest pair of factors (config x cout) alone needs 108 cases
    print('%d cases, %d pairs' % (len(cases), len(covered)))
    assert 108 <= len(cases) <= 200
    # at most 1768 output rows each
    for c in cases:
        k, s, tr = CM.MODE[c.mode]
        n, h, w = c.img
        assert (4 * n * h * w if tr else n * -(-h // s) * -(-w // s)) <= 1768


def test_table_is_reproducible():
    assert CM.generate() == CM.table()


def test_l2norm_references_have_no_accidental_small_norm():
    """The L2NORM allowance divides the convolution's error by ||v||: every pixel except the deliberate zero one must have
    ||v||_2 >= 1 in the fp64 reference (a violation is cured by another SEED, never by another threshold)."""
    seen = 0
    smallest = np.inf
    for i, c in CM.cases():
        if c.epi != CM.EPI_L2NORM:
            continue
        seen += 1
        x, w, b = CM.make_inputs(i, c)
        v = CM.reference(c, x, w, b)
        nrm = np.sqrt((v * v).sum(axis=-1))
        zm = CM.zero_mask(c, x)
        assert zm.any() == (CM.zero_pixel(c) is not None)
        assert np.all(nrm[zm] == 0.0), (i, c)
        nrm[zm] = np.inf
        assert nrm.min() >= 1.0, (i, c, float(nrm.min()))
        smallest = min(smallest, float(nrm.min()))
    print('%d L2NORM cases, smallest norm %.3f' % (seen, smallest))
    assert seen >= 4
    # the floor is executed: some L2NORM case has its zero pixel, with and without a bias
    zs = [c for c in CM.table() if CM.zero_pixel(c) is not None]
    assert any(c.bias for c in zs) and any(not c.bias for c in zs)
