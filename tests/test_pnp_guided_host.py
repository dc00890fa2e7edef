"""CPU tests of guided sampling (no GPU): the C surface of kfn_pnp_ransac_guided with its refusals, the host classes' and
command lines' flag checks, the sampling rule of tests/pnp_guided_ref.py against hand-computed values, its identity with
the uniform draw on equal confidences, the exhaustion of the 16-draw limit, and what the feature is for: on frames with
70 % outliers whose confidence is informative, the guided reference solves more frames than pnp_ref.ransac."""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pnp_guided_ref as G
import pnp_ref as P
from kfnet_amd import _lib, modes
from kfnet_amd.KFNet import pnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (G.CONFIDENCE, G.CONFIDENCE_SQ)
NAMES = ('kfn_pnp_guided_scratch_bytes', 'kfn_pnp_ransac_guided', 'kfn_pnp_hypotheses_guided')


# ---- exports and refusals -----------------------------------------------------------------------------------------------

def test_exports_descriptor_and_documents():
    hdr = open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()
    body = re.search(r'typedef struct kfn_pnp_sample_desc \{(.*?)\} kfn_pnp_sample_desc;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    ctype = {'int32_t': C.c_int32, 'float': C.c_float}
    fields = []
    for stmt in body.split(';'):
        if stmt.strip():
            typ, names = stmt.strip().split(None, 1)
            fields += [(n.strip(), ctype[typ]) for n in names.split(',')]
    assert fields == list(_lib.PnPSampleDesc._fields_)
    assert _lib.PnPSampleDesc().struct_size == C.sizeof(_lib.PnPSampleDesc) == 4 * len(fields) == 12
    assert '#define KFN_PNP_SAMPLE_CONFIDENCE 1' in hdr and '#define KFN_PNP_SAMPLE_CONFIDENCE_SQ 2' in hdr
    assert (_lib.PNP_SAMPLE_CONFIDENCE, _lib.PNP_SAMPLE_CONFIDENCE_SQ) == (1, 2) == MODES
    assert ('#define KFN_PNP_SAMPLE_DESC_INIT {(int32_t)sizeof(kfn_pnp_sample_desc), KFN_PNP_SAMPLE_CONFIDENCE, 1000.0f}'
            in hdr)
    s = pnp.PnPSolver(4, 4, sampling='confidence2').sample_desc()
    assert (s.struct_size, s.mode, s.confidence_cap) == (12, 2, 1000.0)
    assert pnp.PnPSolver(4, 4).sample_desc() is None
    lib = _lib.load()
    assert lib.kfn_abi_version() == 13 == _lib.ABI_VERSION and '#define KFN_ABI_VERSION 13' in hdr
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NAMES:
        assert re.search(r'\bint %s\(' % name, hdr) and name in _lib.SYMBOLS and hasattr(lib, name) and name in doc, name
    assert 'sampling=' in doc


def _desc(**kw):
    d = pnp.PnPSolver(9, 13, hypotheses=64).desc(3, t0=5, ld=4)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _sample(**kw):
    s = _lib.PnPSampleDesc(mode=1, confidence_cap=1000.0)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _align256(x):
    return (x + 255) & ~255


def test_scratch_query():
    lib = _lib.load()
    n, m = C.c_size_t(7), C.c_size_t(7)
    d = _desc()
    assert lib.kfn_pnp_scratch_bytes(C.byref(d), C.byref(m)) == 0
    assert lib.kfn_pnp_guided_scratch_bytes(C.byref(d), C.byref(_sample()), C.byref(n)) == 0
    assert m.value == _align256(3 * 64 * 48) + _align256(3 * 64 * 4)
    assert n.value == m.value + _align256(3 * 9 * 13 * 8) + _align256(3 * 4)          # today's scratch plus the CDF and n
    assert lib.kfn_pnp_guided_scratch_bytes(C.byref(d), C.byref(_sample()), None) == -1
    assert lib.kfn_pnp_guided_scratch_bytes(C.byref(d), None, C.byref(n)) == -1
    assert lib.kfn_pnp_guided_scratch_bytes(None, C.byref(_sample()), C.byref(n)) == -1
    assert lib.kfn_pnp_guided_scratch_bytes(C.byref(d), C.byref(_sample(mode=0)), C.byref(n)) == -1


def test_entry_points_validate_arguments_without_a_gpu():
    lib = _lib.load()
    dummy = C.c_void_p(16)          # never dereferenced: every call below fails its checks first
    unc_ok = _lib.PnPUncDesc(weighted=1, pixel_sigma=1.0)

    def ransac(d=None, s=None, unc=None, null=(), args=None):
        a = list(args) if args is not None else [dummy, dummy, None, None, dummy, dummy]  # records poses cov quality info scratch
        if unc is not None and args is None:
            a[2] = a[3] = dummy
        for i in null:
            a[i] = None
        return lib.kfn_pnp_ransac_guided(C.byref(d or _desc()), C.byref(s) if s is not False else None,
                                         C.byref(unc) if unc is not None else None, *a, None)

    def probe(d=None, s=None, null=(), args=None):
        a = list(args) if args is not None else [dummy] * 7      # records samples hyp_poses counts cum n scratch
        for i in null:
            a[i] = None
        return lib.kfn_pnp_hypotheses_guided(C.byref(d or _desc()), C.byref(s) if s is not False else None, *a, None)

    inf, nan = float('inf'), float('nan')
    for call in (ransac, probe):
        assert call(s=False) == -1 and b'null kfn_pnp_sample_desc' in lib.kfn_last_error()
        for size in (0, 8, 14):
            assert call(s=_sample(struct_size=size)) == -1 and b'struct_size' in lib.kfn_last_error(), size
        for mode in (0, 3, -1):
            assert call(s=_sample(mode=mode)) == -1 and b'mode' in lib.kfn_last_error(), mode
        for cap in (inf, nan, -inf):
            assert call(s=_sample(confidence_cap=cap)) == -1 and b'not finite' in lib.kfn_last_error(), cap
        for cap in (20.0, 19.0, 0.0):
            assert call(s=_sample(confidence_cap=cap)) == -1 and b'<= min_confidence' in lib.kfn_last_error(), cap
        assert call(s=_sample(confidence_cap=4096.5)) == -1 and b'> 4096' in lib.kfn_last_error()
        assert call(d=_desc(min_confidence=-1.0), s=_sample()) == -1 and b'min_confidence' in lib.kfn_last_error()
        assert call(d=_desc(struct_size=8), s=_sample()) == -1 and b'kfn_pnp_desc.struct_size' in lib.kfn_last_error()
        assert call(d=_desc(hypotheses=0), s=_sample()) == -1
        # the cap's largest value and both modes pass the descriptor checks: the next refusal is the null argument
        assert call(s=_sample(mode=2, confidence_cap=4096.0), null=(0,)) == -1 and b'null argument' in lib.kfn_last_error()
    for null in (0, 1, 4, 5):
        assert ransac(s=_sample(), null=(null,)) == -1 and b'null argument' in lib.kfn_last_error(), null
    for null in (0, 1, 2, 3, 6):
        assert probe(s=_sample(), null=(null,)) == -1 and b'null argument' in lib.kfn_last_error(), null
    # without a kfn_pnp_unc_desc there is no covariance to write
    for k in (2, 3):
        a = [dummy, dummy, None, None, dummy, dummy]
        a[k] = dummy
        assert ransac(s=_sample(), args=a) == -1 and b'need a kfn_pnp_unc_desc' in lib.kfn_last_error(), k
    # kfn_pnp_ransac_unc's rules with one
    assert ransac(s=_sample(), unc=_lib.PnPUncDesc(weighted=2, pixel_sigma=1.0)) == -1 and b'weighted' in lib.kfn_last_error()
    assert ransac(s=_sample(), unc=_lib.PnPUncDesc(weighted=1, pixel_sigma=0.0)) == -1 and b'pixel_sigma' in lib.kfn_last_error()
    assert ransac(s=_sample(), unc=_lib.PnPUncDesc(struct_size=8, weighted=1, pixel_sigma=1.0)) == -1
    assert ransac(s=_sample(), unc=unc_ok, null=(0,)) == -1 and b'null argument' in lib.kfn_last_error()
    odd = C.c_void_p(20)
    assert ransac(s=_sample(), args=[dummy, dummy, None, None, dummy, odd]) == -1 and b'aligned' in lib.kfn_last_error()
    assert probe(s=_sample(), args=[dummy] * 6 + [odd]) == -1 and b'aligned' in lib.kfn_last_error()
    assert probe(s=_sample(), args=[dummy] * 4 + [odd, dummy, dummy]) == -1 and b'cum' in lib.kfn_last_error()


def test_solver_argument_errors():
    for kw in (dict(sampling='best'), dict(sampling=1), dict(sampling='confidence', confidence_cap=float('inf')),
               dict(sampling='confidence', confidence_cap=float('nan')), dict(sampling='confidence2', confidence_cap=20.0),
               dict(sampling='confidence', confidence_cap=4097.0), dict(sampling='confidence', min_confidence=-1.0),
               dict(sampling='confidence2', min_confidence=1000.0)):
        with pytest.raises(ValueError):
            pnp.PnPSolver(4, 4, **kw)
    s = pnp.PnPSolver(4, 4)
    assert (s.sampling, s.confidence_cap) == ('uniform', 1000.0)
    pnp.PnPSolver(4, 4, confidence_cap=5.0, min_confidence=-1.0)          # 'uniform' refuses nothing it accepted before
    pnp.PnPSolver(4, 4, sampling='confidence', confidence_cap=4096.0, min_confidence=0.0)


def _pose_parser():
    ap = argparse.ArgumentParser()
    modes.add_pose_flags(ap)
    return ap


def test_pose_flags_of_the_eval_programs(capsys):
    ap = _pose_parser()
    a = ap.parse_args([])
    assert (a.pose_sampling, a.pose_confidence_cap) == (None, None) and modes.pose_argument(a, ap) is False
    a = ap.parse_args(['--pose'])
    assert modes.pose_argument(a, ap) is True                          # today's values without the new flags
    a = ap.parse_args(['--pose_weighted'])
    assert modes.pose_argument(a, ap) == modes.POSE_WEIGHTED
    a = ap.parse_args(['--pose', '--pose_sampling', 'uniform'])
    assert modes.pose_argument(a, ap) is True
    a = ap.parse_args(['--pose_smooth', '--pose_sampling', 'confidence2', '--pose_confidence_cap', '500'])
    o = modes.pose_argument(a, ap)
    assert isinstance(o, modes.PoseOptions) and (o.weighted, o.sampling, o.confidence_cap) == (True, 'confidence2', 500.0)
    s = modes.solver_of(o, 15, 20)
    assert (s.weighted, s.sampling, s.confidence_cap, s.h, s.w) == (True, 'confidence2', 500.0, 15, 20)
    u = modes.solver_of(True, 15, 20)
    assert (u.weighted, u.sampling) == (False, 'uniform') and modes.solver_of(modes.POSE_WEIGHTED, 15, 20).weighted
    assert modes.solver_of(False, 15, 20) is None and modes.solver_of(s, 1, 1) is s
    for argv, word in ((['--pose_sampling', 'confidence'], '--pose_sampling needs --pose'),
                       (['--pose_confidence_cap', '100'], '--pose_confidence_cap needs --pose'),
                       (['--pose', '--pose_confidence_cap', '100'], '--pose_sampling'),
                       (['--pose', '--pose_sampling', 'confidence', '--pose_confidence_cap', '10'], 'confidence_cap'),
                       (['--pose', '--pose_sampling', 'best'], 'invalid choice')):
        with pytest.raises(SystemExit) as e:
            modes.pose_argument(ap.parse_args(argv), ap)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv


def _run(args):
    e = dict(os.environ)
    e['PYTHONPATH'] = ROOT + os.pathsep + e.get('PYTHONPATH', '')
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, timeout=300)


def test_command_lines_refuse_bad_flag_combinations_before_a_device_is_touched(tmp_path):
    lst = tmp_path / 'list.txt'
    lst.write_text(str(tmp_path / 'missing_coord_0.npy') + '\n')      # never read: the flags are checked first
    out = tmp_path / 'out'
    for flags, word in ((['--confidence_cap', '100'], '--sampling'), (['--sampling', 'best'], 'invalid choice'),
                        (['--sampling', 'confidence', '--confidence_cap', '5000'], '--confidence_cap'),
                        (['--sampling', 'confidence2', '--confidence_cap', '20'], '--confidence_cap'),
                        (['--sampling', 'confidence', '--min_confidence', '-1'], '--min_confidence')):
        r = _run(['-m', 'kfnet_amd.KFNet.pnp', str(lst), str(out)] + flags)
        assert r.returncode == 2 and word in r.stdout, (flags, r.stdout)
        assert not out.exists()
    r = _run(['-m', 'kfnet_amd.KFNet.pnp', '--help'])
    assert r.returncode == 0 and '--sampling' in r.stdout and '--confidence_cap' in r.stdout
    for prog in ('kfnet_amd.KFNet.eval', 'kfnet_amd.SCoordNet.eval'):
        r = _run(['-m', prog, '--help'])
        assert r.returncode == 0 and '--pose_sampling' in r.stdout and '--pose_confidence_cap' in r.stdout, prog
        r = _run(['-m', prog, '--scene', 'chess', '--synthetic', '4', '--random_weights', '--pose_sampling', 'confidence'])
        assert r.returncode == 2 and '--pose_sampling needs --pose' in r.stdout, (prog, r.stdout)


# ---- the rule -------------------------------------------------------------------------------------------------------------

def test_hand_computed_weights():
    conf = np.array([20.1, 20.0625, 21.0, 30.0, 999.99, 1000.0, 1000.5, 4096.0, np.inf], np.float32)
    # (20.1f - 20) * 16 = 1.6 -> q = 2; 1/16 above the threshold -> 1 * 16 * 1/16 = 1 -> q = 2; 1 above -> 17; 10 above -> 161;
    # 979.99 * 16 = 15679.8 -> 15680; at the cap and beyond it, +inf included: 980 * 16 + 1 = 15681
    q = np.array([2, 2, 17, 161, 15680, 15681, 15681, 15681, 15681], np.uint64)
    w1, w2 = G.weights(conf, G.CONFIDENCE), G.weights(conf, G.CONFIDENCE_SQ)
    assert w1.dtype == w2.dtype == np.uint64
    assert np.array_equal(w1, q) and np.array_equal(w2, q * q)
    just_above = np.nextafter(np.float32(20.0), np.float32(30.0))
    assert G.weights(np.array([just_above]), G.CONFIDENCE)[0] == 1                    # q >= 1 always
    # the largest weight there is: cap 4096 over threshold 0
    assert G.weights(np.array([np.inf], np.float32), G.CONFIDENCE_SQ, 0.0, 4096.0)[0] == 65537 ** 2
    assert 32768 * 65537 ** 2 < 1 << 48                                               # total stays below 2^48
    for bad in (dict(min_confidence=-1.0), dict(confidence_cap=20.0), dict(confidence_cap=4097.0),
                dict(confidence_cap=np.inf)):
        with pytest.raises(ValueError):
            G.weights(conf, G.CONFIDENCE, **bad)
    with pytest.raises(ValueError):
        G.weights(conf, 0)


def spread_9x13():
    """A 9x13 frame whose confidences are spread evenly over 25 .. 1000 (raster order)."""
    rng = np.random.default_rng(7)
    R, t = P.random_pose(rng)
    rec = P.synthetic_records(rng, 9, 13, R, t)
    rec[..., 3] = np.linspace(25.0, 1000.0, 117, dtype=np.float32).reshape(9, 13)
    return rec


def test_cumulative_weights_exceed_32_bits_and_targets_are_exact():
    rec = spread_9x13()
    conf = G.candidate_confidence(rec)
    assert conf.size == 117
    for mode in MODES:
        w = G.weights(conf, mode)
        cum = G.cumulative(w)
        exact = np.cumsum([int(x) for x in w], dtype=object)
        assert cum.dtype == np.uint64 and [int(x) for x in cum] == list(exact)
    total = int(cum[-1])
    print('9x13, confidences 25..1000, squared weights: total = %d = %.3f * 2^32' % (total, total / 2.0 ** 32))
    assert total > 2 << 32                                                            # no 32-bit shortcut
    rng = np.random.default_rng(8)
    M64 = (1 << 64) - 1
    for tot in [total, 1, (1 << 48) - 1, 1 << 32, (1 << 32) + 1] + [int(x) for x in rng.integers(1, 1 << 48, 200)]:
        for h in [0, 1, 0xFFFFFFFF, 0x80000000] + [int(x) for x in rng.integers(0, 1 << 32, 50)]:
            wide = h * tot                                                            # fits 128 bits with room to spare
            assert wide < 1 << 128
            hi64, lo64 = wide >> 64, wide & M64                                       # __umul64hi and the low product
            device = ((hi64 << 32) & M64) | (lo64 >> 32)
            assert G.draw_target(h, tot) == wide >> 32 == device and device < tot


@pytest.mark.parametrize('mode', MODES)
def test_equal_confidences_draw_the_uniform_sample(mode):
    checked = 0
    for conf in (20.1, 100.0, 2000.0):
        for n in (4, 5, 16, 117, 300, 4800, 32768):
            cum = G.cumulative(G.weights(np.full(n, conf, np.float32), mode))
            assert int(cum[-1]) == n * int(cum[0])
            for seed in (0, 99, 0xDEADBEEF):
                for frame in (0, 7, 1000):
                    for hyp in range(0, 64, 7):
                        assert G.draw_sample_guided(seed, frame, hyp, cum) == P.draw_sample(seed, frame, hyp, n)
                        checked += 1
    assert checked > 1000


def exhaustion_frame():
    """4x4: fifteen cells at confidence 20.1 (q = 2) and one at 30 (q = 161)."""
    rng = np.random.default_rng(9)
    R, t = P.random_pose(rng)
    rec = P.synthetic_records(rng, 4, 4, R, t)
    rec[..., 3] = np.float32(20.1)
    rec[2, 1, 3] = 30.0
    return rec


def test_sixteen_draws_run_out_where_one_candidate_takes_the_weight():
    rec = exhaustion_frame()
    invalid = {}
    for mode in MODES:
        samples = G.hypotheses_guided(rec, 0, 256, mode, score=False)[0]
        invalid[mode] = int((samples < 0).any(1).sum())
        assert ((samples < 0).all(1) | (samples >= 0).all(1)).all()
        for s in samples[(samples >= 0).all(1)]:
            assert len(set(s.tolist())) == 4 and max(s) < 16
    print('hypotheses without a sample: %d of 256 (weights), %d of 256 (squared weights)' % (invalid[1], invalid[2]))
    assert 0 < invalid[G.CONFIDENCE] < 256, invalid
    assert invalid[G.CONFIDENCE_SQ] == 256, invalid
    assert not (P.hypotheses(rec, 0, 256)[0] < 0).any()                # the uniform draw has no such trouble at n = 16


# ---- what it is for -----------------------------------------------------------------------------------------------------

# Seed of synthetic_frames_confidence; the GPU tests use the same 40 frames.  Of seeds 1 .. 8, this is the first on which
# at most two frames per mode have a runner-up hypothesis whose scoring bracket reaches the winner's (the GPU test checks
# that again) and on which all three samplers solve all 40 frames at 30 % outliers (seeds 1, 5 and 8 each lose one frame
# there, seed 8 under uniform sampling too: a pose a little over 5 cm off, not a sampling failure).
SEED = 4
_SOLVED = {}


def solved(outliers):
    """{'uniform' | 1 | 2: (poses, info)} of the 40 15x20 frames with 64 hypotheses; computed once."""
    if outliers not in _SOLVED:
        recs, gts = G.synthetic_frames_confidence(SEED, 40, 15, 20, outliers)
        with np.errstate(all='ignore'):
            out = {'uniform': P.ransac(recs, hypotheses_n=64)}
            for mode in MODES:
                out[mode] = G.ransac_guided(recs, mode, hypotheses_n=64)
        _SOLVED[outliers] = (recs, gts, out)
    return _SOLVED[outliers]


def test_guided_draws_solve_frames_that_uniform_draws_lose():
    """The margin: a count of solved frames out of 40 has a binomial standard deviation of at most sqrt(40 / 4) = 3.2
    frames, the difference of two such counts at most sqrt(2) * 3.2 = 4.5.  The guided counts must lead by 10 frames,
    more than twice that.  Measured with seeds 1 .. 8 of the generator, frames of 40: uniform 19, 21, 13, 16, 16, 17, 20,
    17; weights 38, 37, 37, 38, 37, 38, 37, 39; squared weights 38, 40, 36, 39, 35, 39, 37, 39."""
    recs, gts, out = solved(0.7)
    n = {k: int(G.within_5cm_5deg(p, gts).sum()) for k, (p, _) in out.items()}
    print('70 %% outliers, frames within 5 cm / 5 deg of 40: uniform %d, weights %d, squared weights %d'
          % (n['uniform'], n[1], n[2]))
    for mode in MODES:
        assert n[mode] >= n['uniform'] + 10, n


def test_guiding_costs_nothing_at_30_percent_outliers():
    recs, gts, out = solved(0.3)
    n = {k: int(G.within_5cm_5deg(p, gts).sum()) for k, (p, _) in out.items()}
    print('30 %% outliers, frames within 5 cm / 5 deg of 40: uniform %d, weights %d, squared weights %d'
          % (n['uniform'], n[1], n[2]))
    assert n == {'uniform': 40, 1: 40, 2: 40}, n


def test_synthetic_confidence_is_informative_not_a_label():
    recs, _ = G.synthetic_frames_confidence(SEED, 4, 15, 20, 0.7)
    c = recs[..., 3]
    assert c.dtype == np.float32 and (c > 20.0).all() and c.min() < 50.0 and c.max() > 100.0
    assert ((c >= 50.0) & (c <= 100.0)).mean() > 0.3          # the band both kinds of cell share
