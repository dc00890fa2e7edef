"""CPU tests of the eval.py metrics: the numpy oracle against hand-computed values
(what pins it), and the host side of kfnet_amd.KFNet.metrics (label reading, step schedule, line format).
The device reduction itself is checked against the oracle in tests/test_gpu_e2e.py and, through the C ABI at every grid size
that matters, against the fp64 restatement tests/metrics_ref.py in tests/test_gpu_metrics.py; that restatement and the inputs
of the GPU test are pinned here, where no GPU is needed."""
import numpy as np
import pytest

import metrics_ref as MR
from oracle import kfnet_metrics_oracle as M
from kfnet_amd.KFNet import metrics as HM


def test_resize_nearest_picks_8y_8x():
    x = np.arange(480 * 640, dtype=np.float32).reshape(480, 640, 1)
    y = M.resize_nearest(x, (60, 80))
    assert y.shape == (60, 80, 1) and y[3, 5, 0] == x[24, 40, 0] and y[59, 79, 0] == x[472, 632, 0]


def test_label_roundtrip(tmp_path):
    a = np.random.default_rng(0).normal(size=(480, 640, 4)).astype(np.float32)
    p = tmp_path / 'l.bin'
    a.tofile(p)                       # README.md:74: labels are numpy .tofile() dumps
    assert np.array_equal(M.read_label(str(p)), a)


def test_coord_loss_known_values():
    pred = np.zeros((1, 2, 2, 3), np.float32)
    unc = np.full((1, 2, 2, 1), np.exp(-1.0), np.float32)       # 3*log(unc) = -3
    gt = np.zeros((2, 2, 2, 3), np.float32)
    gt[1, 0, 0, 0] = 0.1                                         # one pixel 10 cm off in frame 2
    mask = np.ones((2, 2, 2, 1), np.float32)
    mask[0, 1, 1, 0] = 0.0
    loss, acc = M.coord_loss_with_uncertainty(pred, unc, gt, mask)
    # per-pixel NLL: -3 everywhere (capped at <= -2), except the off pixel: -3 + 0.01/(2 e^-2) = -2.963
    off = -3.0 + 0.01 / (2 * np.exp(-2.0))
    valid = 7 + 1.0
    assert np.isclose(loss, (6 * -3.0 + off) / valid, atol=1e-5)
    assert np.isclose(acc, (valid - 1) / valid)                  # the 10 cm pixel exceeds 5 cm
    # cap from above at -2 (KFNet.py:216)
    loss2, _ = M.coord_loss_with_uncertainty(pred, np.ones_like(unc), gt, mask)
    assert np.isclose(loss2, 7 * -2.0 / valid)


def test_nis_band_and_dist_error():
    nis = np.array([0.0, 0.01, 0.5, 1.0, 3.0, -1.0])
    assert np.isclose(M.get_NIS_measurement(nis), 2 / 4.0)       # positives: .01 .5 1 3 -> .5 and 1 in band
    c = np.zeros((2, 2, 3)); g = np.zeros((2, 2, 3)); g[0, 0] = [0.03, 0.04, 0.0]; g[1, 1] = [0.3, 0.4, 0.0]
    m = np.ones((2, 2, 1)); m[1, 1] = 0
    med, dmap = M.dist_error(c, g, m)
    assert np.isclose(med, 5.0) and np.isclose(dmap[0, 0], 5.0) and dmap[1, 1] == 0


def test_log_line_format():
    m = dict(i=3, pair=(2, 3), l_m=-2.5, l_t=-2.4, l_kf=-2.6, a_m=0.5, a_t=0.4, a_kf=0.6, d_m=3.0, d_t=4.0,
             d_kf=2.0, nis=0.7)
    assert M.format_line(m).startswith('3, frame 2~3, l_m = -2.500, l_t = -2.400, l_kf = -2.600, a_m = 0.500')


def test_host_label_grid_equals_tf_nearest_resize(tmp_path):
    a = np.random.default_rng(1).normal(size=(480, 640, 4)).astype(np.float32)
    p = tmp_path / 'l.bin'
    a.tofile(p)
    g = HM.read_label_grid(str(p), (480, 640), (60, 80))
    assert g.shape == (60, 80, 4) and np.array_equal(g, M.resize_nearest(a, (60, 80)))
    assert np.array_equal(HM.resize_nearest(a, (60, 80)), M.resize_nearest(a, (60, 80)))
    assert HM.format_line(dict(i=3, pair=(2, 3), l_m=-2.5, l_t=-2.4, l_kf=-2.6, a_m=0.5, a_t=0.4, a_kf=0.6, d_m=3.0,
                               d_t=4.0, d_kf=2.0, nis=0.7)) == M.format_line(dict(i=3, pair=(2, 3), l_m=-2.5, l_t=-2.4,
                               l_kf=-2.6, a_m=0.5, a_t=0.4, a_kf=0.6, d_m=3.0, d_t=4.0, d_kf=2.0, nis=0.7))


def test_pair_schedule_follows_get_indexes():
    """KFNet/train.py:67-71: [[s+1, s], [s, s+1], ...] per test sequence; 'stairs' sequences are 500 long."""
    ps = HM.pair_schedule(0, 4, 2000, 1000)
    assert ps.tolist() == [[1, 0], [0, 1], [1, 2], [2, 3]]
    assert HM.pair_schedule(998, 4, 2000, 1000).tolist() == [[997, 998], [998, 999], [1001, 1000], [1000, 1001]]
    assert HM.pair_schedule(499, 3, 1000, 500).tolist() == [[498, 499], [501, 500], [500, 501]]
    assert HM.pair_schedule(0, 1, 1, 1000).tolist() == [[0, 0]]
    assert HM.TEST_SEQUENCE_LENGTH['stairs'] == 500 and HM.TEST_SEQUENCE_LENGTH['heads'] == 1000


# -- tests/metrics_ref.py: the fp64 reference of kfn_eval_metrics, and the inputs tests/test_gpu_metrics.py feeds it ---------------
def test_constants_the_reference_squares_in_python_have_the_bits_tensorflow_folds():
    """`dist_threshold * dist_threshold` and `self.min_uncertainty * self.min_uncertainty` are products of Python doubles that
    TensorFlow rounds once to fp32; squaring the rounded factor gives the neighbouring float in both cases."""
    thr2, eps2 = np.float32(0.05 * 0.05), np.float32(1e-5 * 1e-5)
    assert thr2.view(np.uint32) == 0x3B23D70A and (np.float32(0.05) * np.float32(0.05)).view(np.uint32) == 0x3B23D70B
    assert np.float32(float(np.float32(0.05)) ** 2).view(np.uint32) == 0x3B23D70B        # squaring 0.05f in double does not help
    assert eps2.view(np.uint32) == 0x2EDBE6FF and (np.float32(1e-5) * np.float32(1e-5)).view(np.uint32) == 0x2EDBE6FE
    assert np.sqrt(eps2 + eps2).view(np.uint32) == 929907715
    assert MR.THR2 == float(thr2) and MR.MIN_UNC == float(np.float32(1e-5))
    # a pixel exactly 0.05f from its label: d2 = 0x3B23D70B > thr2, inaccurate in the reference; its lower neighbour is accurate
    c = np.zeros((2, 3))
    c[0, 0], c[1, 0] = np.float32(0.05), np.nextafter(np.float32(0.05), np.float32(0))
    g = np.zeros((2, 4))
    g[:, 3] = 1.0
    assert MR.loss_terms(c, np.ones(2), g)['bad'].tolist() == [1.0, 0.0]
    from oracle import kfnet_oracle as O
    z = np.zeros((1, 2, 2, 1), np.float32)
    flow_prob = np.full((4, 64), 1.0 / 64, np.float32)
    offs = O.coord_volume(np.zeros((1, 2, 2, 1)), np.zeros((1, 2, 2, 1)), 8)[1]
    _, unc, _ = O.process_model(flow_prob, np.zeros((4, 1), np.float32), offs, np.zeros((1, 2, 2, 3), np.float32), z)
    assert unc.dtype == np.float32 and np.all(unc.view(np.uint32) == 929907715)


def _frame_fields(case, t, hw):
    h, w = hw
    T4 = np.eye(4, dtype=np.float32)
    if case['M'] is not None:
        T4[:3] = case['M']
    a, b = case['pair'][t]
    grid = lambda x: x.reshape(h, w, -1)
    return M.frame_metrics(t, (a, b), grid(case['meas'][t]), grid(case['temp'][t]), grid(case['kf'][t]), grid(case['rec'][t]),
                           grid(case['nis'][t]), (grid(case['labels'][a]), grid(case['labels'][b])), T4, bool(case['reset'][t]), hw)


@pytest.mark.parametrize('with_transform', [False, True])
def test_metrics_ref_agrees_with_the_oracle_on_every_field(with_transform):
    """Random 17x23 inputs, grid-sized labels (resize_nearest is then the identity).  The oracle works in fp32: counts and
    the NIS share must be equal (the inputs keep every pixel 1e-6 from the squared threshold), sums and medians agree to fp32
    rounding."""
    hw = (17, 23)
    case = MR.make_case(hw[0] * hw[1], with_transform)
    stats, dist, terms = MR.eval_metrics(case['meas'], case['temp'], case['kf'], case['rec'], case['nis'], case['labels'],
                                         case['pair'], case['reset'], case['M'], with_terms=True)
    MR.check_case(case, terms)
    for t in range(MR.T_FRAMES):
        want = _frame_fields(case, t, hw)
        got = MR.log_fields(stats[t], dist[t])
        for k in ('a_m', 'a_t', 'a_kf'):      # the oracle divides the two integers in fp32: the correctly rounded quotient
            assert np.float32(got[k]) == np.float32(want[k]), (t, k)
        assert got['nis'] == want['nis'], t
        for k in ('l_m', 'l_t', 'l_kf', 'd_m', 'd_t', 'd_kf'):
            assert got[k] == pytest.approx(want[k], rel=2e-5, abs=0), (t, k)
    assert stats[MR.NIS_ALL_POSITIVE, 7] == 3 * hw[0] * hw[1] and stats[MR.NIS_NONE_POSITIVE, 7] == 0
    # a reset step: the distance of the prediction is the measurement's, the losses still see the prediction
    for t in np.nonzero(case['reset'])[0]:
        assert np.array_equal(dist[t, 1], dist[t, 0]) and stats[t, 1] != stats[t, 0]


def test_metrics_ref_reproduces_the_hand_computed_values():
    """The cases of test_coord_loss_known_values / test_nis_band_and_dist_error above, through the kernel's interface."""
    f32 = np.float32
    labels = np.zeros((2, 4, 4), f32)
    labels[..., 3] = 1.0
    labels[0, 3, 3] = 0.0
    labels[1, 0, 0] = 0.1                                         # one pixel 10 cm off in the second label
    pred = np.zeros((1, 4, 4), f32)
    pred[..., 3] = np.exp(-1.0)
    nis = np.array([[[0.0, 0.01, 0.5], [1.0, 3.0, -1.0], [0.0, 0.0, 0.0], [-2.0, 0.0, -1.0]]], f32)
    rec = np.zeros((1, 4, 4), f32)
    rec[0, 1, :3] = (0.03, 0.04, 0.0)
    stats, dist = MR.eval_metrics(pred, pred, pred, rec, nis, labels, [(0, 1)], [0])
    u = float(f32(np.exp(-1.0)))
    assert stats[0, 6] == 8.0 and stats[0, 3:6].tolist() == [1.0, 1.0, 1.0]
    assert np.allclose(stats[0, :3], 7 * 3.0 * np.log(u) + float(f32(0.1)) ** 2 / (2 * u * u), rtol=1e-12)
    assert np.isclose(stats[0, 0] / stats[0, 6], (6 * -3.0 + (-3.0 + 0.01 / (2 * np.exp(-2.0)))) / 8.0, atol=1e-5)
    assert stats[0, 7] == 4.0 and stats[0, 8] == 2.0
    assert np.isclose(dist[0, 2, 1], 5.0, rtol=1e-6) and np.isclose(dist[0, 0, 0], 10.0, rtol=1e-6) and dist[0, 0, 1] == 0.0
    pred[..., 3] = 1.0                                            # 3 log 1 = 0 > -2: capped from above
    stats, _ = MR.eval_metrics(pred, pred, pred, rec, nis, labels, [(0, 1)], [0])
    assert stats[0, 0] == 7 * -2.0


@pytest.mark.parametrize('with_transform', [False, True])
@pytest.mark.parametrize('HW', MR.HW_CASES)
def test_inputs_of_the_gpu_metrics_test_populate_every_branch(HW, with_transform):
    """With numpy alone: every case tests/test_gpu_metrics.py launches satisfies its input conditions (MR.check_case)."""
    case = MR.make_case(HW, with_transform)
    _, _, terms = MR.eval_metrics(case['meas'], case['temp'], case['kf'], case['rec'], case['nis'], case['labels'],
                                  case['pair'], case['reset'], case['M'], with_terms=True)
    MR.check_case(case, terms)
