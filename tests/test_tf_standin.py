"""Known answers for oracle/tf_standin/tensorflow: the eager stand-in over which oracle/run_reference.py runs the reference's own
model modules.  The ops tested here are the ones whose semantics are a READING of TensorFlow's documentation; each expected
value below is worked out by hand from the rule quoted in the op's docstring.  What TensorFlow itself computes stays unpinned.

The package is loaded with importlib under another name: it is never importable as `tensorflow` in a normal run."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_standin():
    path = os.path.join(ROOT, 'oracle', 'tf_standin', 'tensorflow', '__init__.py')
    spec = importlib.util.spec_from_file_location('kfn_tf_standin', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture()
def tf():
    mod = load_standin()
    mod.set_float('float64')
    return mod


def test_the_standin_is_not_importable_as_tensorflow():
    assert 'tensorflow' not in sys.modules or getattr(sys.modules['tensorflow'], '__version__', '') != 'standin'
    assert not any(os.path.abspath(p or '.').startswith(os.path.join(ROOT, 'oracle', 'tf_standin')) for p in sys.path)


@pytest.mark.parametrize('n,k,s,want', [(4, 3, 2, (2, 0, 1)), (5, 3, 2, (3, 1, 1)), (8, 3, 2, (4, 0, 1)), (7, 3, 1, (7, 1, 1)),
                                        (1, 3, 2, (1, 1, 1)), (2, 3, 2, (1, 0, 1)), (6, 1, 1, (6, 0, 0)), (5, 1, 2, (3, 0, 0)),
                                        (9, 4, 3, (3, 0, 1))])
def test_same_padding_rule(tf, n, k, s, want):
    """pad = max((ceil(n / s) - 1) s + k - n, 0), the smaller half first."""
    assert tf.same_padding(n, k, s) == want


def test_conv2d_same_stride_2_puts_the_smaller_half_of_the_padding_first(tf):
    """A row 1 2 3 4 under the taps 1, 10, 100 at stride 2: the one padding column is on the RIGHT, so y = (321, 43); were it on
    the left, y would be (210, 432).  A row of five has one column on either side: (210, 432, 54)."""
    tf.set_variables({'c/kernel': np.array([1.0, 10.0, 100.0]).reshape(1, 3, 1, 1)})
    y = tf.layers.conv2d(tf.constant(np.array([1.0, 2, 3, 4]).reshape(1, 1, 4, 1)), 1, (1, 3), 2, 'SAME', use_bias=False, name='c')
    assert y.get_shape().as_list() == [1, 1, 2, 1] and y.reshape(-1).tolist() == [321.0, 43.0]
    y = tf.layers.conv2d(tf.constant(np.array([1.0, 2, 3, 4, 5]).reshape(1, 1, 5, 1)), 1, (1, 3), 2, 'SAME', use_bias=False, name='c')
    assert y.reshape(-1).tolist() == [210.0, 432.0, 54.0]
    # the same along the rows, with a bias and an activation after it
    tf.set_variables({'c/kernel': np.array([1.0, 10.0, 100.0]).reshape(3, 1, 1, 1), 'c/bias': np.array([-400.0])})
    y = tf.layers.conv2d(tf.constant(np.array([1.0, 2, 3, 4]).reshape(1, 4, 1, 1)), 1, (3, 1), 2, 'SAME', activation=tf.nn.relu, name='c')
    assert y.reshape(-1).tolist() == [0.0, 0.0]
    y = tf.layers.conv2d(tf.constant(np.array([1.0, 2, 3, 4]).reshape(1, 4, 1, 1)), 1, (3, 1), 2, 'SAME', name='c')
    assert y.reshape(-1).tolist() == [-79.0, -357.0]


def test_conv2d_kernel_layout_is_hwio_without_a_flip(tf):
    k = np.zeros((3, 3, 2, 3))
    k[0, 2, 1, 2] = 1.0                                   # output channel 2 reads input channel 1 one row up, one column right
    tf.set_variables({'c/kernel': k})
    x = np.zeros((1, 5, 5, 2))
    x[0, 1, 3, 1] = 7.0
    y = tf.layers.conv2d(tf.constant(x), 3, 3, 1, 'SAME', use_bias=False, name='c').numpy()
    assert y[0, 2, 2, 2] == 7.0 and np.count_nonzero(y) == 1


@pytest.mark.parametrize('stride,hw', [(1, (5, 7)), (2, (3, 5)), (2, (1, 1)), (2, (4, 3))])
def test_conv2d_transpose_is_the_exact_transpose_of_conv2d(tf, stride, hw):
    """<conv(x), y> == <x, conv_T(y)> in fp64 with ONE kernel array: [kh,kw,Cin,Cout] for conv2d is [kh,kw,filters,Cin'] for
    conv2d_transpose.  y has the (odd) size hw, x the size conv2d_transpose infers under SAME: hw * stride."""
    rng = np.random.default_rng([stride, hw[0], hw[1]])
    cin, cout = 3, 4
    k = rng.normal(size=(3, 3, cin, cout))
    tf.set_variables({'c/kernel': k})
    x = tf.constant(rng.normal(size=(2, hw[0] * stride, hw[1] * stride, cin)))
    y = tf.constant(rng.normal(size=(2, hw[0], hw[1], cout)))
    cx = tf.layers.conv2d(x, cout, 3, stride, 'SAME', use_bias=False, name='c')
    ty = tf.layers.conv2d_transpose(y, cin, 3, stride, 'SAME', use_bias=False, name='c')
    assert cx.get_shape() == y.get_shape() and ty.get_shape() == x.get_shape()
    a, b = float((cx * y).sum()), float((x * ty).sum())
    assert abs(a - b) <= 1e-12 * max(abs(a), 1.0), (a, b)


def test_conv2d_transpose_known_answer(tf):
    """One input cell of value 1 at stride 2, k = 3: the forward convolution from 2x2 pads (0, 1), so the output is the kernel's
    upper-left 2x2 block, out[i, j, c] = kernel[i, j, c, 0]; then the bias."""
    k = np.arange(3 * 3 * 2 * 1, dtype=np.float64).reshape(3, 3, 2, 1)
    tf.set_variables({'u/kernel': k, 'u/bias': np.array([0.5, -0.5])})
    y = tf.layers.conv2d_transpose(tf.constant(np.ones((1, 1, 1, 1))), 2, 3, 2, 'SAME', name='u').numpy()
    assert y.shape == (1, 2, 2, 2)
    assert np.array_equal(y[0], k[:2, :2, :, 0] + np.array([0.5, -0.5]))


def test_translate_moves_an_impulse_by_dx_right_and_dy_down_and_fills_with_zero(tf):
    x = np.zeros((1, 5, 6, 2))
    x[0, 2, 3] = (1.0, 2.0)
    y = tf.contrib.image.translate(tf.constant(x), [1, -2], interpolation='NEAREST').numpy()
    assert y[0, 0, 4].tolist() == [1.0, 2.0] and np.count_nonzero(y) == 2
    y = tf.contrib.image.translate(tf.constant(x), [-3, 1], interpolation='NEAREST').numpy()
    assert y[0, 3, 0].tolist() == [1.0, 2.0] and np.count_nonzero(y) == 2
    assert not tf.contrib.image.translate(tf.constant(x), [3, 0], interpolation='NEAREST').numpy().any()      # pushed out
    ramp = np.arange(12, dtype=np.float64).reshape(1, 3, 4, 1) + 1.0
    y = tf.contrib.image.translate(tf.constant(ramp), [1, 0], interpolation='NEAREST').numpy()[0, :, :, 0]
    assert np.array_equal(y, np.array([[0, 1, 2, 3], [0, 5, 6, 7], [0, 9, 10, 11.0]]))
    with pytest.raises(NotImplementedError):
        tf.contrib.image.translate(tf.constant(x), [1, 0], interpolation='BILINEAR')


def test_resize_nearest_neighbor_on_an_index_ramp(tf):
    rows, cols = np.meshgrid(np.arange(64.0), np.arange(96.0), indexing='ij')
    x = np.stack([rows, cols], -1)[None]
    y = tf.image.resize_nearest_neighbor(tf.constant(x), [8, 12]).numpy()[0]
    assert np.array_equal(y[:, 0, 0], np.arange(8) * 8.0) and np.array_equal(y[0, :, 1], np.arange(12) * 8.0)
    y = tf.image.resize_nearest_neighbor(tf.constant(x[:, :5, :7]), [3, 4]).numpy()[0]          # floor(i 5/3), floor(j 7/4)
    assert y[:, 0, 0].tolist() == [0.0, 1.0, 3.0] and y[0, :, 1].tolist() == [0.0, 1.0, 3.0, 5.0]
    y = tf.image.resize_nearest_neighbor(tf.constant(x[:, :3, :3]), [6, 3]).numpy()[0]          # enlarging: floor(i / 2)
    assert y[:, 0, 0].tolist() == [0.0, 0.0, 1.0, 1.0, 2.0, 2.0]
    same = tf.image.resize_nearest_neighbor(tf.constant(x[:, :8, :12]), [8, 12]).numpy()
    assert np.array_equal(same, x[:, :8, :12])


def test_l2_normalize_floors_the_sum_of_squares_at_1e_12(tf):
    x = np.array([[3.0, 4.0], [0.0, 0.0], [1e-7, 0.0], [2e-6, 0.0]])
    y = tf.nn.l2_normalize(tf.constant(x), axis=-1).numpy()
    assert np.allclose(y[0], [0.6, 0.8], rtol=1e-15) and not y[1].any()
    assert np.isclose(y[2, 0], 1e-7 * 1e6, rtol=1e-12)          # below the floor: x / sqrt(1e-12)
    assert np.isclose(y[3, 0], 1.0, rtol=1e-12)                 # above it (4e-12): a unit vector
    assert np.array_equal(tf.nn.l2_normalize(tf.constant(x), dim=-1).numpy(), y)


def test_dense_kernel_is_in_by_out(tf):
    tf.set_variables({'fc/kernel': np.array([[1.0, 10.0, 100.0], [2.0, 20.0, 200.0]]), 'fc/bias': np.array([0.5, 0.0, -1000.0])})
    y = tf.layers.dense(tf.constant(np.array([[1.0, 1.0], [1.0, -1.0]])), 3, activation=tf.nn.relu, name='fc').numpy()
    assert np.array_equal(y, np.array([[3.5, 30.0, 0.0], [0.0, 0.0, 0.0]]))


def test_scopes_compose_variable_names_and_named_results_are_kept(tf):
    tf.set_variables({'ScoreNet/conv1a/kernel': np.ones((1, 1, 1, 1)), 'ScoreNet/conv1a/bias': np.zeros(1),
                      'Temporal/fc1/kernel': np.ones((1, 1)), 'Temporal/fc1/bias': np.zeros(1)})
    x = tf.constant(np.ones((1, 2, 2, 1)))
    with tf.variable_scope('ScoreNet'):
        with tf.name_scope('ignored'), tf.device('/device:CPU:0'):
            tf.layers.conv2d(x, 1, 1, 1, 'SAME', name='conv1a', reuse=tf.AUTO_REUSE, trainable=False)
    with tf.variable_scope('Temporal'):
        tf.layers.dense(tf.reshape(x, [4, 1]), 1, name='fc1')
        with pytest.raises(KeyError):
            tf.layers.dense(tf.reshape(x, [4, 1]), 1, name='fc2')
    assert tf.variables_used() == ['ScoreNet/conv1a/kernel', 'ScoreNet/conv1a/bias', 'Temporal/fc1/kernel', 'Temporal/fc1/bias']
    tf.reset_named()
    a = tf.add(x, 1.0, name='flow')
    b = tf.reshape(x, [4], name='flow')
    assert [t.data_ptr() for t in tf.named('flow')] == [a.data_ptr(), b.data_ptr()] and tf.named('nothing') == []
    assert x.get_shape().as_list() == [1, 2, 2, 1] and len(x.get_shape()) == 4


def test_what_is_outside_the_list_raises(tf):
    for call in (lambda: tf.placeholder, lambda: tf.Session, lambda: tf.layers.batch_normalization, lambda: tf.layers.conv3d,
                 lambda: tf.layers.dropout, lambda: tf.nn.local_response_normalization, lambda: tf.image.random_brightness,
                 lambda: tf.contrib.image.rotate, lambda: tf.contrib.layers, lambda: tf.train):
        with pytest.raises(NotImplementedError):
            call()


def test_elementwise_slices_and_gathers(tf):
    x = tf.constant(np.arange(24.0).reshape(1, 2, 3, 4))
    assert tf.slice(x, [0, 0, 1, 2], [-1, -1, 1, -1]).numpy().tolist() == [[[[6.0, 7.0]], [[18.0, 19.0]]]]
    a, b = tf.split(x, [1, 3], axis=3)
    assert a.get_shape().as_list() == [1, 2, 3, 1] and b.numpy()[0, 1, 2].tolist() == [21.0, 22.0, 23.0]
    assert tf.gather(tf.reshape(x, [-1, 4]), tf.cast(tf.constant([5.0, 0.0]), 'int32')).numpy()[:, 0].tolist() == [20.0, 0.0]
    with pytest.raises(IndexError):
        tf.gather(tf.reshape(x, [-1, 4]), tf.constant([6]))
    assert tf.tile(tf.constant([[1.0, 2.0]]), [2, 2]).numpy().tolist() == [[1.0, 2.0, 1.0, 2.0]] * 2
    assert float(tf.minimum(tf.constant(-3.0), -2.0)) == -3.0 and float(tf.minimum(tf.constant(-1.0), -2.0)) == -2.0
    assert int(tf.count_nonzero(tf.maximum(tf.constant([-1.0, 0.5, 0.0]), 0))) == 1
    assert tf.clip_by_value(tf.constant([-1.0, 5.0, 2.0]), 0.0, tf.cast(3, 'float32')).numpy().tolist() == [0.0, 3.0, 2.0]
    assert tf.transpose(x, [0, 2, 1, 3]).get_shape().as_list() == [1, 3, 2, 4]
    assert float(tf.reduce_sum(x)) == 276.0 and tf.reduce_mean(x, axis=3, keepdims=True).get_shape().as_list() == [1, 2, 3, 1]
    inv = tf.matrix_inverse(tf.constant(np.array([[[2.0, 0.0], [0.0, 4.0]]]))).numpy()
    assert np.array_equal(inv, np.array([[[0.5, 0.0], [0.0, 0.25]]]))
    m = tf.matmul(tf.constant(np.ones((3, 1, 2))), tf.constant(np.ones((3, 2, 5))))
    assert m.get_shape().as_list() == [3, 1, 5] and float(m.sum()) == 30.0
    p = tf.nn.softmax(tf.constant(np.array([[0.0, np.log(3.0)]])), axis=-1).numpy()
    assert np.allclose(p, [[0.25, 0.75]], rtol=1e-15)


def test_float32_switch(tf):
    tf.set_float('float32')
    try:
        x = tf.constant(np.array([0.1]))
        assert x.dtype == torch.float32 and tf.cast(x, tf.float32).dtype == torch.float32
        assert tf.maximum(x, 1e-5 * 1e-5).dtype == torch.float32 and tf.ones([2]).dtype == torch.float32
        V = tf.set_variables({'a/kernel': np.ones((1, 1))}, requires_grad=True)
        assert V['a/kernel'].dtype == torch.float32 and V['a/kernel'].requires_grad
        # a Python double constant is rounded ONCE to float32, as TensorFlow folds it: float32(1e-10), not float32(1e-5)^2
        eps2 = float(tf.maximum(tf.constant(0.0), 1e-5 * 1e-5))
        assert eps2 == float(np.float32(1e-5 * 1e-5)) != float(np.float32(1e-5) * np.float32(1e-5))
    finally:
        tf.set_float('float64')
    assert tf.constant(np.array([0.1])).dtype == torch.float64
