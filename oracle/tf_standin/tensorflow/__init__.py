"""An eager stand-in for the slice of TensorFlow 1.x that the reference's model modules call (KFNet/KFNet.py, KFNet/util.py,
cnn_wrapper/*.py, tools/util.py): test infrastructure, NOT product code and NOT TensorFlow.

Every op runs at once on torch CPU tensors, float64 unless set_float('float32') was called; `tf.float32` and 'float32' mean
"the working float type".  It is written from TensorFlow's documented op semantics; the ops whose semantics are a READING of that
documentation say in their docstrings which rule they implement (SAME padding, conv2d_transpose, contrib.image.translate,
nn.l2_normalize, image.resize_nearest_neighbor, layers.dense), and tests/test_tf_standin.py holds known answers for them.
What TensorFlow itself would compute stays unpinned by this package.

The package is never on sys.path of a normal run: oracle/run_reference.py puts it there in a child process of its own, and
tests load it with importlib under another name.

Variables: layers look their kernel and bias up by composed scope name ('ScoreNet/conv1a/kernel') in the dictionary given to
set_variables(); a missing name is a KeyError.  Results of ops called with name= are kept, in call order, and returned by
named(name).  Anything not defined here raises NotImplementedError (augmentation, batch normalisation, dropout, 3-D
convolutions, sessions, placeholders, optimisers).
"""
import builtins as _b
import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as _F

__version__ = 'standin'
AUTO_REUSE = 'AUTO_REUSE'

_state = {'float': torch.float64, 'scopes': [], 'variables': {}, 'named': {}, 'used': []}

float32 = 'float32'
float64 = 'float64'
int32 = 'int32'
int64 = 'int64'
bool = 'bool'   # noqa: A001  (tf.bool)


# ------------------------------------------------------------------------------------------------------------------------------
# the stand-in's own controls (not TensorFlow API)
# ------------------------------------------------------------------------------------------------------------------------------
def set_float(name):
    """'float64' (default) or 'float32': the type every float tensor, constant and variable gets from now on."""
    _state['float'] = {'float64': torch.float64, 'float32': torch.float32}[name]


def set_variables(values, requires_grad=False):
    """values {composed name: ndarray}.  Each becomes a leaf tensor of the working float type; returns {name: tensor}."""
    vs = {}
    for k, v in values.items():
        t = torch.from_numpy(np.array(v, dtype=np.float64)).to(_state['float'])
        vs[k] = t.requires_grad_(True) if requires_grad else t
    _state['variables'] = vs
    _state['used'] = []
    return vs


def variables_used():
    """Composed names that layers have looked up since set_variables(), in first-use order."""
    return list(_state['used'])


def reset_named():
    _state['named'] = {}


def named(name):
    """The results of every op that was called with name=`name` since reset_named(), in call order."""
    return list(_state['named'].get(name, []))


def constant(value, dtype=None, name=None):
    return _reg(_t(value, dtype), name)


# ------------------------------------------------------------------------------------------------------------------------------
# tensors and shapes
# ------------------------------------------------------------------------------------------------------------------------------
class TensorShape(tuple):
    """get_shape()'s result: a tuple of ints (each dimension is a plain int) with as_list()."""

    def as_list(self):
        return list(self)


class Tensor(torch.Tensor):
    """A torch tensor that answers get_shape(); arithmetic, comparison and slicing are torch's (numpy-style broadcasting, as
    TensorFlow's), and results stay of this class."""

    def get_shape(self):
        return TensorShape(int(d) for d in self.shape)


def _dtype(d):
    if d is None:
        return None
    if isinstance(d, torch.dtype):
        return d
    d = str(d)
    if d in ('float32', 'float64', 'float'):
        return _state['float']
    if d in ('int32', 'int64'):
        return torch.int64
    if d == 'bool':
        return torch.bool
    raise NotImplementedError('dtype %r' % (d,))


def _t(x, dtype=None):
    """Anything -> Tensor.  Python and numpy floats take the working float type, integers int64."""
    want = _dtype(dtype)
    if isinstance(x, torch.Tensor):
        t = x
    else:
        if isinstance(x, (list, tuple)) and any(isinstance(e, torch.Tensor) for e in x):
            t = torch.stack([_t(e) for e in x])
        else:
            a = np.asarray(x)
            if a.dtype.kind == 'f':
                t = torch.from_numpy(a.astype(np.float64)).to(_state['float'])
            elif a.dtype.kind in 'iu':
                t = torch.from_numpy(a.astype(np.int64))
            elif a.dtype.kind == 'b':
                t = torch.from_numpy(a)
            else:
                raise TypeError('cannot convert %r' % (x,))
    if want is not None and t.dtype != want:
        t = t.to(want)
    return t.as_subclass(Tensor)


def _pair(a, b):
    """Two operands of a binary op, a Python number taking the other side's type as in TensorFlow."""
    ta = isinstance(a, torch.Tensor)
    tb = isinstance(b, torch.Tensor)
    if ta and not tb:
        return _t(a), _t(b, a.dtype if a.dtype.is_floating_point or isinstance(b, int) else None)
    if tb and not ta:
        return _t(a, b.dtype if b.dtype.is_floating_point or isinstance(a, int) else None), _t(b)
    return _t(a), _t(b)


def _reg(t, name):
    t = t.as_subclass(Tensor) if isinstance(t, torch.Tensor) else _t(t)
    if name is not None:
        if t.requires_grad and not t.is_leaf:
            t.retain_grad()
        _state['named'].setdefault(name, []).append(t)
    return t


def _ints(shape):
    if isinstance(shape, torch.Tensor):
        return [int(v) for v in shape.reshape(-1).tolist()]
    return [int(v) for v in shape]


# ------------------------------------------------------------------------------------------------------------------------------
# scopes
# ------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def variable_scope(name, reuse=None, **kw):
    """Variable names compose with '/': variable_scope('ScoreNet') around a layer named 'conv1a' gives
    'ScoreNet/conv1a/kernel'.  Entering a scope again reuses its variables (AUTO_REUSE is the only mode)."""
    _state['scopes'].append(name)
    try:
        yield name
    finally:
        _state['scopes'].pop()


@contextlib.contextmanager
def name_scope(name, *a, **kw):
    """Op names are not composed here: named() is keyed by the bare name= string."""
    yield name


@contextlib.contextmanager
def device(name):
    yield


def _variable(layer_name, var):
    full = '/'.join(_state['scopes'] + [layer_name, var])
    v = _state['variables'][full]
    if full not in _state['used']:
        _state['used'].append(full)
    return v


# ------------------------------------------------------------------------------------------------------------------------------
# elementwise
# ------------------------------------------------------------------------------------------------------------------------------
def _binary(fn):
    def op(x, y, name=None):
        a, b = _pair(x, y)
        return _reg(fn(a, b), name)
    return op


add = _binary(lambda a, b: a + b)
subtract = _binary(lambda a, b: a - b)
multiply = _binary(lambda a, b: a * b)
div = _binary(lambda a, b: a / b if a.dtype.is_floating_point else torch.div(a, b, rounding_mode='floor'))
divide = _binary(lambda a, b: a / b)
maximum = _binary(torch.maximum)
minimum = _binary(torch.minimum)
equal = _binary(lambda a, b: a == b)


def _unary(fn):
    def op(x, name=None):
        return _reg(fn(_t(x)), name)
    return op


square = _unary(lambda a: a * a)
sqrt = _unary(torch.sqrt)
exp = _unary(torch.exp)
log = _unary(torch.log)
abs = _unary(torch.abs)   # noqa: A001
floor = _unary(torch.floor)
tanh = _unary(torch.tanh)
ones_like = _unary(torch.ones_like)
identity = _unary(lambda a: a)


def add_n(inputs, name=None):
    """Sum of a list, accumulated left to right."""
    acc = _t(inputs[0])
    for v in inputs[1:]:
        acc = acc + _t(v)
    return _reg(acc, name)


def clip_by_value(t, clip_value_min, clip_value_max, name=None):
    t = _t(t)
    lo, hi = _t(clip_value_min, t.dtype), _t(clip_value_max, t.dtype)
    return _reg(torch.minimum(torch.maximum(t, lo), hi), name)


def cast(x, dtype, name=None):
    return _reg(_t(x).to(_dtype(dtype)) if isinstance(x, torch.Tensor) else _t(x, dtype), name)


def convert_to_tensor(value, dtype=None, name=None):
    return _reg(_t(value, dtype), name)


# ------------------------------------------------------------------------------------------------------------------------------
# reductions
# ------------------------------------------------------------------------------------------------------------------------------
def reduce_sum(x, axis=None, keepdims=False, name=None):
    x = _t(x)
    return _reg(x.sum() if axis is None else x.sum(dim=axis, keepdim=keepdims), name)


def reduce_mean(x, axis=None, keepdims=False, name=None):
    x = _t(x)
    return _reg(x.mean() if axis is None else x.mean(dim=axis, keepdim=keepdims), name)


def count_nonzero(x, axis=None, name=None):
    """Number of elements != 0, an integer tensor."""
    if axis is not None:
        raise NotImplementedError('count_nonzero(axis=)')
    return _reg((_t(x) != 0).sum(), name)


# ------------------------------------------------------------------------------------------------------------------------------
# shapes, slices, gathers
# ------------------------------------------------------------------------------------------------------------------------------
def shape(x, name=None):
    return _reg(_t(list(_t(x).shape)), name)


def zeros(shape, dtype=float32, name=None):
    return _reg(torch.zeros(_ints(shape), dtype=_dtype(dtype)), name)


def ones(shape, dtype=float32, name=None):
    return _reg(torch.ones(_ints(shape), dtype=_dtype(dtype)), name)


def range(start, limit=None, delta=1, name=None):   # noqa: A001
    if limit is None:
        start, limit = 0, start
    return _reg(torch.arange(int(start), int(limit), int(delta), dtype=torch.int64), name)


def linspace(start, stop, num, name=None):
    return _reg(torch.linspace(float(start), float(stop), int(num), dtype=_state['float']), name)


def reshape(tensor, shape, name=None):
    return _reg(_t(tensor).reshape(_ints(shape)), name)


def transpose(a, perm=None, name=None):
    a = _t(a)
    if perm is None:
        perm = list(reversed(_b.range(a.dim())))
    return _reg(a.permute(*_ints(perm)), name)


def expand_dims(input, axis=None, name=None, dim=None):   # noqa: A002
    return _reg(_t(input).unsqueeze(axis if axis is not None else dim), name)


def squeeze(input, axis=None, name=None, squeeze_dims=None):   # noqa: A002
    t = _t(input)
    axis = axis if axis is not None else squeeze_dims
    if axis is None:
        return _reg(t.squeeze(), name)
    if isinstance(axis, int):
        axis = [axis]
    for ax in sorted((a % t.dim() for a in axis), reverse=True):
        if t.shape[ax] != 1:
            raise ValueError('cannot squeeze dimension %d of %s' % (ax, tuple(t.shape)))
        t = t.squeeze(ax)
    return _reg(t, name)


def tile(input, multiples, name=None):   # noqa: A002
    return _reg(_t(input).repeat(*_ints(multiples)), name)


def concat(values, axis, name=None):
    vs = [_t(v) for v in values]
    return _reg(torch.cat(vs, dim=axis), name)


def stack(values, axis=0, name=None):
    return _reg(torch.stack([_t(v) for v in values], dim=axis), name)


def split(value, num_or_size_splits, axis=0, name=None):
    v = _t(value)
    if isinstance(num_or_size_splits, int):
        return [p.as_subclass(Tensor) for p in torch.chunk(v, num_or_size_splits, dim=axis)]
    return [p.as_subclass(Tensor) for p in torch.split(v, _ints(num_or_size_splits), dim=axis)]


def slice(input_, begin, size, name=None):   # noqa: A001
    """input_[begin[i] : begin[i] + size[i]] along every axis; size -1 means "to the end"."""
    t = _t(input_)
    idx = []
    for d, (b, s) in enumerate(zip(_ints(begin), _ints(size))):
        idx.append(_b.slice(b, t.shape[d] if s == -1 else b + s))
    return _reg(t[tuple(idx)], name)


def gather(params, indices, name=None, axis=0):
    """params[indices] along axis 0; an index outside the range is an error, as on TensorFlow's CPU kernel."""
    if axis != 0:
        raise NotImplementedError('gather(axis != 0)')
    p, i = _t(params), _t(indices).to(torch.int64)
    if i.numel() and (int(i.min()) < 0 or int(i.max()) >= p.shape[0]):
        raise IndexError('gather index out of range')
    return _reg(p[i], name)


def matmul(a, b, name=None):
    """Matrix product over the last two axes, leading axes batched."""
    return _reg(torch.matmul(_t(a), _t(b)), name)


def matrix_inverse(input, name=None):   # noqa: A002
    return _reg(torch.linalg.inv(_t(input)), name)


# ------------------------------------------------------------------------------------------------------------------------------
# the ops that are readings of TensorFlow's documentation
# ------------------------------------------------------------------------------------------------------------------------------
def same_padding(n, k, s):
    """TensorFlow's 'SAME' rule for one axis (tf.nn.convolution, "Note on padding"): out = ceil(n / s), the total padding is
    max((out - 1) s + k - n, 0), and the SMALLER half goes in front (pad_before = total // 2).  Returns (out, before, after)."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return out, total // 2, total - total // 2


def _two(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def _conv2d_nhwc(x, kernel, strides, padding):
    """Cross-correlation (no kernel flip) of NHWC x with an HWIO kernel: y[b,o,p,co] = sum x[b, o s + i - pad_top,
    p s + j - pad_left, ci] kernel[i,j,ci,co], zeros outside."""
    kh, kw = kernel.shape[0], kernel.shape[1]
    sh, sw = strides
    xt = x.permute(0, 3, 1, 2)
    if padding.upper() == 'SAME':
        _, pt, pb = same_padding(x.shape[1], kh, sh)
        _, pl, pr = same_padding(x.shape[2], kw, sw)
        xt = _F.pad(xt, (pl, pr, pt, pb))
    elif padding.upper() != 'VALID':
        raise NotImplementedError('padding %r' % (padding,))
    return _F.conv2d(xt, kernel.permute(3, 2, 0, 1).contiguous(), stride=(sh, sw)).permute(0, 2, 3, 1)


def _conv2d_transpose_nhwc(y, kernel, strides, padding):
    """tf.nn.conv2d_transpose, which TensorFlow documents as "the transpose (gradient) of conv2d": with an HWIO-of-the-forward
    kernel [kh,kw,C_out_of_this_op,C_in_of_this_op], the result is d<conv2d(x, kernel), y>/dx for x of the output size.
    tf.layers.conv2d_transpose infers that size under 'SAME' as input * stride (under 'VALID' as (input-1) stride + k).
    Entry by entry: out[b, o s + i - pad_top, p s + j - pad_left, c] += y[b,o,p,d] kernel[i,j,c,d], pad_* being the forward
    convolution's SAME padding for the output size; entries that land outside are dropped."""
    kh, kw = kernel.shape[0], kernel.shape[1]
    sh, sw = strides
    full = _F.conv_transpose2d(y.permute(0, 3, 1, 2), kernel.permute(3, 2, 0, 1).contiguous(), stride=(sh, sw))
    if padding.upper() == 'SAME':
        Ho, Wo = y.shape[1] * sh, y.shape[2] * sw
        _, pt, _ = same_padding(Ho, kh, sh)
        _, pl, _ = same_padding(Wo, kw, sw)
        full = _F.pad(full, (0, max(Wo + pl - full.shape[3], 0), 0, max(Ho + pt - full.shape[2], 0)))
        full = full[:, :, pt:pt + Ho, pl:pl + Wo]
    elif padding.upper() != 'VALID':
        raise NotImplementedError('padding %r' % (padding,))
    return full.permute(0, 2, 3, 1)


def _finish(y, layer_name, use_bias, activation, name_for_registry=None):
    if use_bias:
        y = y + _variable(layer_name, 'bias')
    y = y.as_subclass(Tensor)
    if activation is not None:
        y = activation(y)
    return _reg(y, name_for_registry)


class _Layers(object):
    def __getattr__(self, item):
        raise NotImplementedError('tf.layers.%s is outside the stand-in' % item)

    @staticmethod
    def conv2d(inputs, filters, kernel_size, strides=1, padding='valid', activation=None, use_bias=True, trainable=True,
               reuse=None, name=None, **kw):
        """tf.layers.conv2d, channels_last: variables '<scope>/<name>/kernel' [kh,kw,Cin,filters] and '<scope>/<name>/bias'
        [filters]; cross-correlation, 'SAME' by same_padding(); bias, then activation."""
        if kw:
            raise NotImplementedError('conv2d arguments %s' % sorted(kw))
        x = _t(inputs)
        k = _variable(name, 'kernel')
        kh, kw_ = _two(kernel_size)
        assert tuple(k.shape) == (kh, kw_, x.shape[3], filters), (name, tuple(k.shape), tuple(x.shape), filters)
        return _finish(_conv2d_nhwc(x, k, _two(strides), padding), name, use_bias, activation)

    @staticmethod
    def conv2d_transpose(inputs, filters, kernel_size, strides=1, padding='valid', activation=None, use_bias=True,
                         trainable=True, reuse=None, name=None, **kw):
        """tf.layers.conv2d_transpose, channels_last: kernel [kh,kw,filters,Cin] (output channels BEFORE input channels),
        bias [filters]; see _conv2d_transpose_nhwc for the arithmetic."""
        if kw:
            raise NotImplementedError('conv2d_transpose arguments %s' % sorted(kw))
        x = _t(inputs)
        k = _variable(name, 'kernel')
        kh, kw_ = _two(kernel_size)
        assert tuple(k.shape) == (kh, kw_, filters, x.shape[3]), (name, tuple(k.shape), tuple(x.shape), filters)
        return _finish(_conv2d_transpose_nhwc(x, k, _two(strides), padding), name, use_bias, activation)

    @staticmethod
    def dense(inputs, units, activation=None, use_bias=True, trainable=True, reuse=None, name=None, **kw):
        """tf.layers.dense: kernel [in, units], y = x . kernel + bias over the last axis, then activation."""
        if kw:
            raise NotImplementedError('dense arguments %s' % sorted(kw))
        x = _t(inputs)
        k = _variable(name, 'kernel')
        assert tuple(k.shape) == (x.shape[-1], units), (name, tuple(k.shape), tuple(x.shape), units)
        return _finish(torch.matmul(x, k), name, use_bias, activation)


class _NN(object):
    def __getattr__(self, item):
        raise NotImplementedError('tf.nn.%s is outside the stand-in' % item)

    @staticmethod
    def relu(features, name=None):
        return _reg(_F.relu(_t(features)), name)

    @staticmethod
    def tanh(x, name=None):
        return _reg(torch.tanh(_t(x)), name)

    @staticmethod
    def softmax(logits, axis=None, name=None, dim=None):
        """exp(x - max) / sum exp(x - max) over `axis` (default, and `dim`'s old spelling: the last)."""
        ax = axis if axis is not None else (dim if dim is not None else -1)
        return _reg(torch.softmax(_t(logits), dim=ax), name)

    @staticmethod
    def l2_normalize(x, axis=None, epsilon=1e-12, name=None, dim=None):
        """x * rsqrt(max(sum(x^2, axis), epsilon)), epsilon = 1e-12: the floor is on the SUM OF SQUARES, not on the norm."""
        ax = axis if axis is not None else dim
        x = _t(x)
        ss = (x * x).sum(dim=ax, keepdim=True)
        return _reg(x * torch.rsqrt(torch.maximum(ss, _t(epsilon, x.dtype))), name)


class _Image(object):
    def __getattr__(self, item):
        raise NotImplementedError('tf.image.%s is outside the stand-in' % item)

    @staticmethod
    def resize_nearest_neighbor(images, size, align_corners=False, name=None):
        """TF 1.x, align_corners=False: out[r, c] = in[min(floor(r * in_h / out_h), in_h - 1), min(floor(c * in_w / out_w),
        in_w - 1)] -- the top-left sample of each cell, no half-pixel offset.  The scale is the float32 quotient in_/out, as
        the kernel computes it."""
        if align_corners:
            raise NotImplementedError('align_corners=True')
        x = _t(images)
        oh, ow = _ints(size)
        ih, iw = x.shape[1], x.shape[2]

        def index(n_in, n_out):
            scale = np.float32(n_in) / np.float32(n_out)
            src = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
            return torch.from_numpy(np.minimum(src, n_in - 1))
        return _reg(x[:, index(ih, oh)][:, :, index(iw, ow)], name)


class _ContribImage(object):
    def __getattr__(self, item):
        raise NotImplementedError('tf.contrib.image.%s is outside the stand-in' % item)

    @staticmethod
    def translate(images, translations, interpolation='NEAREST', name=None):
        """tf.contrib.image.translate(images, [dx, dy]): the content MOVES by dx to the right and dy down, so
        out[y, x] = in[y - dy, x - dx], and what comes from outside the image is 0.  (It is transform() with the projective
        row [1, 0, -dx, 0, 1, -dy, 0, 0], which maps an OUTPUT point to the INPUT point it is read from.)  Integer shifts
        only, so NEAREST and BILINEAR would agree; only NEAREST is accepted."""
        if interpolation != 'NEAREST':
            raise NotImplementedError('interpolation %r' % (interpolation,))
        x = _t(images)
        dx, dy = translations
        if int(dx) != dx or int(dy) != dy:
            raise NotImplementedError('fractional translation')
        dx, dy = int(dx), int(dy)
        H, W = x.shape[-3], x.shape[-2]
        out = torch.zeros_like(x)
        ys0, ys1 = max(dy, 0), min(H + dy, H)
        xs0, xs1 = max(dx, 0), min(W + dx, W)
        if ys0 < ys1 and xs0 < xs1:
            out[..., ys0:ys1, xs0:xs1, :] = x[..., ys0 - dy:ys1 - dy, xs0 - dx:xs1 - dx, :]
        return _reg(out, name)


class _Contrib(object):
    image = _ContribImage()

    def __getattr__(self, item):
        raise NotImplementedError('tf.contrib.%s is outside the stand-in' % item)


layers = _Layers()
nn = _NN()
image = _Image()
contrib = _Contrib()
pi = math.pi


def __getattr__(item):
    if item.startswith('__'):
        raise AttributeError(item)
    raise NotImplementedError('tf.%s is outside the stand-in (oracle/tf_standin)' % item)
