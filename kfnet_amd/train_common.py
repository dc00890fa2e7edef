"""What the three trainers share on the host (DESIGN.md 6b "Shared host pieces"): the flat parameter store with its Adam
step and state dict, the snapshot writer and reader, the lazily read step statistics, and the library's size queries.
kfnet_amd.train, train_flow and train_kfnet build on it; nothing here loads libkfnet_hip.so before a launch needs it, so the
store works on CPU tensors too."""
import ctypes as C
import os

import numpy as np

from . import _lib, staging

BETA1, BETA2, EPSILON = 0.9, 0.999, 1e-8          # tf.train.AdamOptimizer defaults (KFNet/train.py:313)
WEIGHTS_NAME = 'kfnet_weights-%d.npz'             # tools.io.get_snapshot's kind: SCoordNet.eval --model_folder reads it
STATE_NAME = 'kfnet_train_state-%d.npz'           # NOT matched by get_snapshot's kfnet_weights*.npz


def learning_rate(base_lr, gamma, stepvalue, global_step):
    """tf.train.exponential_decay without staircase (KFNet/train.py:306-310): a real-valued exponent."""
    return float(base_lr) * float(gamma) ** (float(global_step) / float(stepvalue))


def adam_lr_t(lr, t):
    """lr_t of TensorFlow's Adam for update number t (from 1)."""
    return lr * np.sqrt(1.0 - BETA2 ** t) / (1.0 - BETA1 ** t)


def snapshot_paths(folder, step):
    return os.path.join(folder, WEIGHTS_NAME % step), os.path.join(folder, STATE_NAME % step)


def size_query(fn, *args):
    """What one of the library's size queries (workspace bytes, pack floats) writes through its last, size_t* argument."""
    n = C.c_size_t()
    _lib.check(fn(*(args + (C.byref(n),))), fn.__name__)
    return n.value


class ParamStore(object):
    """The variables of one scope in flat float32 buffers -- params, grads and Adam's m and v -- with a slot per variable:
    slots[TF name] = (offset, count, shape), in the order of `specs` = [(TF name, shape)], every offset a multiple of 4
    floats.  It fills named slots from a dict and reads them back, holds the counters and the schedule, and issues the fp32
    Adam launch.  The two trainers are stores; `_packs_stale` tells them that params changed under their packed copies."""

    def __init__(self, specs, device='cpu', base_lr=1e-4, gamma=0.5, stepvalue=1, weight_decay=0.0):
        import torch
        self.torch, self.device = torch, torch.device(device)
        self.base_lr, self.gamma, self.stepvalue = float(base_lr), float(gamma), float(stepvalue)
        self.weight_decay = float(weight_decay)
        self.global_step = self.adam_t = 0
        self.slots, off = {}, 0
        for name, shape in specs:
            n = int(np.prod(shape))
            self.slots[name] = (off, n, tuple(shape))
            off += -(-n // 4) * 4
        self.num_floats = off
        f32 = dict(dtype=torch.float32, device=self.device)
        self.params, self.grads = torch.zeros(off, **f32), torch.zeros(off, **f32)
        self.m, self.v = torch.zeros(off, **f32), torch.zeros(off, **f32)
        self._packs_stale = True

    def _fill(self, buf, arrays, prefix=''):
        """Every variable's slot of the flat buffer `buf` from arrays[prefix + its name]."""
        for name, (off, n, shape) in self.slots.items():
            if prefix + name not in arrays:
                raise KeyError('weights lack %s%s' % (prefix, name))
            a = np.ascontiguousarray(np.asarray(arrays[prefix + name], dtype=np.float32))
            if a.shape != tuple(shape):
                raise ValueError('%s%s has shape %s, expected %s' % (prefix, name, a.shape, tuple(shape)))
            buf[off:off + n].copy_(self.torch.from_numpy(a.reshape(-1)))

    def _named(self, buf, prefix=''):
        host = buf.cpu().numpy()
        return {prefix + name: host[off:off + n].reshape(shape).copy() for name, (off, n, shape) in self.slots.items()}

    def set_weights(self, weights):
        self._fill(self.params, weights)
        self._packs_stale = True

    def weights(self):
        """{TF variable name: float32 array}: what kfnet_amd.weights.save_npz stores and the engines load."""
        return self._named(self.params)

    def gradients(self):
        """Debug view of the last step's gradients of the loss (without the regulariser, which kfn_adam_step adds), in TF
        layout under the variables' names."""
        return self._named(self.grads)

    def state(self):
        """The counters and the Adam slots, as numpy arrays (an .npz's content)."""
        st = dict(global_step=np.int64(self.global_step), adam_t=np.int64(self.adam_t))
        st.update(self._named(self.m, 'adam_m/'))
        st.update(self._named(self.v, 'adam_v/'))
        return st

    def load_slots(self, st):
        """Adam's m and v from the adam_m/* and adam_v/* of a state dict; the counters stay."""
        self._fill(self.m, st, 'adam_m/')
        self._fill(self.v, st, 'adam_v/')

    def zero_slots(self):
        self.m.zero_()
        self.v.zero_()

    def load_state(self, st):
        self.load_slots(st)
        self.global_step, self.adam_t = int(st['global_step']), int(st['adam_t'])

    def save(self, folder, step=None):
        """Writes kfnet_weights-<step>.npz (self.weights()) and kfnet_train_state-<step>.npz (self.state()); returns the two
        paths.  KFNetTrainer, which holds two stores, borrows it."""
        from .weights import save_npz
        step = self.global_step if step is None else step
        os.makedirs(folder, exist_ok=True)
        wp, sp = snapshot_paths(folder, step)
        save_npz(wp, self.weights())
        np.savez(sp, **self.state())
        return wp, sp

    def apply_gradients(self, stream=None, counters=None):
        """TensorFlow's Adam on the flat buffer, with the regulariser's weight_decay * w folded into the gradient.  Update
        number global_step + 1 with Adam's t = adam_t + 1, from this store's counters or from `counters` = (global_step,
        adam_t) -- joint stage 3 steps Temporal/* with SCoordNet's; both advance.  Returns the learning rate."""
        stream = staging.current_stream(self.device) if stream is None else stream
        if counters is not None:
            self.global_step, self.adam_t = counters
        lr = learning_rate(self.base_lr, self.gamma, self.stepvalue, self.global_step)
        t = self.adam_t + 1
        _lib.check(_lib.load().kfn_adam_step(self.params.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                             self.grads.data_ptr(), self.num_floats, adam_lr_t(lr, t), BETA1, BETA2, EPSILON,
                                             self.weight_decay, stream), 'kfn_adam_step')
        self.adam_t = t
        self.global_step += 1
        self._packs_stale = True
        return lr


class LazyStats(object):
    """What a step reports, read from the device on first access (so that steps queue).  A subclass names its KEYS and
    decodes the stats vector: _decode(host array) -> {key: number}.  dict(stats) gives plain numbers."""
    KEYS = ()

    def __init__(self, stats_dev, lr):
        self._dev, self._lr, self._host = stats_dev, lr, None

    def keys(self):
        return list(self.KEYS)

    def __getitem__(self, k):
        if self._host is None:
            self._host = self._decode(self._dev.cpu().numpy())
        return self._host[k]


def read_snapshot(model_folder, scopes, verbose=True):
    """The newest snapshot of a model folder -- a TF checkpoint or a kfnet_weights*.npz -- and the kfnet_train_state-<step>.npz
    beside it, if any: (weights, Adam state or None, step), or (None, None, 0) where there is no folder or no snapshot.
    `scopes` is what a TF checkpoint yields (an .npz yields all it holds).  Prints load_snapshot's line, then which of the two
    cases the Adam slots are."""
    from .tools.io import get_snapshot
    from .weights import load_snapshot
    snapshot, step = get_snapshot(model_folder) if model_folder and os.path.isdir(model_folder) else (None, 0)
    if snapshot is None:
        return None, None, 0
    W = load_snapshot(snapshot, scopes=scopes, verbose=verbose)
    sp = snapshot_paths(model_folder, step)[1]
    state = None
    if os.path.exists(sp):
        with np.load(sp) as z:
            state = {k: z[k] for k in z.files}
    if verbose:
        print('Adam slots restored from %s' % sp if state is not None else
              'no %s: the Adam slots start at zero' % os.path.basename(sp))
    return W, state, step
