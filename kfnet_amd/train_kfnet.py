"""Stage 3 of the reference's procedure ("Train KFNet"): fine-tuning SCoordNet through the Kalman filter with OFlowNet frozen
(--fix_flownet; KFNet/train.py:268-298 with KFNet.GetKFCoordBatch, KFNet/KFNet.py:102-162), or training both
networks through it (train_flownet=True, the reference's default; KFNet/train.py:282-303).

A step sees S groups of T consecutive frames (T = 4 on the command line).  Its launches, on top of kfnet_amd.train's:

    flow        OFlowNetEngine.heavy on the Temporal/* weights, on a stream of its own: flow and sigma_trans of every frame
                from the frame before it in group order -- constants of the step (slot 0 of a group means nothing)
    forward     SCoordNetTrainer.forward on the S T frames
    measurement kfn_measurement_map: (z, exp(log sigma)) from the raw prediction
    filter      kfn_kalman_scan_ex with a reset on frame 0 of every group: the launch eval runs, writing the temporal and KF maps
    loss        kfn_filter_loss_grad: 0.2 L_measure + 0.2 L_temporal + 0.6 L_KF and the direct gradients of the three outputs
                (reproj_weights only) kfn_reproj_loss_grad behind it: weight_measure * w_m * R_m + weight_temporal * w_t * R_t +
                weight_kf * w_kf * R_KF of KFNet.ReprojectionLoss, gradients added to those of the three outputs
    backward    kfn_filter_backward: the reverse scan, whose measurement gradients join d(loss)/d(prediction);
                then SCoordNetTrainer.backward, Adam and the packs as in stage 1

Only ScoreNet/* is trained and regularised; Temporal/* is handed through unchanged.

With train_flownet=True an OFlowNetTrainer stands where the frozen engine stood: the S (T - 1) pairs (t - 1, t) of the groups
share the staged frames, its forward pass (activations kept) gives flow and sigma_trans, kfn_filter_backward_joint emits their
gradients beside the measurement's, OFlowNetTrainer.backward takes them down to feat1 on the flow stream beside SCoordNet's
backward pass, and both scopes take an Adam step with one global_step, learning rate and weight decay.

There is no fallback: a missing entry point raises, and so does a flow outside the radius the reverse scan gathers over.
"""
import ctypes as C

import numpy as np

from . import _lib, staging
from .train import LAYERS, SCOPE, SCoordNetTrainer
from .train_common import LazyStats, ParamStore, read_snapshot, size_query

FLOW_SCOPE = 'Temporal'
GROUP = 4                                 # frames per group, KFNet/train.py:60-66
LOSS_WEIGHTS = (0.2, 0.2, 0.6)            # measure, temporal, KF: KFNet/train.py:293-295
RADIUS = 4                                # the soft-argmax over the offsets -4..3 cannot leave it
MIN_UNCERTAINTY = 1e-5
FLOW_MESSAGE = '%d pixels have a flow beyond the radius %d of kfn_filter_backward: their gradient would be lost'


def sequence_length(scene):
    """The length of the ranges get_indexes draws its groups from (KFNet/train.py:75-141)."""
    return 500 if scene == 'stairs' else 1000


def group_list(count, length, group=GROUP):
    """KFNet/train.py:60-66 over the ranges [k length, min((k + 1) length, count)): every [i, .., i + group - 1] inside a range
    followed by its reverse.  A range shorter than `group` yields nothing."""
    groups = []
    for start in range(0, count, length):
        end = min(start + length, count)
        for i in range(start, end - (group - 1)):
            fwd = list(range(i, i + group))
            groups.append(fwd)
            groups.append(fwd[::-1])
    return groups


def group_indices(step, S, groups, shuffle=False, seed=0):
    """The frames of update number `step` (from 0): groups step S .. step S + S - 1 of the list, wrapping round; with `shuffle`
    position q of the stream is entry q % n of a permutation drawn per epoch q // n from (seed, epoch).  A function of its
    arguments alone, so a resumed run continues the same stream.  Returns S T indices, group after group."""
    from .train import batch_indices
    out = []
    for g in batch_indices(step, S, len(groups), shuffle, seed):
        out.extend(groups[g])
    return out


def pair_table(S, T):
    """The pairs of a joint step over S groups of T frames: (a_idx, b_idx), pair s (T - 1) + t - 1 = frames (s T + t - 1, s T + t)
    for t = 1 .. T - 1.  OFlowNet sees frame b = t from frame a = t - 1, as the eval engine does."""
    b = np.array([s * T + t for s in range(S) for t in range(1, T)], dtype=np.int64)
    return b - 1, b


def split_state(st, scopes=(SCOPE, FLOW_SCOPE)):
    """Which of `scopes` a train-state file carries Adam slots for: {scope: bool}."""
    return {scope: any(k.startswith('adam_m/%s/' % scope) for k in st) for scope in scopes}


def start_step(snapshot_step, stepvalue, reset_step, scoordnet, oflownet):
    """set_stepvalue's rule (KFNet/train.py:348-350, :364-365): with both --scoordnet and --oflownet the step is reset to 4
    stepvalue; otherwise an explicit --reset_step wins over the snapshot's step."""
    if scoordnet and oflownet:
        return 4 * stepvalue
    return snapshot_step if reset_step < 0 else reset_step


class StepStats(LazyStats):
    """loss, l_measure, l_temp, l_KF (each NLL + 50 smoothness, as the reference logs them), a_measure, a_temp, a_KF, pixels,
    lr.  The read-back raises when a flow left the radius of the reverse scan."""
    KEYS = ('loss', 'l_measure', 'l_temp', 'l_KF', 'a_measure', 'a_temp', 'a_KF', 'pixels', 'lr')
    REPROJ_KEYS = ('l_reproj_measure', 'l_reproj_temp', 'l_reproj_kf')   # reproj_weights only: the three R; `loss` includes them

    def __init__(self, stats_dev, lr, radius, reproj_dev=None):
        LazyStats.__init__(self, stats_dev, lr)
        self._radius, self._reproj_dev = radius, reproj_dev

    def keys(self):
        return list(self.KEYS) + (list(self.REPROJ_KEYS) if self._reproj_dev is not None else [])

    def _decode(self, s):
        check_flow_count(s, self._radius)
        host = dict(loss=float(s[0]), l_measure=float(s[12]), l_temp=float(s[13]), l_KF=float(s[14]), a_measure=float(s[7]),
                    a_temp=float(s[8]), a_KF=float(s[9]), pixels=float(s[10]) - 1.0, lr=self._lr)
        if self._reproj_dev is not None:
            r = self._reproj_dev.cpu().numpy()       # kfn_reproj_loss_grad's stats: the three R, their weighted sum
            host.update(l_reproj_measure=float(r[0]), l_reproj_temp=float(r[1]), l_reproj_kf=float(r[2]),
                        loss=float(s[0]) + float(r[3]))
        return host


def check_flow_count(stats_host, radius):
    n = int(np.asarray(stats_host, dtype=np.float32).view(np.uint32)[11])
    if n:
        raise _lib.KfnError(FLOW_MESSAGE % (n, radius))


class KFNetTrainer(object):
    def __init__(self, weights, image_size=(480, 640), groups=1, group=GROUP, transform=None, base_lr=1e-4, gamma=0.5,
                 stepvalue=80000, weight_decay=1e-4, loss_clip=None, smooth_weight=50.0, loss_weights=LOSS_WEIGHTS,
                 radius=RADIUS, device='cuda:0', train_flownet=False, overlap=True, reproj_weights=None, camera=None):
        """weights: {TF name: array} holding ScoreNet/* and Temporal/*.  groups = S, group = T.  The other arguments are
        SCoordNetTrainer's; loss_weights = (measure, temporal, KF).  train_flownet: train Temporal/* too, with the same
        schedule and weight decay; overlap: run its backward pass on the flow stream beside SCoordNet's (else behind it).
        reproj_weights: None, or (w_m, w_t, w_kf) of the reprojection terms that join L_measure, L_temporal and L_KF (the
        reference: 50, 10, 10); all zero = None: nothing of the term is launched or allocated.  camera: the
        kfnet_amd.labels.DepthCamera of the cells' rays (None: the 7-Scenes defaults).  Every step() then needs a set_poses()."""
        import torch
        from .engine import OFlowNetEngine
        if groups < 1 or group < 2:
            raise ValueError('groups must be >= 1 and group >= 2')
        self.S, self.T = int(groups), int(group)
        B = self.S * self.T
        self.sc = SCoordNetTrainer(weights, image_size=image_size, batch=B, transform=transform, base_lr=base_lr, gamma=gamma,
                                   stepvalue=stepvalue, weight_decay=weight_decay, loss_clip=loss_clip,
                                   smooth_weight=smooth_weight, device=device)
        sc = self.sc
        self.torch, self.lib, self.device = torch, sc.lib, sc.device
        self.loss_weights = tuple(float(x) for x in loss_weights)
        self.radius = int(radius)
        from .reproj import check_weights
        self.reproj_weights = None if reproj_weights is None else check_weights(reproj_weights, 3)
        if self.reproj_weights is not None and not any(self.reproj_weights):
            self.reproj_weights = None
        self.reproj = None
        self._poses_set = False
        self.train_flownet, self.overlap = bool(train_flownet), bool(overlap)
        self.flow_weights = {k: np.asarray(v, dtype=np.float32).copy() for k, v in weights.items()
                             if k.startswith(FLOW_SCOPE + '/')}
        h, w = sc.grid
        with torch.cuda.device(self.device):
            self.flow_stream = torch.cuda.Stream(device=self.device)
            self.ev_frames, self.ev_flow = torch.cuda.Event(), torch.cuda.Event()
            f32 = dict(dtype=torch.float32, device=self.device)
            if self.train_flownet:
                from .train_flow import OFlowNetTrainer
                self.engine = None
                self.ft = OFlowNetTrainer(self.flow_weights, image_size=image_size, pairs=self.S * (self.T - 1), base_lr=base_lr,
                                          gamma=gamma, stepvalue=stepvalue, weight_decay=weight_decay, device=device, frames=B,
                                          pair_index=pair_table(self.S, self.T))
                self.ev_back, self.ev_flow_done = torch.cuda.Event(), torch.cuda.Event()
                # flow and sigma_trans in the scan's [S,T,hw] layout (slot 0 of a group is never read) and their gradients
                self.c_flow, self.c_sigma = torch.zeros((B, h, w, 2), **f32), torch.zeros((B, h, w), **f32)
                self.d_flow, self.d_sigma = torch.zeros((B, h, w, 2), **f32), torch.zeros((B, h, w), **f32)
            else:
                with torch.cuda.stream(self.flow_stream):
                    self.engine = OFlowNetEngine(self.flow_weights, image_size=image_size, batch=self.T, max_chunk=B, device=device)
                self.flow_stream.synchronize()
            self.meas = torch.zeros((B, h, w, 4), **f32)
            self.temp = torch.zeros((B, h, w, 4), **f32)
            self.kf = torch.zeros((B, h, w, 4), **f32)
            self.d_temp = torch.zeros((B, h, w, 4), **f32)
            self.d_kf = torch.zeros((B, h, w, 4), **f32)
            self.records = torch.zeros((B, h, w, 4), **f32)
            self.filter_state = torch.zeros((self.S, h, w, 4), **f32)
            self.stats = torch.zeros(16, **f32)
            if self.reproj_weights is not None:
                from .reproj import ReprojTerm
                self.reproj = ReprojTerm(B, h, w, camera, sc.transform, self.device)
            self._flow_count = torch.zeros(1, dtype=torch.int32).pin_memory()
            self.ev_count = torch.cuda.Event()
            # frame 0 of every group is a reset frame (t0 = 0, reset_period = T): both estimates equal the measurement
            self.scan_desc = _lib.KalmanDesc(S=self.S, T=self.T, H=h, W=w, t0=0, reset_period=self.T,
                                             min_uncertainty=MIN_UNCERTAINTY, nis_gate=0.0, has_transform=0)
            need = size_query(self.lib.kfn_kalman_scan_scratch_bytes, C.byref(self.scan_desc))
            self.scan_scratch = torch.zeros(-(-need // 4), **f32) if need else None
            self.back_desc = _lib.FilterBackwardDesc(S=self.S, T=self.T, H=h, W=w, ld_dpred=sc.dact[-1].shape[3],
                                                     radius=self.radius, min_uncertainty=MIN_UNCERTAINTY)
            need = size_query(self.lib.kfn_filter_backward_scratch_bytes, C.byref(self.back_desc))
            self.back_scratch = torch.zeros(-(-need // 4), **f32)

    # ---- what the stage-1 trainer keeps ------------------------------------------------------------------------------
    global_step = property(lambda self: self.sc.global_step, lambda self, v: setattr(self.sc, 'global_step', v))
    adam_t = property(lambda self: self.sc.adam_t)

    def weights(self):
        """Both scopes: ScoreNet/* as trained, Temporal/* as given (as trained with train_flownet) -- what KFNet.eval
        --model_folder reads."""
        W = self.sc.weights()
        W.update(self.ft.weights() if self.train_flownet else {k: v.copy() for k, v in self.flow_weights.items()})
        return W

    def gradients(self):
        g = self.sc.gradients()
        if self.train_flownet:
            g.update(self.ft.gradients())
        return g

    def state(self):
        """One file's content: the counters and ScoreNet/*'s Adam slots, with train_flownet Temporal/*'s beside them."""
        st = self.sc.state()
        if self.train_flownet:
            st.update({k: v for k, v in self.ft.state().items() if k.startswith('adam_')})
        return st

    def load_state(self, st, verbose=True):
        """With train_flownet a state of an --fix_flownet run, of stage 1 or of stage 2 loads too: the slots of the scope it
        lacks start at zero."""
        if not self.train_flownet:
            self.sc.load_state(st)
            return
        for scope, held in split_state(st).items():
            tr = self.sc if scope == SCOPE else self.ft
            if held:
                tr.load_slots(st)
            else:
                tr.zero_slots()
                if verbose:
                    print('the train state holds no Adam slots of %s/*: they start at zero' % scope)
        self.sc.global_step, self.sc.adam_t = int(st['global_step']), int(st['adam_t'])

    save = ParamStore.save        # both scopes' weights() and state() in the two files

    # ---- one step ----------------------------------------------------------------------------------------------------
    def flow(self, main):
        """The frozen OFlowNet on the staged frames, on its own stream, ordered against `main` by events: it starts when the
        frames are staged, and `main` waits for it in front of the filter."""
        self.ev_frames.record(main)
        self.flow_stream.wait_event(self.ev_frames)
        with self.torch.cuda.stream(self.flow_stream):
            if self.train_flownet:
                self.flow_forward()
            else:
                self.engine.heavy(self.sc.frames, self.S * self.T)
            self.ev_flow.record(self.flow_stream)

    def flow_forward(self):
        """OFlowNetTrainer's forward pass on the frames SCoordNet staged, on torch's current stream; then its flow [P hw,2] and
        sigma_trans [P hw] into slots 1 .. T-1 of every group of the scan's layout."""
        ft, (S, T) = self.ft, (self.S, self.T)
        ft.stage(self.sc.frames)
        ft.forward()
        self.c_flow.view(S, T, -1, 2)[:, 1:].copy_(ft.flow.view(S, T - 1, -1, 2))
        self.c_sigma.view(S, T, -1)[:, 1:].copy_(ft.sigma.view(S, T - 1, -1))

    def flow_backward(self, main):
        """The gradients of the reverse scan back in the pair layout, then OFlowNetTrainer.backward: on the flow stream behind
        an event (overlap), so that it runs beside SCoordNet's backward pass, or on `main`."""
        ft, (S, T) = self.ft, (self.S, self.T)
        side = self.flow_stream if self.overlap else main
        if self.overlap:
            self.ev_back.record(main)
            side.wait_event(self.ev_back)
        with self.torch.cuda.stream(side):
            ft.d_flow.view(S, T - 1, -1, 2).copy_(self.d_flow.view(S, T, -1, 2)[:, 1:])
            ft.d_sigma.view(S, T - 1, -1).copy_(self.d_sigma.view(S, T, -1)[:, 1:])
            ft.backward(stream=side.cuda_stream)

    def _scan_inputs(self):
        if self.train_flownet:
            return self.c_flow.data_ptr(), self.c_sigma.data_ptr()
        return self.engine.c_flow.ptr, self.engine.c_sigma.ptr

    def forward(self, stream=None):
        """SCoordNet, the measurement map and the filter: self.meas, self.temp, self.kf.  The flow must have been launched
        (self.flow) on the same frames."""
        sc = self.sc
        main = self.torch.cuda.current_stream(self.device)
        stream = main.cuda_stream if stream is None else stream
        sc.forward(stream)
        B, (h, w) = sc.batch, sc.grid
        _lib.check(self.lib.kfn_measurement_map(sc.act[-1].data_ptr(), LAYERS[-1][3], self.meas.data_ptr(), B * h * w, stream),
                   'kfn_measurement_map')
        main.wait_event(self.ev_flow)
        _lib.check(self.lib.kfn_memset(self.filter_state.data_ptr(), 0, self.filter_state.numel() * 4, stream),
                   'kfn_memset state')
        c_flow, c_sigma = self._scan_inputs()
        _lib.check(self.lib.kfn_kalman_scan_ex(C.byref(self.scan_desc), c_flow, c_sigma, self.meas.data_ptr(),
                                               self.filter_state.data_ptr(), self.records.data_ptr(), self.temp.data_ptr(), None,
                                               self.kf.data_ptr(), 0,
                                               self.scan_scratch.data_ptr() if self.scan_scratch is not None else None, stream),
                   'kfn_kalman_scan_ex')

    def loss(self, label_stride, stream=None):
        sc = self.sc
        stream = staging.current_stream(self.device) if stream is None else stream
        B, (h, w) = sc.batch, sc.grid
        d = _lib.FilterLossDesc(B=B, h=h, w=w, ld_pred=LAYERS[-1][3], ld_dpred=sc.dact[-1].shape[3], label_stride=label_stride,
                                img_stride=8, has_transform=int(sc.transform is not None),
                                has_loss_clip=int(sc.loss_clip is not None), loss_clip=sc.loss_clip or 0.0,
                                smooth_weight=sc.smooth_weight, weight_measure=self.loss_weights[0],
                                weight_temporal=self.loss_weights[1], weight_kf=self.loss_weights[2], dist_threshold=0.05,
                                min_uncertainty=MIN_UNCERTAINTY)
        if sc.transform is not None:
            d.transform = (C.c_float * 12)(*[float(x) for x in sc.transform[:3].reshape(-1)])
        _lib.check(self.lib.kfn_filter_loss_grad(C.byref(d), sc.act[-1].data_ptr(), self.temp.data_ptr(), self.kf.data_ptr(),
                                                 sc.labels.data_ptr(), sc.frames.data_ptr(), sc.dact[-1].data_ptr(),
                                                 self.d_temp.data_ptr(), self.d_kf.data_ptr(), self.stats.data_ptr(), stream),
                   'kfn_filter_loss_grad')
        if self.reproj is not None:           # adds into the three gradient buffers: behind the loss, in front of the reverse scan
            wr, wl = self.reproj_weights, self.loss_weights
            self.reproj.launch([(sc.act[-1], sc.dact[-1], wl[0] * wr[0]), (self.temp, self.d_temp, wl[1] * wr[1]),
                                (self.kf, self.d_kf, wl[2] * wr[2])], sc.labels, label_stride, None, self.stats, 10, stream)

    def filter_backward(self, stream=None):
        stream = staging.current_stream(self.device) if stream is None else stream
        c_flow, c_sigma = self._scan_inputs()
        if self.train_flownet:
            _lib.check(self.lib.kfn_filter_backward_joint(C.byref(self.back_desc), c_flow, c_sigma, self.meas.data_ptr(),
                                                          self.temp.data_ptr(), self.kf.data_ptr(), self.d_temp.data_ptr(),
                                                          self.d_kf.data_ptr(), self.sc.dact[-1].data_ptr(), self.d_flow.data_ptr(),
                                                          self.d_sigma.data_ptr(), self.stats.data_ptr(),
                                                          self.back_scratch.data_ptr(), stream), 'kfn_filter_backward_joint')
            return
        _lib.check(self.lib.kfn_filter_backward(C.byref(self.back_desc), c_flow, self.meas.data_ptr(),
                                                self.temp.data_ptr(), self.kf.data_ptr(), self.d_temp.data_ptr(),
                                                self.d_kf.data_ptr(), self.sc.dact[-1].data_ptr(), self.stats.data_ptr(),
                                                self.back_scratch.data_ptr(), stream), 'kfn_filter_backward')

    def set_poses(self, poses):
        """The camera-to-world 4x4 of each of the S T frames of the NEXT step, as SCoordNetTrainer.set_poses."""
        if self.reproj is not None:
            with self.torch.cuda.device(self.device):
                self.reproj.set_poses(poses)
            self._poses_set = True

    def step(self, frames_u8, labels):
        """One update on S groups: frames uint8 [S T,H,W,3] group after group in group order, labels float32 [S T,H,W,4] or
        grid-sized.  Returns StepStats of THIS step's loss, before the update, read back only when accessed.  Raises, before the
        update is queued, when a flow left the radius of the reverse scan.  With reproj_weights set_poses() must have handed over
        this batch's poses (ValueError otherwise)."""
        sc, torch = self.sc, self.torch
        if self.reproj is not None and not self._poses_set:
            raise ValueError('the reprojection term needs the poses of this batch: call set_poses(poses) before every step')
        self._poses_set = False
        with torch.cuda.device(self.device):
            main = torch.cuda.current_stream(self.device)
            stream = main.cuda_stream
            stride = sc.stage(frames_u8, labels, None, stream)
            self.flow(main)
            self.forward(stream)
            self.loss(stride, stream)
            self.filter_backward(stream)
            self._flow_count.copy_(self.stats.view(torch.int32)[11:12], non_blocking=True)
            self.ev_count.record(main)
            if self.train_flownet:
                self.flow_backward(main)
            sc.backward(stream)
            stats = self.stats.clone()
            # the one wait of a step: for the reverse scan's counter, while the backward pass is still queued
            self.ev_count.synchronize()
            if int(self._flow_count[0]):
                raise _lib.KfnError(FLOW_MESSAGE % (int(self._flow_count[0]), self.radius))
            if self.train_flownet:
                self.flow_update(main)
            lr = sc.apply_gradients(stream)
            sc._repack(stream)
            reproj = self.reproj.stats.clone() if self.reproj is not None else None
        return StepStats(stats, lr, self.radius, reproj)

    def flow_update(self, main):
        """Temporal/*'s Adam step and packs with SCoordNet's counters, where its backward pass ran; `main` then waits for the
        flow stream, so that the next step may overwrite the frames."""
        side = self.flow_stream if self.overlap else main
        with self.torch.cuda.stream(side):
            self.ft.apply_gradients(side.cuda_stream, counters=(self.sc.global_step, self.sc.adam_t))
            self.ft._repack(side.cuda_stream)
        if self.overlap:
            self.ev_flow_done.record(side)
            main.wait_event(self.ev_flow_done)


def restore(model_folder, scoordnet='', oflownet='', verbose=True):
    """The reference's restore order (KFNet/train.py:398-408): the newest snapshot of model_folder (all scopes), then
    ScoreNet/* from the newest snapshot of `scoordnet`, then Temporal/* from that of `oflownet`.  Returns (weights -- possibly
    lacking a scope --, Adam state or None, step of model_folder's snapshot)."""
    from .tools.io import get_snapshot
    from .weights import load_snapshot
    W, state, step = read_snapshot(model_folder, (SCOPE, FLOW_SCOPE), verbose)
    W = W or {}
    for folder, scope in ((scoordnet, SCOPE), (oflownet, FLOW_SCOPE)):
        if not folder:
            continue
        snapshot, _ = get_snapshot(folder)
        if snapshot is None:
            raise ValueError('no kfnet_weights*.npz or model.ckpt-*.index in %s' % folder)
        if verbose:
            print('Restore from scope', scope, ':', snapshot)
        part = load_snapshot(snapshot, scopes=(scope,), verbose=verbose)
        W.update({k: v for k, v in part.items() if k.startswith(scope + '/')})
    return W, state, step
