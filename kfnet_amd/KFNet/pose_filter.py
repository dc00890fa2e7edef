"""Temporal smoothing of the per-frame camera poses: a random-walk error-state Kalman filter on the device
(kfn_pose_filter, DESIGN.md 5c "Uncertainty"), and the pose tracker (kfn_pose_track, DESIGN.md 5c "Pose tracker"): the
same recursion under a walk or a constant-velocity model, with backward smoothing and a carried state (PoseTracker, below).

`PnPSolver.solve_unc` gives every frame's camera-to-world pose with the 6x6 covariance of its body-frame perturbation
(dtheta, drho), C ~ C_hat [exp(dtheta) | drho].  `PoseFilter.run` fuses a sequence of them forwards in time: a frame
without a pose is bridged by the prediction, a pose whose normalised innovation squared exceeds the gate is rejected,
and `max_rejects` rejections in a row re-initialise the state from the measurement.  rot_sigma, trans_sigma (per
frame) and the gate are the user's model of the camera's motion, not tolerances.
"""
import ctypes as C

import numpy as np

from .. import _lib

FLAG_NAMES = {_lib.POSE_UPDATED: 'updated', _lib.POSE_MISSING: 'missing', _lib.POSE_REJECTED: 'rejected',
              _lib.POSE_INIT: 'initialised', _lib.POSE_NONE: 'no estimate'}


def position_covariance(pose, cov):
    """Covariance [..,3,3] of the camera centre in the scene frame: R_c2w Sigma_tau,tau R_c2w^T for camera-to-world poses
    [..,4,4] and their covariances [..,6,6] (rotation block first)."""
    pose = np.asarray(pose, dtype=np.float64)
    cov = np.asarray(cov, dtype=np.float64)
    R = pose[..., :3, :3]
    return R @ cov[..., 3:, 3:] @ np.swapaxes(R, -1, -2)


class PoseFilter(object):
    """run(poses [T,4,4] or [S,T,4,4], cov [T,6,6] or [S,T,6,6]) -> (poses, cov, flags, nis) of the same leading shape;
    flags are _lib.POSE_*; nis is NaN where no test was made.  numpy in, numpy out; CUDA tensors in, tensors out (no
    sync)."""

    def __init__(self, rot_sigma=0.02, trans_sigma=0.02, gate=22.46, max_rejects=3):
        if not (float(rot_sigma) >= 0.0 and float(trans_sigma) >= 0.0):
            raise ValueError('rot_sigma and trans_sigma must be >= 0')
        if not float(gate) > 0.0:
            raise ValueError('gate must be > 0')
        if int(max_rejects) < 1:
            raise ValueError('max_rejects must be >= 1')
        self.rot_sigma, self.trans_sigma, self.gate = float(rot_sigma), float(trans_sigma), float(gate)
        self.max_rejects = int(max_rejects)

    def desc(self, S, T):
        return _lib.PoseFilterDesc(S=S, T=T, rot_sigma=self.rot_sigma, trans_sigma=self.trans_sigma, gate=self.gate,
                                   max_rejects=self.max_rejects)

    def run(self, poses, cov):
        import torch
        lib = _lib.load()
        host = not isinstance(poses, torch.Tensor)
        if host:
            poses = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float32)).cuda()
            cov = torch.from_numpy(np.ascontiguousarray(cov, dtype=np.float32)).to(poses.device)
        if not (isinstance(cov, torch.Tensor) and poses.is_cuda and cov.is_cuda and poses.dtype == torch.float32
                and cov.dtype == torch.float32):
            raise TypeError('poses and cov must both be float32 on a CUDA (HIP) device')
        lead = tuple(poses.shape[:-2])
        if len(lead) not in (1, 2) or tuple(poses.shape[-2:]) != (4, 4) or tuple(cov.shape) != lead + (6, 6):
            raise ValueError('poses must be [T,4,4] or [S,T,4,4] and cov [..,6,6] alike, got %s and %s'
                             % (tuple(poses.shape), tuple(cov.shape)))
        S, T = (1, lead[0]) if len(lead) == 1 else lead
        if S * T <= 0:
            raise ValueError('empty sequence')
        poses, cov = poses.contiguous(), cov.contiguous()
        out_poses, out_cov = torch.empty_like(poses), torch.empty_like(cov)
        flags = torch.empty(lead, dtype=torch.int32, device=poses.device)
        nis = torch.empty(lead, dtype=torch.float32, device=poses.device)
        d = self.desc(S, T)
        _lib.check(lib.kfn_pose_filter(C.byref(d), poses.data_ptr(), cov.data_ptr(), out_poses.data_ptr(), out_cov.data_ptr(),
                                       flags.data_ptr(), nis.data_ptr(), torch.cuda.current_stream(poses.device).cuda_stream),
                   'kfn_pose_filter')
        if host:
            return out_poses.cpu().numpy(), out_cov.cpu().numpy(), flags.cpu().numpy(), nis.cpu().numpy()
        return out_poses, out_cov, flags, nis


MODELS = {'walk': _lib.POSE_MODEL_WALK, 'velocity': _lib.POSE_MODEL_VELOCITY}
DEFAULT_SIGMA = {'walk': 0.02, 'velocity': 0.005}     # rot_sigma = trans_sigma: per-frame walk / white acceleration


class PoseTracker(object):
    """kfn_pose_track (DESIGN.md 5c "Pose tracker"): PoseFilter's recursion under a motion model -- 'walk', PoseFilter's
    own, or 'velocity', whose state also carries a body-frame twist per frame --, with `smooth` a backward
    (Rauch-Tung-Striebel) pass over the frames of each call, and a state that is carried from call to call until reset().

    run(poses, cov) takes PoseFilter.run's arguments and returns (poses, cov, flags, nis) and, with `smooth`,
    (.., smooth_poses, smooth_cov).  rot_sigma / trans_sigma default to the model's (0.02 for the walk, 0.005 for the
    velocity model, where they are the white acceleration per frame); rot_rate_sigma / trans_rate_sigma are the sigma of
    the unknown twist at a (re-)initialisation.  The number of sequences must not change between calls."""

    def __init__(self, model='walk', smooth=False, rot_sigma=None, trans_sigma=None, rot_rate_sigma=0.05,
                 trans_rate_sigma=0.05, gate=22.46, max_rejects=3):
        if model not in MODELS:
            raise ValueError("model must be 'walk' or 'velocity', got %r" % (model,))
        rot_sigma = DEFAULT_SIGMA[model] if rot_sigma is None else rot_sigma
        trans_sigma = DEFAULT_SIGMA[model] if trans_sigma is None else trans_sigma
        if not (float(rot_sigma) >= 0.0 and float(trans_sigma) >= 0.0):
            raise ValueError('rot_sigma and trans_sigma must be >= 0')
        if model == 'velocity' and not (float(rot_rate_sigma) > 0.0 and float(trans_rate_sigma) > 0.0):
            raise ValueError('rot_rate_sigma and trans_rate_sigma must be > 0')
        if not float(gate) > 0.0:
            raise ValueError('gate must be > 0')
        if int(max_rejects) < 1:
            raise ValueError('max_rejects must be >= 1')
        self.model, self.smooth = model, bool(smooth)
        self.rot_sigma, self.trans_sigma, self.gate = float(rot_sigma), float(trans_sigma), float(gate)
        self.rot_rate_sigma, self.trans_rate_sigma = float(rot_rate_sigma), float(trans_rate_sigma)
        self.max_rejects = int(max_rejects)
        self.reset()

    def reset(self):
        """Forget the carried state: the next run() starts without an estimate (and may have another S)."""
        self._state, self._S = None, None

    def desc(self, S, T):
        return _lib.PoseTrackDesc(S=S, T=T, model=MODELS[self.model], smooth=int(self.smooth), rot_sigma=self.rot_sigma,
                                  trans_sigma=self.trans_sigma, rot_rate_sigma=self.rot_rate_sigma,
                                  trans_rate_sigma=self.trans_rate_sigma, gate=self.gate, max_rejects=self.max_rejects)

    def run(self, poses, cov):
        import torch
        lib = _lib.load()
        host = not isinstance(poses, torch.Tensor)
        if host:
            poses = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float32)).cuda()
            cov = torch.from_numpy(np.ascontiguousarray(cov, dtype=np.float32)).to(poses.device)
        if not (isinstance(cov, torch.Tensor) and poses.is_cuda and cov.is_cuda and poses.dtype == torch.float32
                and cov.dtype == torch.float32):
            raise TypeError('poses and cov must both be float32 on a CUDA (HIP) device')
        lead = tuple(poses.shape[:-2])
        if len(lead) not in (1, 2) or tuple(poses.shape[-2:]) != (4, 4) or tuple(cov.shape) != lead + (6, 6):
            raise ValueError('poses must be [T,4,4] or [S,T,4,4] and cov [..,6,6] alike, got %s and %s'
                             % (tuple(poses.shape), tuple(cov.shape)))
        S, T = (1, lead[0]) if len(lead) == 1 else lead
        if S * T <= 0:
            raise ValueError('empty sequence')
        if self._S is not None and S != self._S:
            raise ValueError('the carried state holds %d sequences, this call has %d: reset() first' % (self._S, S))
        d = self.desc(S, T)
        dev = poses.device
        if self._state is not None and self._state.device != dev:
            raise ValueError('the carried state is on %s, this call on %s: reset() first' % (self._state.device, dev))
        if self._state is None:
            n = C.c_size_t()
            _lib.check(lib.kfn_pose_track_state_bytes(C.byref(d), C.byref(n)), 'kfn_pose_track_state_bytes')
            self._state, self._S = torch.zeros(n.value // 8, dtype=torch.float64, device=dev), S
        poses, cov = poses.contiguous(), cov.contiguous()
        out = [torch.empty_like(poses), torch.empty_like(cov), torch.empty(lead, dtype=torch.int32, device=dev),
               torch.empty(lead, dtype=torch.float32, device=dev)]
        smooth_ptrs, scratch = (None, None), None
        if self.smooth:
            n = C.c_size_t()
            _lib.check(lib.kfn_pose_track_scratch_bytes(C.byref(d), C.byref(n)), 'kfn_pose_track_scratch_bytes')
            scratch = torch.empty(n.value // 8, dtype=torch.float64, device=dev)
            out += [torch.empty_like(poses), torch.empty_like(cov)]
            smooth_ptrs = (out[4].data_ptr(), out[5].data_ptr())
        _lib.check(lib.kfn_pose_track(C.byref(d), poses.data_ptr(), cov.data_ptr(), self._state.data_ptr(), out[0].data_ptr(),
                                      out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), smooth_ptrs[0], smooth_ptrs[1],
                                      scratch.data_ptr() if scratch is not None else None,
                                      torch.cuda.current_stream(dev).cuda_stream), 'kfn_pose_track')
        if host:
            return tuple(x.cpu().numpy() for x in out)
        return tuple(out)
