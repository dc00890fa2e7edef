"""The reference's reprojection loss (KFNet.ReprojectionLoss, KFNet/KFNet.py:405-428) for the trainers of stages 1 and 3:
the host side of kfn_reproj_loss_grad.  DESIGN.md 6i holds the definitions.

    M = pose_matrices(poses, transform)           [B,12] float32: the rows of P_b G^-1, fp64 rounded once
    term = ReprojTerm(B, h, w, camera, transform, device)
    term.set_poses(poses); term.launch(outputs, labels, label_stride, pixel_map, nll_stats, valid_index, stream)

The launch ADDS weight * dR/dx into channels 0..2 of each output's gradient buffer, so it goes behind the NLL launch of the
same step and in front of whatever reads those buffers.  There is no fallback: a missing entry point raises.
"""
import ctypes as C

import numpy as np

from . import _lib

STAGE1_WEIGHT = 50.0                      # MeasureCoordLoss, KFNet/KFNet.py:246-248
STAGE3_WEIGHTS = (50.0, 10.0, 10.0)       # measure (:246-248), temporal (:270-272), KF (:292-294)
POSE_LIST = 'pose_list.txt'


def check_weights(weights, count):
    """`count` finite, non-negative numbers as a tuple of floats, or ValueError."""
    w = tuple(float(x) for x in (weights if np.ndim(weights) else (weights,)))
    if len(w) != count:
        raise ValueError('expected %d reprojection weight%s, got %d' % (count, 's' if count > 1 else '', len(w)))
    if not all(np.isfinite(x) and x >= 0.0 for x in w):
        raise ValueError('a reprojection weight must be a finite number >= 0, got %r' % (w,))
    return w


def pose_matrices(poses, transform=None):
    """poses [B,4,4] camera to world, transform = the 4x4 G by which the loss launches map the labels (None: identity) ->
    float32 [B,12], the first three rows of M_b = P_b G^-1 with P_b = inv(pose_b): the training loss asks the prediction to
    equal G [X_world; 1], so M_b takes it to frame b's camera.  fp64 throughout, each entry rounded once."""
    p = np.asarray(poses, dtype=np.float64)
    if p.ndim != 3 or p.shape[1:] != (4, 4):
        raise ValueError('poses must be [B,4,4] camera-to-world matrices, got %s' % (np.shape(poses),))
    G = np.eye(4) if transform is None else np.asarray(transform, dtype=np.float64).reshape(4, 4)
    Gi = np.linalg.inv(G)
    M = np.stack([np.linalg.inv(q) @ Gi for q in p])
    return np.ascontiguousarray(M[:, :3, :].reshape(len(p), 12), dtype=np.float32)


def camera_constants(camera):
    """(u, v, inv_fx, inv_fy) of a kfnet_amd.labels.DepthCamera as Python floats: ctypes rounds each to fp32 once, as
    DepthCamera.descriptor does."""
    return camera.u, camera.v, 1.0 / camera.fx, 1.0 / camera.fy


def descriptor(camera, B, h, w, label_stride, outputs):
    """kfn_reproj_desc; outputs = [(x_ptr, ld_x, dx_ptr, ld_dx, weight), ...], one to three."""
    d = _lib.ReprojDesc(B=B, h=h, w=w, label_stride=label_stride, outputs=len(outputs))
    d.u, d.v, d.inv_fx, d.inv_fy = camera_constants(camera)
    for o, (x, ld_x, dx, ld_dx, weight) in enumerate(outputs[:_lib.REPROJ_MAX_OUTPUTS]):
        d.out[o] = _lib.ReprojOutput(x=x, dx=dx, weight=weight, ld_x=ld_x, ld_dx=ld_dx)
    return d


class ReprojTerm(object):
    """kfn_reproj_loss_grad with its buffers for a batch of B frames on an h x w grid: M [B,12] and stats [8] =
    (R per output, the weighted sum added to the loss, valid + 1, 0, 0, 0) on the device."""

    def __init__(self, B, h, w, camera=None, transform=None, device='cuda:0'):
        import torch
        from .labels import DepthCamera
        self.lib, self.torch, self.device = _lib.load(), torch, torch.device(device)
        self.shape = (B, h, w)
        self.camera = DepthCamera() if camera is None else camera
        self.transform = transform
        with torch.cuda.device(self.device):
            self.M = torch.zeros((B, 12), dtype=torch.float32, device=self.device)
            self.stats = torch.zeros(8, dtype=torch.float32, device=self.device)

    def set_poses(self, poses):
        if poses is None:
            raise ValueError('the reprojection term needs the camera-to-world poses of the batch (poses=None)')
        if self.torch.is_tensor(poses):
            poses = poses.detach().cpu().numpy()
        M = pose_matrices(poses, self.transform)
        if M.shape[0] != self.shape[0]:
            raise ValueError('%d poses for a batch of %d frames' % (M.shape[0], self.shape[0]))
        self.M.copy_(self.torch.from_numpy(M), non_blocking=True)

    def launch(self, outputs, labels, label_stride, pixel_map, nll_stats, valid_index, stream):
        """outputs: [(x tensor, dx tensor, weight), ...] of [B,h,w,ld] float32 device tensors."""
        B, h, w = self.shape
        d = descriptor(self.camera, B, h, w, label_stride,
                       [(x.data_ptr(), x.shape[3], dx.data_ptr(), dx.shape[3], wgt) for x, dx, wgt in outputs])
        _lib.check(self.lib.kfn_reproj_loss_grad(C.byref(d), self.M.data_ptr(), labels.data_ptr(),
                                                 None if pixel_map is None else pixel_map.data_ptr(), nll_stats.data_ptr(),
                                                 valid_index, self.stats.data_ptr(), stream), 'kfn_reproj_loss_grad')


def read_pose_list(input_folder):
    """The camera-to-world poses [count,4,4] that pose_list.txt of an input folder names (`labels make` writes it next to the
    label files).  ValueError, naming the file, when it is missing."""
    import os
    from .labels import read_lines, read_poses
    path = os.path.join(input_folder, POSE_LIST)
    if not os.path.exists(path):
        raise ValueError('%s has no %s: --reproj needs the poses (`python -m kfnet_amd.labels make` writes the list)'
                         % (input_folder, POSE_LIST))
    return read_poses([x for x in read_lines(path) if x])
