"""Camera poses from the scene-coordinate maps and a depth frame: batched RANSAC-Kabsch on the device (kfn_kabsch_ransac).

The sibling of KFNet.pnp.PnPSolver for RGB-D frames (DESIGN.md 5c "Poses with depth").  With the depth frame of the same
image, every confident cell of a record is a 3-D/3-D correspondence -- the network's scene point and the back-projected
camera point of pixel (8c, 8r) -- and the pose is a rigid alignment: three points per hypothesis, a closed-form refinement
weighted by the maps' own sigma, no ambiguity along the viewing ray.  The camera points are what kfn_depth_labels writes at
stride 8 under the identity pose (kfnet_amd.labels.DepthLabeler, registration of unregistered depth included); there is no
second back-projection.  `KFNet.pnp --depth_list` is the program.  There is no fallback: a missing entry point raises.
"""
import ctypes as C

import numpy as np

from .. import _lib
from ..labels import DepthCamera, DepthLabeler

IDENTITY_ROWS = (1., 0., 0., 0., 0., 1., 0., 0., 0., 0., 1., 0.)


class KabschSolver(object):
    """RANSAC-Kabsch over [B,h,w,>=4] records (x, y, z, 1/sigma) of an h x w grid and the frames' depth.  `depth` is either
    the uint16 depth maps [B,8h,8w] (back-projected here with `camera`, a labels.DepthCamera) or ready camera points
    [B,h,w,>=4] float32 = (Xc, Yc, Zc, mask).  `solve` returns camera-to-world poses [B,4,4] (NaN on failure) and info
    [B,4] = (status, candidates, final inliers, best hypothesis); `solve_unc` also every pose's 6x6 covariance, in
    PnPSolver.solve_unc's coordinates, and (weighted cost, 3 * inliers - 6).  numpy in, numpy out; CUDA tensors in, tensors
    out (no sync).  `weighted` weighs the refinement by 1 / (sigma^2 + point_sigma^2); `inlier_m` is the inlier distance in
    metres."""

    def __init__(self, h, w, camera=None, hypotheses=256, refine_iters=10, min_points=16, seed=0, min_confidence=20.,
                 inlier_m=0.10, weighted=False, point_sigma=0.01):
        if not 1 <= int(hypotheses) <= _lib.PNP_MAX_HYPOTHESES:
            raise ValueError('hypotheses must be in 1..%d' % _lib.PNP_MAX_HYPOTHESES)
        if not float(point_sigma) > 0.0:
            raise ValueError('point_sigma must be > 0')
        if not float(inlier_m) > 0.0:
            raise ValueError('inlier_m must be > 0')
        if not float(np.float32(min_confidence)) >= 0.0:
            raise ValueError('min_confidence must be >= 0')
        if int(min_points) < 3:
            raise ValueError('min_points must be >= 3')
        self.h, self.w = int(h), int(w)
        self.camera = DepthCamera() if camera is None else camera
        self.hypotheses, self.refine_iters, self.min_points = int(hypotheses), int(refine_iters), int(min_points)
        self.seed, self.min_confidence, self.inlier_m = int(seed) & 0xFFFFFFFF, float(min_confidence), float(inlier_m)
        self.weighted, self.point_sigma = bool(weighted), float(point_sigma)
        self._scratch = None
        self._labeler = None

    def desc(self, B, t0=0, ld=4, ldp=4):
        return _lib.KabschDesc(B=B, h=self.h, w=self.w, ld=ld, ldp=ldp, t0=t0, seed=self.seed, hypotheses=self.hypotheses,
                               refine_iters=self.refine_iters, min_points=self.min_points,
                               min_confidence=self.min_confidence, inlier_m=self.inlier_m, weighted=int(self.weighted),
                               point_sigma=self.point_sigma)

    def _scratch_for(self, lib, d, device):
        import torch
        nbytes = C.c_size_t()
        _lib.check(lib.kfn_kabsch_scratch_bytes(C.byref(d), C.byref(nbytes)), 'kfn_kabsch_scratch_bytes')
        if self._scratch is None or self._scratch.numel() < nbytes.value or self._scratch.device != device:
            self._scratch = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=device)
        return self._scratch

    def _device_records(self, records):
        import torch
        host = not isinstance(records, torch.Tensor)
        if host:
            records = torch.from_numpy(np.ascontiguousarray(records, dtype=np.float32)).cuda()
        if records.dtype != torch.float32 or not records.is_cuda:
            raise TypeError('records must be float32 on a CUDA (HIP) device')
        if records.dim() != 4 or tuple(records.shape[1:3]) != (self.h, self.w) or records.shape[3] < 4:
            raise ValueError('records must be [B,%d,%d,>=4], got %s' % (self.h, self.w, tuple(records.shape)))
        return records.contiguous(), host

    def cam_points(self, depth, device=None):
        """uint16 depth maps [B,8h,8w] (numpy or tensor) -> the device tensor [B,h,w,4] = (Xc, Yc, Zc, mask) of
        kfn_depth_labels at stride 8 under the identity pose; the next call overwrites it."""
        import torch
        B = int(depth.shape[0]) if len(depth.shape) == 3 else -1
        if B < 1 or tuple(depth.shape[1:]) != (8 * self.h, 8 * self.w):
            raise ValueError('depth maps must be uint16 [B,%d,%d], got %s' % (8 * self.h, 8 * self.w, tuple(depth.shape)))
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else device
        lab = self._labeler
        if lab is None or lab.shape[0] < B or lab.device != device:
            lab = self._labeler = DepthLabeler(B, 8 * self.h, 8 * self.w, 8, self.camera, device)
            self._identity = torch.tensor(IDENTITY_ROWS, dtype=torch.float32, device=device).repeat(B, 1)
        return lab.labels(depth, self._identity[:B])

    def _device_points(self, depth, rec):
        import torch
        if depth is None:
            raise ValueError('KabschSolver needs the depth maps or the camera points of the frames')
        # four dimensions: camera points (a host array of any float type is rounded to float32 once); three: depth maps
        if len(depth.shape) != 4:
            cam = self.cam_points(depth, rec.device)
        else:
            if isinstance(depth, torch.Tensor):
                cam = depth
            else:
                if np.asarray(depth).dtype.kind != 'f':
                    raise ValueError('camera points [B,h,w,>=4] must be floating point, got %s' % np.asarray(depth).dtype)
                cam = torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)).to(rec.device)
            if (cam.dtype != torch.float32 or not cam.is_cuda or tuple(cam.shape[1:3]) != (self.h, self.w)
                    or cam.shape[3] < 4):
                raise ValueError('camera points must be float32 [B,%d,%d,>=4] on the device, got %s'
                                 % (self.h, self.w, tuple(cam.shape)))
            cam = cam.contiguous()
        if cam.shape[0] != rec.shape[0]:
            raise ValueError('%d depth frames for %d records' % (cam.shape[0], rec.shape[0]))
        return cam

    def _ransac(self, records, depth, t0, with_cov):
        import torch
        lib = _lib.load()
        rec, host = self._device_records(records)
        cam = self._device_points(depth, rec)
        B = rec.shape[0]
        d = self.desc(B, t0, rec.shape[3], cam.shape[3])
        scratch = self._scratch_for(lib, d, rec.device)
        poses = torch.empty((B, 4, 4), dtype=torch.float32, device=rec.device)
        info = torch.empty((B, 4), dtype=torch.int32, device=rec.device)
        cov = torch.empty((B, 6, 6), dtype=torch.float32, device=rec.device) if with_cov else None
        quality = torch.empty((B, 2), dtype=torch.float32, device=rec.device) if with_cov else None
        stream = torch.cuda.current_stream(rec.device).cuda_stream
        _lib.check(lib.kfn_kabsch_ransac(C.byref(d), rec.data_ptr(), cam.data_ptr(), poses.data_ptr(),
                                         cov.data_ptr() if with_cov else None, quality.data_ptr() if with_cov else None,
                                         info.data_ptr(), scratch.data_ptr(), stream), 'kfn_kabsch_ransac')
        out = (poses, cov, quality, info) if with_cov else (poses, info)
        return tuple(x.cpu().numpy() for x in out) if host else out

    def solve(self, records, depth=None, t0=0):
        return self._ransac(records, depth, t0, False)

    def solve_unc(self, records, depth=None, t0=0):
        """(poses [B,4,4], cov [B,6,6], quality [B,2] = (weighted cost, 3 * inliers - 6), info [B,4]); poses and info are
        `solve`'s bit for bit.  cov is NaN where there is no pose."""
        return self._ransac(records, depth, t0, True)

    def hypotheses_probe(self, records, depth=None, t0=0):
        """kfn_kabsch_hypotheses: (samples [B,H,3], hypothesis poses [B,H,12] = [R | t] camera-to-world, counts [B,H]) as
        numpy arrays -- the sampled and scored hypotheses before selection."""
        import torch
        lib = _lib.load()
        rec, _ = self._device_records(records)
        cam = self._device_points(depth, rec)
        B, H = rec.shape[0], self.hypotheses
        d = self.desc(B, t0, rec.shape[3], cam.shape[3])
        samples = torch.empty((B, H, 3), dtype=torch.int32, device=rec.device)
        hp = torch.empty((B, H, 12), dtype=torch.float32, device=rec.device)
        counts = torch.empty((B, H), dtype=torch.int32, device=rec.device)
        stream = torch.cuda.current_stream(rec.device).cuda_stream
        _lib.check(lib.kfn_kabsch_hypotheses(C.byref(d), rec.data_ptr(), cam.data_ptr(), samples.data_ptr(), hp.data_ptr(),
                                             counts.data_ptr(), stream), 'kfn_kabsch_hypotheses')
        return samples.cpu().numpy(), hp.cpu().numpy(), counts.cpu().numpy()


def select_probe(counts):
    """kfn_kabsch_select: counts [B,H] int32 (numpy) -> best [B], the first index of each row's maximum, -1 where every
    count is negative."""
    import torch
    lib = _lib.load()
    c = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda()
    best = torch.empty((c.shape[0],), dtype=torch.int32, device=c.device)
    _lib.check(lib.kfn_kabsch_select(c.data_ptr(), c.shape[0], c.shape[1], best.data_ptr(),
                                     torch.cuda.current_stream(c.device).cuda_stream), 'kfn_kabsch_select')
    return best.cpu().numpy()
