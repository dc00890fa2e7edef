"""Training labels from depth maps and camera poses, on the device.

What a user has is an RGB-D sequence in the 7-Scenes layout: frame-XXXXXX.color.png, a 16-bit frame-XXXXXX.depth.png in
millimetres and a 4x4 camera-to-world frame-XXXXXX.pose.txt.  What stage 1 of the training reads is one [H,W,4] float32
scene-coordinate-and-mask file per image and transform.txt, the Euclidean transformation that decorrelates the scene's
point cloud.  This module makes the second from the first:

    python -m kfnet_amd.labels make --sequence S [--sequence S2 ...] --output_folder I [--no_labels]
                                    [--focal_x 525 --focal_y 525 --u 320 --v 240]
                                    [--depth_focal_x F --depth_focal_y F --depth_u U --depth_v V]
                                    [--height 480 --width 640] [--batch 16] [--gpu 0]

writes image_list.txt, depth_list.txt, pose_list.txt (absolute paths; pose_list.txt is the --gt list of KFNet.pnp and of
eval --pose), transform.txt and, unless --no_labels, labels/label_<i>.bin with label_list.txt.  `SCoordNet.train --depth`
needs only the three lists and transform.txt: it makes every batch's labels from the depth maps.

    cam = DepthCamera(525, 525, 320, 240)                 the one place where the fp64 -> fp32 constants are derived
    lab = DepthLabeler(B, H, W, stride, cam)              kfn_depth_labels / kfn_label_moments with their buffers
    M = decorrelating_transform(moments_total, pivot)     transform.txt from the ten fp64 sums

Any of the depth_* arguments switches registration on: 7-Scenes' depth maps are not registered to the colour images (same
centre and orientation, other intrinsics).  There is no fallback: a missing entry point or an unsupported shape raises.
"""
import argparse
import ctypes as C
import glob
import os
import sys

import numpy as np

from . import _lib
from .staging import check_size, current_stream
from .tools.io import read_lines

LISTS = ('image_list.txt', 'depth_list.txt', 'pose_list.txt')


class DepthCamera(object):
    """The colour camera (fx, fy, u, v: the pixel grid of the labels), optionally the depth camera's intrinsics (any of
    depth_fx, depth_fy, depth_u, depth_v given: the others default to the colour camera's), the raw-to-metres `scale` and
    the validity window raw_min <= raw <= raw_max."""

    def __init__(self, fx=525., fy=525., u=320., v=240., depth_fx=None, depth_fy=None, depth_u=None, depth_v=None,
                 scale=0.001, raw_min=1, raw_max=65534):
        self.fx, self.fy, self.u, self.v = float(fx), float(fy), float(u), float(v)
        if not (self.fx > 0.0 and self.fy > 0.0):
            raise ValueError('focal lengths must be positive, got %r, %r' % (fx, fy))
        self.register = any(x is not None for x in (depth_fx, depth_fy, depth_u, depth_v))
        self.depth_fx = self.fx if depth_fx is None else float(depth_fx)
        self.depth_fy = self.fy if depth_fy is None else float(depth_fy)
        self.depth_u = self.u if depth_u is None else float(depth_u)
        self.depth_v = self.v if depth_v is None else float(depth_v)
        if not (self.depth_fx > 0.0 and self.depth_fy > 0.0):
            raise ValueError('depth focal lengths must be positive, got %r, %r' % (depth_fx, depth_fy))
        self.scale, self.raw_min, self.raw_max = float(scale), int(raw_min), int(raw_max)
        if not 0 <= self.raw_min <= self.raw_max <= 65535:
            raise ValueError('the validity window must lie in 0..65535, got [%d, %d]' % (self.raw_min, self.raw_max))

    def descriptor(self, B, H, W, stride, ld_out=4):
        """kfn_depth_labels_desc for a batch [B,H,W]: every derived constant in fp64, rounded to fp32 once (ctypes does the
        rounding)."""
        d = _lib.DepthLabelsDesc(B=B, H=H, W=W, stride=stride, ld_out=ld_out, registration=int(self.register),
                                 raw_min=self.raw_min, raw_max=self.raw_max)
        d.u, d.v = self.u, self.v
        d.inv_fx, d.inv_fy = 1.0 / self.fx, 1.0 / self.fy
        d.kx, d.ky = self.depth_fx / self.fx, self.depth_fy / self.fy
        d.ud, d.vd = self.depth_u, self.depth_v
        d.scale = self.scale
        return d


def pose_rows(poses):
    """Camera-to-world poses [B,4,4], [B,3,4] or [B,12] -> the twelve floats [R|t] per frame, float32 [B,12]: each fp64
    entry rounded once."""
    p = np.asarray(poses, dtype=np.float64)
    if p.ndim == 3 and p.shape[1:] in ((4, 4), (3, 4)):
        p = p[:, :3, :].reshape(p.shape[0], 12)
    if p.ndim != 2 or p.shape[1] != 12:
        raise ValueError('poses must be [B,4,4], [B,3,4] or [B,12], got %s' % (np.shape(poses),))
    return np.ascontiguousarray(p, dtype=np.float32)


class DepthLabeler(object):
    """kfn_depth_labels and kfn_label_moments with their buffers.  labels(depth, poses) takes uint16 depth maps [n,H,W]
    and poses of n <= batch frames (numpy arrays or tensors) and returns the device tensor [n,H/stride,W/stride,4] that
    the next call overwrites; nothing waits for the device."""

    def __init__(self, batch, H, W, stride=8, camera=None, device='cuda:0'):
        import torch
        if batch < 1:
            raise ValueError('batch must be >= 1')
        check_size(H, W, 'the height and width of depth labels')
        if stride not in (1, 8):
            raise ValueError('stride must be 1 or 8')
        self.lib = _lib.load()
        self.torch, self.device = torch, torch.device(device)
        self.shape, self.stride = (batch, H, W), stride
        self.camera = DepthCamera() if camera is None else camera
        with torch.cuda.device(self.device):
            self.depth = torch.zeros((batch, H, W), dtype=torch.int16, device=self.device)     # the uint16 bits
            self.poses = torch.zeros((batch, 12), dtype=torch.float32, device=self.device)
            self.out = torch.zeros((batch, H // stride, W // stride, 4), dtype=torch.float32, device=self.device)

    def labels(self, depth_u16, poses):
        torch = self.torch
        B, H, W = self.shape
        if torch.is_tensor(depth_u16):
            dp = depth_u16
            if dp.dtype not in (torch.int16, torch.uint16):
                raise ValueError('depth must be uint16 (or its bits as int16), got %s' % dp.dtype)
            dp = dp.contiguous().view(torch.int16)
        else:
            dp = np.ascontiguousarray(depth_u16)
            if dp.dtype != np.uint16:
                raise ValueError('depth must be uint16, got %s' % dp.dtype)
            dp = torch.from_numpy(dp.view(np.int16))
        n = dp.shape[0] if dp.dim() == 3 else -1
        if not 1 <= n <= B or tuple(dp.shape[1:]) != (H, W):
            raise ValueError('depth must be uint16 [1..%d,%d,%d], got %s' % (B, H, W, tuple(dp.shape)))
        if torch.is_tensor(poses) and poses.dtype == torch.float32 and tuple(poses.shape) == (n, 12):
            ps = poses
        else:
            ps = torch.from_numpy(pose_rows(poses.cpu().numpy() if torch.is_tensor(poses) else poses))
        if ps.shape[0] != n:
            raise ValueError('%d poses for %d depth maps' % (ps.shape[0], n))
        with torch.cuda.device(self.device):
            self.depth[:n].copy_(dp, non_blocking=True)
            self.poses[:n].copy_(ps, non_blocking=True)
            d = self.camera.descriptor(n, H, W, self.stride)
            _lib.check(self.lib.kfn_depth_labels(C.byref(d), self.depth.data_ptr(), self.poses.data_ptr(), self.out.data_ptr(),
                                                 current_stream(self.device)), 'kfn_depth_labels')
        return self.out[:n]

    def moments(self, labels, pivot):
        """The [n,10] fp64 partial sums of kfn_label_moments over a device tensor of labels [n,h,w,>=4], about `pivot`."""
        torch = self.torch
        if not (torch.is_tensor(labels) and labels.is_cuda and labels.dtype == torch.float32 and labels.dim() == 4
                and labels.shape[3] >= 4):
            raise ValueError('labels must be a float32 device tensor [n,h,w,>=4]')
        labels = labels.contiguous()
        n, h, w, ld = labels.shape
        d = _lib.LabelMomentsDesc(B=n, h=h, w=w, ld=ld)
        d.pivot = (C.c_double * 3)(*[float(x) for x in pivot])
        with torch.cuda.device(self.device):
            partial = torch.zeros((n, 10), dtype=torch.float64, device=self.device)
            _lib.check(self.lib.kfn_label_moments(C.byref(d), labels.data_ptr(), partial.data_ptr(),
                                                  current_stream(self.device)), 'kfn_label_moments')
        return partial


def add_frames(total, partial):
    """Adds the frames of a [n,10] partial to the running total in index order (a fixed order: a fixed result)."""
    total = np.zeros(10, dtype=np.float64) if total is None else total
    for row in np.asarray(partial, dtype=np.float64):
        total = total + row
    return total


def decorrelating_transform(moments_total, pivot):
    """transform.txt from the ten sums (n, sum d, upper triangle of sum d d^T, d = p - pivot) over all valid label points:
    the 4x4 fp64 M = [R | -R mu; 0 0 0 1] with mu the mean, the rows of R the eigenvectors of the covariance by descending
    eigenvalue, each with its largest-magnitude component positive, the third negated if that leaves det R < 0."""
    m = np.asarray(moments_total, dtype=np.float64).reshape(10)
    pivot = np.asarray(pivot, dtype=np.float64).reshape(3)
    n = m[0]
    if not n >= 3:
        raise ValueError('the transform needs at least 3 valid label points, got %d' % int(n))
    md = m[1:4] / n
    S = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]], dtype=np.float64)
    cov = S / n - np.outer(md, md)
    lam, V = np.linalg.eigh(cov)
    R = V[:, np.argsort(-lam, kind='stable')].T.copy()
    for row in R:
        if row[np.argmax(np.abs(row))] < 0.0:
            row *= -1.0
    if np.linalg.det(R) < 0.0:
        R[2] *= -1.0
    M = np.eye(4, dtype=np.float64)
    M[:3, :3] = R
    M[:3, 3] = -R.dot(pivot + md)
    return M


def write_transform(path, M):
    with open(path, 'w') as f:
        for row in np.asarray(M, dtype=np.float64).reshape(4, 4):
            f.write(' '.join('%.9e' % x for x in row) + '\n')


def _decode_depth_pil(path, size):
    try:
        from PIL import Image
    except ImportError:
        raise ValueError('%s is not a non-interlaced 16-bit gray PNG and PIL is not there to decode it' % path)
    try:
        with Image.open(path) as im:
            if im.mode not in ('I;16', 'I;16B', 'I;16L', 'I', 'L'):
                raise ValueError('%s: a depth map must be a single-channel image, got mode %s' % (path, im.mode))
            a = np.asarray(im)
    except ValueError:
        raise
    except Exception as e:      # PIL's own error types: one type for the caller
        raise ValueError('%s: %s' % (path, e))
    if a.shape != tuple(size):
        raise ValueError('%s is %s, expected %dx%d' % (path, 'x'.join(str(x) for x in a.shape), size[0], size[1]))
    if a.min() < 0 or a.max() > 65535:
        raise ValueError('%s: depth values outside 0..65535' % path)
    return a.astype(np.uint16)


def load_depth(paths, size, workers=None):
    """16-bit depth PNGs -> uint16 [n,H,W] on the library's threads (kfn_decode_png_gray16); files it reports unsupported
    go through PIL.  A broken file raises ValueError naming it."""
    lib = _lib.load()
    H, W = size
    n = len(paths)
    out = np.zeros((n, H, W), dtype=np.uint16)
    if n == 0:
        return out
    arr = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
    status = (C.c_int * n)()
    if workers is None:
        workers = max(4, min(32, (os.cpu_count() or 8) // 2))
    rc = lib.kfn_decode_png_gray16(arr, n, H, W, out.ctypes.data, status, int(workers))
    if rc != 0:
        raise ValueError(lib.kfn_last_error().decode())
    for i in range(n):
        if status[i] == _lib.PNG_UNSUPPORTED:
            out[i] = _decode_depth_pil(paths[i], size)
    return out


def read_sequence(folder):
    """The sorted (colour, depth, pose) path triples of a 7-Scenes sequence folder (frame-*.color.png, frame-*.depth.png,
    frame-*.pose.txt), or of a folder holding image_list.txt, depth_list.txt and pose_list.txt.  ValueError, naming it, when
    the counts differ or a member is missing."""
    if not os.path.isdir(folder):
        raise ValueError('%s is not a folder' % folder)
    if os.path.exists(os.path.join(folder, LISTS[0])):
        cols = []
        for name in LISTS:
            p = os.path.join(folder, name)
            if not os.path.exists(p):
                raise ValueError('%s is missing' % p)
            cols.append([x for x in read_lines(p) if x])
        for name, col in zip(LISTS[1:], cols[1:]):
            if len(col) != len(cols[0]):
                raise ValueError('%s lists %d files for the %d images of %s' %
                                 (os.path.join(folder, name), len(col), len(cols[0]), os.path.join(folder, LISTS[0])))
        triples = list(zip(*cols))
    else:
        colour = sorted(glob.glob(os.path.join(glob.escape(folder), 'frame-*.color.png')))
        depth = sorted(glob.glob(os.path.join(glob.escape(folder), 'frame-*.depth.png')))
        pose = sorted(glob.glob(os.path.join(glob.escape(folder), 'frame-*.pose.txt')))
        if not colour:
            raise ValueError('%s holds no frame-*.color.png and no %s' % (folder, LISTS[0]))
        triples = [(c, c[:-len('color.png')] + 'depth.png', c[:-len('color.png')] + 'pose.txt') for c in colour]
        for t in triples:
            for p in t:
                if not os.path.exists(p):
                    raise ValueError('%s is missing' % p)
        if len(depth) != len(colour) or len(pose) != len(colour):      # a depth map or pose without its colour image
            raise ValueError('%s holds %d colour images, %d depth maps and %d poses' % (folder, len(colour), len(depth), len(pose)))
    for t in triples:
        for p in t:
            if not os.path.exists(p):
                raise ValueError('%s is missing' % p)
    return triples


def read_frames(folder):
    """The sorted (colour, depth) path pairs of a folder of frame-*.color.png and frame-*.depth.png, with or without pose
    files (`kfnet_amd.track make` finds the poses).  ValueError, naming it, when there is no depth map or a member is missing."""
    if not os.path.isdir(folder):
        raise ValueError('%s is not a folder' % folder)
    depth = sorted(glob.glob(os.path.join(glob.escape(folder), 'frame-*.depth.png')))
    if not depth:
        raise ValueError('%s holds no frame-*.depth.png' % folder)
    pairs = [(d[:-len('depth.png')] + 'color.png', d) for d in depth]
    for colour, _ in pairs:
        if not os.path.exists(colour):
            raise ValueError('%s is missing' % colour)
    colour = glob.glob(os.path.join(glob.escape(folder), 'frame-*.color.png'))
    if len(colour) != len(depth):
        raise ValueError('%s holds %d colour images and %d depth maps' % (folder, len(colour), len(depth)))
    return pairs


def add_camera_flags(ap):
    ap.add_argument('--focal_x', type=float, default=525.)
    ap.add_argument('--focal_y', type=float, default=525.)
    ap.add_argument('--u', type=float, default=320.)
    ap.add_argument('--v', type=float, default=240.)
    ap.add_argument('--depth_focal_x', type=float, default=None, help='any --depth_* flag switches registration on')
    ap.add_argument('--depth_focal_y', type=float, default=None)
    ap.add_argument('--depth_u', type=float, default=None)
    ap.add_argument('--depth_v', type=float, default=None)


def camera_of(a):
    """The DepthCamera of parsed add_camera_flags arguments (ValueError on impossible values)."""
    return DepthCamera(a.focal_x, a.focal_y, a.u, a.v, a.depth_focal_x, a.depth_focal_y, a.depth_u, a.depth_v)


def read_poses(paths):
    from .KFNet.pnp import read_pose
    return np.stack([read_pose(p) for p in paths])


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m kfnet_amd.labels', description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='command')
    mk = sub.add_parser('make', help='lists, transform.txt and label files from RGB-D sequences')
    mk.add_argument('--sequence', action='append', default=[], help='a sequence folder; may be given several times')
    mk.add_argument('--output_folder', default='')
    mk.add_argument('--no_labels', action='store_true', help='write the lists and transform.txt only (for train --depth)')
    add_camera_flags(mk)
    mk.add_argument('--height', type=int, default=480)
    mk.add_argument('--width', type=int, default=640)
    mk.add_argument('--batch', type=int, default=16)
    mk.add_argument('--gpu', type=int, default=0)
    return ap


def make(a):
    if not a.sequence:
        print('labels make: at least one --sequence is required', file=sys.stderr)
        return 1
    if not a.output_folder:
        print('labels make: --output_folder is required', file=sys.stderr)
        return 1
    if a.batch < 1:
        print('--batch must be >= 1', file=sys.stderr)
        return 1
    try:
        check_size(a.height, a.width, '--height and --width')
        camera = camera_of(a)
        triples = []
        for s in a.sequence:
            triples += read_sequence(s)
    except ValueError as e:
        print(e, file=sys.stderr)
        return 1
    triples = [tuple(os.path.abspath(p) for p in t) for t in triples]
    count, size = len(triples), (a.height, a.width)
    label_bytes = 0 if a.no_labels else count * a.height * a.width * 16
    print('%d frames; writing %d bytes to %s (%s)' %
          (count, label_bytes, a.output_folder,
           'lists and transform.txt only' if a.no_labels else '%.1f MB of labels per frame' % (a.height * a.width * 16 / 1e6)),
          flush=True)
    import torch
    if not torch.cuda.is_available():
        print('labels make needs a GPU: the labels are computed on the device', file=sys.stderr)
        return 1
    os.makedirs(a.output_folder, exist_ok=True)
    label_dir = os.path.join(a.output_folder, 'labels')
    if not a.no_labels:
        os.makedirs(label_dir, exist_ok=True)
    device = 'cuda:%d' % a.gpu
    grid = DepthLabeler(a.batch, a.height, a.width, 8, camera, device)
    full = None if a.no_labels else DepthLabeler(a.batch, a.height, a.width, 1, camera, device)
    total, pivot, label_paths = None, None, []
    try:
        for lo in range(0, count, a.batch):
            part = triples[lo:lo + a.batch]
            depth = load_depth([t[1] for t in part], size)
            poses = read_poses([t[2] for t in part])
            if pivot is None:
                pivot = poses[0, :3, 3].copy()          # the first frame's camera centre
            # the transform comes from the pixels the loss reads: stride 8
            total = add_frames(total, grid.moments(grid.labels(depth, poses), pivot).cpu().numpy())
            if full is not None:
                host = full.labels(depth, poses).cpu().numpy()
                for k in range(len(part)):
                    p = os.path.join(label_dir, 'label_%d.bin' % (lo + k))
                    host[k].tofile(p)
                    label_paths.append(os.path.abspath(p))
        M = decorrelating_transform(total, pivot)
    except ValueError as e:
        print(e, file=sys.stderr)
        return 1
    for name, col in zip(LISTS, zip(*triples)):
        with open(os.path.join(a.output_folder, name), 'w') as f:
            f.write(''.join(p + '\n' for p in col))
    write_transform(os.path.join(a.output_folder, 'transform.txt'), M)
    if full is not None:
        with open(os.path.join(a.output_folder, 'label_list.txt'), 'w') as f:
            f.write(''.join(p + '\n' for p in label_paths))
    print('%d valid label points at stride 8; transform.txt%s written to %s' %
          (int(total[0]), '' if a.no_labels else ' and %d label files' % count, a.output_folder))
    return 0


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.command != 'make':
        ap.print_usage(sys.stderr)
        return 1
    return make(a)


if __name__ == '__main__':
    sys.exit(main())
