"""RGB-D sequences fused into a truncated signed distance volume, and the scene mesh extracted from it.

7-Scenes ships colour, raw depth and poses, and no mesh; `kfnet_amd.render make --model` needs one.  This module makes it:
every depth map of a sequence is integrated into a dense volume under its pose, through the depth camera's own intrinsics
(so unregistered depth is handled exactly), and a triangle mesh with vertex colours is extracted by marching tetrahedra, in
the arrays `kfn_render` and `write_ply` take:

    python -m kfnet_amd.fuse make --sequence S [--sequence S2 ...] --output scene.ply [--voxel 0.02] [--trunc T]
                                  [--bounds x0 y0 z0 x1 y1 z1] [--min_weight 2] [--every K] [--no_color]
                                  [--focal_x 525 --focal_y 525 --u 320 --v 240]
                                  [--depth_focal_x F --depth_focal_y F --depth_u U --depth_v V]
                                  [--height 480 --width 640] [--batch 16] [--gpu 0]

The data path then closes: raw sequence -> `fuse make` -> scene.ply -> `render make` -> labels and depth without holes ->
`SCoordNet.train`.

    vol = Volume(dims, origin, voxel, trunc, DepthCamera(...), (H, W), batch, color=True)
    vol.integrate(depth_u16, poses, frames)                n <= batch frames; nothing waits for the device
    vertices, colors, triangles = vol.mesh(min_weight)     numpy arrays; one read of the two totals between count and emit
    lo, hi = bounds_from_sequence(depth_paths, poses, camera, (H, W), pad)

There is no fallback: a missing entry point or an unsupported shape raises.
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _lib
from .labels import DepthCamera, DepthLabeler, add_camera_flags, camera_of, load_depth, pose_rows, read_poses, read_sequence
from .modes import load_images
from .staging import check_size, current_stream

MAX_POINTS = 1 << 31


def fuse_descriptor(camera, dims, origin, voxel, trunc, B=1, H=480, W=640, near=0.05, max_weight=64.0, min_weight=1.0):
    """kfn_fuse_desc: every constant rounded from fp64 to fp32 once (ctypes does the rounding).  The camera's depth_* fields
    are the depth camera, fx, fy, u, v the colour camera."""
    d = _lib.FuseDesc(nx=dims[0], ny=dims[1], nz=dims[2], B=B, H=H, W=W, raw_min=camera.raw_min, raw_max=camera.raw_max)
    d.ox, d.oy, d.oz = origin
    d.voxel, d.trunc, d.near, d.scale = voxel, trunc, near, camera.scale
    d.max_weight, d.min_weight = max_weight, min_weight
    d.dfx, d.dfy, d.du, d.dv = camera.depth_fx, camera.depth_fy, camera.depth_u, camera.depth_v
    d.fx, d.fy, d.u, d.v = camera.fx, camera.fy, camera.u, camera.v
    return d


def check_volume(dims, voxel, trunc):
    dims = tuple(int(x) for x in dims)
    if len(dims) != 3 or min(dims) < 1:
        raise ValueError('the volume is empty: %s lattice points' % ' x '.join(str(x) for x in dims))
    if dims[0] * dims[1] * dims[2] >= MAX_POINTS:
        raise ValueError('%d x %d x %d lattice points do not fit int32 (2^31 or more): raise --voxel or narrow --bounds' % dims)
    if not voxel > 0.0:
        raise ValueError('voxel must be positive, got %r' % (voxel,))
    if not trunc > 0.0:
        raise ValueError('trunc must be positive, got %r' % (trunc,))
    return dims


class Volume(object):
    """kfn_fuse_integrate, kfn_fuse_extract_count and kfn_fuse_extract with their buffers.  `tsdf_volume` [nz,ny,nx,2] and
    `color_volume` [nz,ny,nx,4] (None without colour) are device tensors carried from call to call; zeros are the empty
    volume."""

    def __init__(self, dims, origin, voxel, trunc=None, camera=None, image_size=(480, 640), batch=16, color=True,
                 max_weight=64.0, near=0.05, device='cuda:0'):
        import torch
        trunc = 4.0 * voxel if trunc is None else trunc
        self.dims = check_volume(dims, voxel, trunc)
        if batch < 1:
            raise ValueError('batch must be >= 1')
        if not max_weight >= 1.0:
            raise ValueError('max_weight must be at least 1, got %r' % (max_weight,))
        if not near > 0.0:
            raise ValueError('near must be positive, got %r' % (near,))
        H, W = image_size
        if H < 1 or W < 1:
            raise ValueError('the image must have a positive size, got %dx%d' % (H, W))
        self.origin = tuple(float(x) for x in origin)
        self.voxel, self.trunc, self.max_weight, self.near = float(voxel), float(trunc), float(max_weight), float(near)
        self.camera = DepthCamera() if camera is None else camera
        self.shape = (batch, H, W)
        self.lib = _lib.load()
        self.torch, self.device = torch, torch.device(device)
        nx, ny, nz = self.dims
        size = C.c_size_t()
        _lib.check(self.lib.kfn_fuse_scratch_bytes(C.byref(self.descriptor(1)), C.byref(size)), 'kfn_fuse_scratch_bytes')
        with torch.cuda.device(self.device):
            self.tsdf_volume = torch.zeros((nz, ny, nx, 2), dtype=torch.float32, device=self.device)
            self.color_volume = torch.zeros((nz, ny, nx, 4), dtype=torch.float32, device=self.device) if color else None
            self.depth = torch.zeros((batch, H, W), dtype=torch.int16, device=self.device)          # the uint16 bits
            self.frames = torch.zeros((batch, H, W, 3), dtype=torch.uint8, device=self.device) if color else None
            self.poses = torch.zeros((batch, 12), dtype=torch.float32, device=self.device)
            self.scratch = torch.zeros((size.value + 7) // 8, dtype=torch.int64, device=self.device)
            self.totals = torch.zeros(2, dtype=torch.int64, device=self.device)

    def descriptor(self, n, min_weight=1.0):
        B, H, W = self.shape
        return fuse_descriptor(self.camera, self.dims, self.origin, self.voxel, self.trunc, n, H, W, self.near, self.max_weight,
                               min_weight)

    def integrate(self, depth_u16, poses, frames=None):
        """n <= batch depth maps uint16 [n,H,W] (numpy or tensor), their poses, and with colour the frames uint8 [n,H,W,3]."""
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
        if (frames is None) != (self.color_volume is None):
            raise ValueError('frames go with a colour volume: give both or neither')
        if frames is not None:
            fr = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))
            if fr.dtype != torch.uint8 or tuple(fr.shape) != (n, H, W, 3):
                raise ValueError('frames must be uint8 [%d,%d,%d,3], got %s %s' % (n, H, W, fr.dtype, tuple(fr.shape)))
        if torch.is_tensor(poses) and poses.dtype == torch.float32 and tuple(poses.shape) == (n, 12):
            ps = poses
        else:
            ps = torch.from_numpy(pose_rows(poses.cpu().numpy() if torch.is_tensor(poses) else poses))
        if ps.shape[0] != n:
            raise ValueError('%d poses for %d depth maps' % (ps.shape[0], n))
        with torch.cuda.device(self.device):
            self.depth[:n].copy_(dp, non_blocking=True)
            self.poses[:n].copy_(ps, non_blocking=True)
            if frames is not None:
                self.frames[:n].copy_(fr, non_blocking=True)
            d = self.descriptor(n)
            _lib.check(self.lib.kfn_fuse_integrate(C.byref(d), self.tsdf_volume.data_ptr(),
                                                   None if self.color_volume is None else self.color_volume.data_ptr(),
                                                   self.depth.data_ptr(), None if self.frames is None else self.frames.data_ptr(),
                                                   self.poses.data_ptr(), current_stream(self.device)), 'kfn_fuse_integrate')

    def count(self, min_weight=1.0):
        """kfn_fuse_extract_count alone: the totals stay on the device (`totals`)."""
        with self.torch.cuda.device(self.device):
            d = self.descriptor(1, min_weight)
            _lib.check(self.lib.kfn_fuse_extract_count(C.byref(d), self.tsdf_volume.data_ptr(), self.scratch.data_ptr(),
                                                       self.totals.data_ptr(), current_stream(self.device)), 'kfn_fuse_extract_count')

    def emit(self, vertices, colors, triangles, min_weight=1.0, cap_vertices=None, cap_triangles=None):
        """kfn_fuse_extract alone into device tensors [V,3] float32, [V,3] uint8, [N,3] int32 after count(min_weight); the
        capacities default to the tensors' rows."""
        cap_vertices = vertices.shape[0] if cap_vertices is None else cap_vertices
        cap_triangles = triangles.shape[0] if cap_triangles is None else cap_triangles
        if cap_vertices > vertices.shape[0] or cap_vertices > colors.shape[0] or cap_triangles > triangles.shape[0]:
            raise ValueError('the capacities exceed the tensors')
        with self.torch.cuda.device(self.device):
            d = self.descriptor(1, min_weight)
            _lib.check(self.lib.kfn_fuse_extract(C.byref(d), self.tsdf_volume.data_ptr(),
                                                 None if self.color_volume is None else self.color_volume.data_ptr(),
                                                 self.scratch.data_ptr(), vertices.data_ptr(), colors.data_ptr(), triangles.data_ptr(),
                                                 cap_vertices, cap_triangles, current_stream(self.device)), 'kfn_fuse_extract')

    def mesh(self, min_weight=1.0):
        """-> (vertices float32 [V,3], colors uint8 [V,3], triangles int32 [N,3]) as numpy arrays: count, one read of the
        totals, emit."""
        torch = self.torch
        if not min_weight >= 1.0:
            raise ValueError('min_weight must be at least 1, got %r' % (min_weight,))
        self.count(min_weight)
        V, N = (int(x) for x in self.totals.cpu().numpy())
        if V >= MAX_POINTS or N >= MAX_POINTS:
            raise ValueError('the mesh has %d vertices and %d triangles: 2^31 or more do not fit int32' % (V, N))
        with torch.cuda.device(self.device):
            # one spare row each: an empty mesh still has buffers to name
            vertices = torch.zeros((V + 1, 3), dtype=torch.float32, device=self.device)
            colors = torch.zeros((V + 1, 3), dtype=torch.uint8, device=self.device)
            triangles = torch.zeros((N + 1, 3), dtype=torch.int32, device=self.device)
        self.emit(vertices, colors, triangles, min_weight, V, N)
        return vertices[:V].cpu().numpy(), colors[:V].cpu().numpy(), triangles[:N].cpu().numpy()

    def tsdf(self):
        return self.tsdf_volume.cpu().numpy()

    def colors(self):
        return None if self.color_volume is None else self.color_volume.cpu().numpy()


def box_lattice(lo, hi, voxel):
    """A box [lo, hi] -> (dims, origin): lattice points from lo in steps of voxel up to the first at or beyond hi."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()) or not (hi > lo).all():
        raise ValueError('the box is empty: %s .. %s' % (lo.tolist(), hi.tolist()))
    dims = tuple(int(np.ceil((hi[k] - lo[k]) / voxel)) + 1 for k in range(3))
    return dims, tuple(float(x) for x in lo)


def bounds_from_sequence(depth_paths, poses, camera, image_size, pad, batch=16, device='cuda:0'):
    """The default box: the minimum and maximum of the valid stride-8 labels DepthLabeler gives over the frames, padded by
    `pad` (the truncation distance).  ValueError when no label is valid."""
    H, W = image_size
    lab = DepthLabeler(batch, H, W, 8, camera, device)
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for at in range(0, len(depth_paths), batch):
        part = poses[at:at + batch]
        keep = [k for k in range(len(part)) if np.isfinite(part[k]).all()]
        if not keep:
            continue
        depth = load_depth([depth_paths[at + k] for k in keep], (H, W))
        out = lab.labels(depth, part[keep]).cpu().numpy()
        pts = out[..., :3][out[..., 3] > 0]
        if len(pts):
            lo, hi = np.minimum(lo, pts.min(axis=0)), np.maximum(hi, pts.max(axis=0))
    if not np.isfinite(lo).all():
        raise ValueError('no valid depth in the sequence: there is no box to fuse into')
    return lo - pad, hi + pad


# ---- the program --------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(prog='python -m kfnet_amd.fuse', description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='command')
    mk = sub.add_parser('make', help='a scene mesh (PLY, vertex colours) from RGB-D sequences with poses')
    mk.add_argument('--sequence', action='append', default=[], help='a sequence folder; may be given several times')
    mk.add_argument('--output', default='', help='the PLY file to write')
    mk.add_argument('--voxel', type=float, default=0.02, help='metres between lattice points')
    mk.add_argument('--trunc', type=float, default=None, help='truncation distance in metres (4 voxels)')
    mk.add_argument('--bounds', type=float, nargs=6, default=None, metavar=('X0', 'Y0', 'Z0', 'X1', 'Y1', 'Z1'),
                    help='the box to fuse into (the padded extent of the sequences\' stride-8 labels)')
    mk.add_argument('--min_weight', type=float, default=2.0, help='a lattice point counts once this many frames saw it')
    mk.add_argument('--every', type=int, default=1, help='use every K-th frame')
    mk.add_argument('--no_color', action='store_true', help='fuse depth only: the vertices are white')
    add_camera_flags(mk)
    mk.add_argument('--height', type=int, default=480)
    mk.add_argument('--width', type=int, default=640)
    mk.add_argument('--batch', type=int, default=16)
    mk.add_argument('--gpu', type=int, default=0)
    return ap


def make(a):
    from .render import write_ply

    def refuse(text):
        print(text, file=sys.stderr)
        return 1
    if not a.sequence:
        return refuse('fuse make: at least one --sequence is required')
    if not a.output:
        return refuse('fuse make: --output is required')
    if a.batch < 1:
        return refuse('--batch must be >= 1')
    if a.every < 1:
        return refuse('--every must be >= 1')
    if not a.voxel > 0.0:
        return refuse('--voxel must be positive')
    trunc = 4.0 * a.voxel if a.trunc is None else a.trunc
    if not trunc > 0.0:
        return refuse('--trunc must be positive')
    if not a.min_weight >= 1.0:
        return refuse('--min_weight must be at least 1')
    try:
        check_size(a.height, a.width, '--height and --width')
        camera = camera_of(a)
        triples = []
        for s in a.sequence:
            triples += read_sequence(s)
        triples = triples[::a.every]
        box = None
        if a.bounds is not None:
            box = box_lattice(a.bounds[:3], a.bounds[3:], a.voxel)
            check_volume(box[0], a.voxel, trunc)
        poses = read_poses([t[2] for t in triples])
    except ValueError as e:
        return refuse(str(e))
    size = (a.height, a.width)
    import torch
    if not torch.cuda.is_available():
        return refuse('fuse make needs a GPU: the volume is integrated on the device')
    device = 'cuda:%d' % a.gpu
    try:
        if box is None:
            lo, hi = bounds_from_sequence([t[1] for t in triples], poses, camera, size, trunc, a.batch, device)
            box = box_lattice(lo, hi, a.voxel)
            check_volume(box[0], a.voxel, trunc)
        dims, origin = box
        print('%d x %d x %d = %d voxels of %g m from (%g, %g, %g); %d frames' %
              (dims + (dims[0] * dims[1] * dims[2], a.voxel) + origin + (len(triples),)), flush=True)
        vol = Volume(dims, origin, a.voxel, trunc, camera, size, a.batch, not a.no_color, device=device)
        used = 0
        for at in range(0, len(triples), a.batch):
            keep = [k for k in range(at, min(at + a.batch, len(triples))) if np.isfinite(poses[k]).all()]
            for k in range(at, min(at + a.batch, len(triples))):
                if k not in keep:
                    print('%s: the pose is not finite: the frame is left out' % triples[k][2], flush=True)
            if not keep:
                continue
            depth = load_depth([triples[k][1] for k in keep], size)
            frames = None if a.no_color else load_images([triples[k][0] for k in keep], size)
            vol.integrate(depth, poses[keep], frames)
            used += len(keep)
        vertices, colors, triangles = vol.mesh(a.min_weight)
    except ValueError as e:
        return refuse(str(e))
    if not len(triangles):
        return refuse('the volume holds no surface: nothing to write (frames used: %d)' % used)
    write_ply(a.output, vertices, triangles, colors)
    print('%d voxels, %d frames used, %d vertices, %d triangles written to %s' %
          (dims[0] * dims[1] * dims[2], used, len(vertices), len(triangles), a.output))
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
