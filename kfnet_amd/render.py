"""Training labels, depth maps and frames rendered from a scene mesh, on the device.

Some scenes ship a model and no usable depth (12-Scenes' meshes; 7-Scenes' fused model, whose rendered depth the common
practice trains on).  This module turns a triangle mesh with vertex colours and camera-to-world poses into what
`kfnet_amd.labels make` writes from depth maps, in the same formats:

    python -m kfnet_amd.render make --model scene.ply (--poses pose_list.txt | --sequence DIR [--sequence DIR2 ...])
                                    --output_folder I [--stride 1|8] [--depth_png] [--frames]
                                    [--focal_x 525 --focal_y 525 --u 320 --v 240] [--height 480 --width 640]
                                    [--batch 16] [--gpu 0] [--near 0.05]

writes pose_list.txt, transform.txt (from the stride-8 labels, the pixels the loss reads) and labels/label_<i>.bin with
label_list.txt; --depth_png adds 16-bit depth/frame-<i>.depth.png with depth_list.txt (the input of `SCoordNet.train
--depth`), --frames adds frames/frame-<i>.color.png with image_list.txt.  A frame whose pose is not finite is reported
and left out of every list.

    vertices, colors, triangles = read_ply(path)          ascii and binary_little_endian, hand-written
    write_ply(path, vertices, triangles, colors)
    r = Renderer(vertices, triangles, colors, (H, W), batch, stride, DepthCamera(...))
    labels, depth, frames, stats = r.render(poses)        device tensors the next call overwrites

There is no fallback: a missing entry point or an unsupported shape raises.
"""
import argparse
import ctypes as C
import os
import struct
import sys
import zlib

import numpy as np

from . import _lib
from .labels import (DepthCamera, DepthLabeler, add_camera_flags, add_frames, camera_of, decorrelating_transform, pose_rows,
                     read_poses, read_sequence, write_transform)
from .staging import check_size, current_stream
from .tools.io import read_lines

# ---- PLY ----------------------------------------------------------------------------------------------------------------
PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2',
             'uint16': 'u2', 'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4',
             'double': 'f8', 'float64': 'f8'}


def _ply_header(path, data):
    """-> (format, elements [(name, count, [property])], body offset, header line count); a property is (name, type) or
    (name, count type, item type)."""
    if not data.startswith(b'ply'):
        raise ValueError('%s: line 1: not a PLY file' % path)
    end = data.find(b'end_header')
    stop = data.find(b'\n', end) if end >= 0 else -1
    if stop < 0:
        raise ValueError('%s: the header has no end_header line' % path)
    fmt, elements = None, []
    lines = data[:stop].decode('ascii', 'replace').split('\n')
    for no, line in enumerate(lines, 1):
        w = line.split()
        if not w or w[0] in ('ply', 'comment', 'obj_info', 'end_header'):
            continue
        try:
            if w[0] == 'format':
                fmt = w[1]
                if fmt == 'binary_big_endian':
                    raise ValueError('%s: line %d: big-endian files are not read (format %s)' % (path, no, fmt))
                if fmt not in ('ascii', 'binary_little_endian') or w[2] != '1.0':
                    raise ValueError('%s: line %d: unknown format %s' % (path, no, ' '.join(w[1:])))
            elif w[0] == 'element':
                elements.append((w[1], int(w[2]), []))
            elif w[0] == 'property' and elements:
                if w[1] == 'list':
                    elements[-1][2].append((w[4], PLY_TYPES[w[2]], PLY_TYPES[w[3]]))
                else:
                    elements[-1][2].append((w[2], PLY_TYPES[w[1]]))
            else:
                raise ValueError('%s: line %d: unexpected header line %r' % (path, no, line))
        except (IndexError, KeyError):
            raise ValueError('%s: line %d: malformed header line %r' % (path, no, line))
    if fmt is None:
        raise ValueError('%s: the header has no format line' % path)
    return fmt, elements, stop + 1, len(lines)


def _fan(polygons, path, where):
    tris = []
    for k, (poly, at) in enumerate(zip(polygons, where)):
        if len(poly) < 3:
            raise ValueError('%s: %s: face %d lists %d vertices, a face needs at least 3' % (path, at, k, len(poly)))
        for i in range(1, len(poly) - 1):
            tris.append((poly[0], poly[i], poly[i + 1]))
    return np.asarray(tris, dtype=np.int64).reshape(-1, 3)


def read_ply(path):
    """-> (vertices float32 [V,3], colors uint8 [V,3] or None, triangles int32 [N,3]) of an ascii or binary_little_endian PLY
    file: vertex properties x y z (float or double), optionally red green blue (uchar), any others skipped; faces with a
    uchar or int count and int or uint indices, polygons fan-triangulated.  ValueError names the file and the line or byte."""
    with open(path, 'rb') as f:
        data = f.read()
    fmt, elements, offset, line_no = _ply_header(path, data)
    names = [e[0] for e in elements]
    if 'vertex' not in names:
        raise ValueError('%s: no vertex element' % path)
    if 'face' not in names:
        raise ValueError('%s: no face element (point clouds without faces are not rendered)' % path)
    vprops = dict((p[0], p) for p in elements[names.index('vertex')][2])
    for axis in 'xyz':
        if axis not in vprops or len(vprops[axis]) != 2 or vprops[axis][1] not in ('f4', 'f8'):
            raise ValueError('%s: vertex property %s must be float or double' % (path, axis))
    has_colour = all(c in vprops and vprops[c][1:] == ('u1',) for c in ('red', 'green', 'blue'))
    vertices = colors = triangles = None
    text = data[offset:].decode('ascii', 'replace').split('\n') if fmt == 'ascii' else None
    row = 0
    for name, count, props in elements:
        lists = [p for p in props if len(p) == 3]
        if name == 'face' and (len(lists) != 1 or lists[0][1] not in ('u1', 'i4') or lists[0][2] not in ('i4', 'u4')):
            raise ValueError('%s: a face needs one list with a uchar or int count and int or uint indices' % path)
        if name != 'face' and lists and fmt != 'ascii':
            raise ValueError('%s: element %s: list properties are read in the face element only' % (path, name))
        if fmt == 'ascii':
            if row + count > len(text) or (count and not ''.join(text[row + count - 1:row + count]).strip()):
                raise ValueError('%s: line %d: truncated: element %s has %d rows, the file ends before' %
                                 (path, line_no + len(text), name, count))
            rows, at = text[row:row + count], ['line %d' % (line_no + row + k + 1) for k in range(count)]
            row += count
            try:
                if name == 'vertex':
                    table = np.array([r.split() for r in rows], dtype=np.float64).reshape(count, len(props))
                    cols = dict((p[0], table[:, k]) for k, p in enumerate(props))
                elif name == 'face':
                    k0 = [len(p) == 3 for p in props].index(True)
                    polys = []
                    for r, a in zip(rows, at):
                        w = r.split()
                        n = int(w[k0])
                        if n < 3:
                            raise ValueError('%s: %s: a list count of %d is below 3' % (path, a, n))
                        if len(w) < k0 + 1 + n:
                            raise ValueError('%s: %s: truncated: the face lists %d indices and holds %d' % (path, a, n, len(w) - k0 - 1))
                        polys.append([int(x) for x in w[k0 + 1:k0 + 1 + n]])
                    triangles = _fan(polys, path, at)
            except ValueError as e:
                if str(e).startswith(path):
                    raise
                raise ValueError('%s: line %d: element %s: %s' % (path, line_no + row - count + 1, name, e))
        else:
            if not lists:
                dt = np.dtype([(p[0], '<' + p[1]) for p in props])
                if offset + count * dt.itemsize > len(data):
                    raise ValueError('%s: byte %d: truncated: element %s needs %d bytes, %d are left' %
                                     (path, len(data), name, count * dt.itemsize, len(data) - offset))
                table = np.frombuffer(data, dtype=dt, count=count, offset=offset)
                offset += count * dt.itemsize
                cols = dict((p[0], table[p[0]]) for p in props)
            else:
                lp = lists[0]
                fast = np.dtype([('n', '<' + lp[1]), ('i', '<' + lp[2], (3,))])
                tri = None
                if len(props) == 1 and offset + count * fast.itemsize <= len(data):
                    table = np.frombuffer(data, dtype=fast, count=count, offset=offset)
                    if (table['n'] == 3).all():
                        tri, offset = table['i'].astype(np.int64), offset + count * fast.itemsize
                if tri is None:
                    polys, at = [], []
                    for k in range(count):
                        poly = None
                        for p in props:
                            size = np.dtype(p[1]).itemsize
                            if offset + size > len(data):
                                raise ValueError('%s: byte %d: truncated in face %d of %d' % (path, len(data), k, count))
                            if len(p) == 2:
                                offset += size
                                continue
                            n = int(np.frombuffer(data, dtype='<' + p[1], count=1, offset=offset)[0])
                            if n < 3:
                                raise ValueError('%s: byte %d: a list count of %d is below 3' % (path, offset, n))
                            at.append('byte %d' % offset)
                            offset += size
                            size = n * np.dtype(p[2]).itemsize
                            if offset + size > len(data):
                                raise ValueError('%s: byte %d: truncated in face %d of %d' % (path, len(data), k, count))
                            poly = np.frombuffer(data, dtype='<' + p[2], count=n, offset=offset).astype(np.int64).tolist()
                            offset += size
                        polys.append(poly)
                    tri = _fan(polys, path, at)
                triangles = tri
        if name == 'vertex':
            vertices = np.stack([cols['x'], cols['y'], cols['z']], axis=1).astype(np.float32)
            if has_colour:
                colors = np.stack([cols['red'], cols['green'], cols['blue']], axis=1).astype(np.uint8)
    if triangles.size and (triangles.min() < -(1 << 31) or triangles.max() >= (1 << 31)):
        raise ValueError('%s: a face index does not fit 32 bits' % path)
    return np.ascontiguousarray(vertices), colors, np.ascontiguousarray(triangles, dtype=np.int32)


def write_ply(path, vertices, triangles, colors=None, binary=True):
    """A PLY file of float vertices, optional uchar colours and triangles (uchar count, int indices)."""
    vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    triangles = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    head = ['ply', 'format %s 1.0' % ('binary_little_endian' if binary else 'ascii'), 'element vertex %d' % len(vertices),
            'property float x', 'property float y', 'property float z']
    if colors is not None:
        colors = np.asarray(colors, dtype=np.uint8).reshape(len(vertices), 3)
        head += ['property uchar red', 'property uchar green', 'property uchar blue']
    head += ['element face %d' % len(triangles), 'property list uchar int vertex_indices', 'end_header']
    with open(path, 'wb') as f:
        f.write(('\n'.join(head) + '\n').encode('ascii'))
        if binary:
            fields = [('p', '<f4', (3,))] + ([('c', 'u1', (3,))] if colors is not None else [])
            v = np.zeros(len(vertices), dtype=np.dtype(fields))
            v['p'] = vertices
            if colors is not None:
                v['c'] = colors
            f.write(v.tobytes())
            t = np.zeros(len(triangles), dtype=np.dtype([('n', 'u1'), ('i', '<i4', (3,))]))
            t['n'], t['i'] = 3, triangles
            f.write(t.tobytes())
        else:
            for k in range(len(vertices)):
                line = '%.9g %.9g %.9g' % tuple(vertices[k])
                if colors is not None:
                    line += ' %d %d %d' % tuple(colors[k])
                f.write((line + '\n').encode('ascii'))
            for t in triangles:
                f.write(('3 %d %d %d\n' % tuple(t)).encode('ascii'))


# ---- PNG ----------------------------------------------------------------------------------------------------------------
def write_png(path, image):
    """uint16 [H,W] -> 16-bit grey, uint8 [H,W,3] -> 8-bit RGB; filter 0 on every row, one IDAT."""
    image = np.ascontiguousarray(image)
    if image.dtype == np.uint16 and image.ndim == 2:
        depth, colour, rows = 16, 0, image.astype('>u2').view(np.uint8).reshape(image.shape[0], -1)
    elif image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3:
        depth, colour, rows = 8, 2, image.reshape(image.shape[0], -1)
    else:
        raise ValueError('write_png takes uint16 [H,W] or uint8 [H,W,3], got %s %s' % (image.dtype, image.shape))
    raw = np.concatenate([np.zeros((rows.shape[0], 1), dtype=np.uint8), rows], axis=1).tobytes()

    def chunk(kind, body):
        return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body) & 0xFFFFFFFF)
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', image.shape[1], image.shape[0], depth, colour, 0, 0, 0)) +
                chunk(b'IDAT', zlib.compress(raw, 6)) + chunk(b'IEND', b''))


# ---- the renderer -------------------------------------------------------------------------------------------------------
def render_descriptor(camera, B, V, N, H, W, stride, near=0.05, ld_labels=4):
    """kfn_render_desc: every derived constant in fp64, rounded to fp32 once (ctypes does the rounding), as
    DepthCamera.descriptor does."""
    d = _lib.RenderDesc(B=B, V=V, N=N, H=H, W=W, stride=stride, ld_labels=ld_labels, raw_min=camera.raw_min,
                        raw_max=camera.raw_max)
    d.u, d.v = camera.u, camera.v
    d.inv_fx, d.inv_fy = 1.0 / camera.fx, 1.0 / camera.fy
    d.fx, d.fy = camera.fx, camera.fy
    d.near, d.scale = near, camera.scale
    return d


def check_mesh(vertices, triangles, colors):
    vertices = np.ascontiguousarray(vertices, dtype=np.float32)
    triangles = np.ascontiguousarray(triangles, dtype=np.int32)
    if vertices.ndim != 2 or vertices.shape[1] != 3 or not len(vertices):
        raise ValueError('vertices must be [V,3] with V >= 1, got %s' % (vertices.shape,))
    if triangles.ndim != 2 or triangles.shape[1] != 3 or not len(triangles):
        raise ValueError('triangles must be [N,3] with N >= 1, got %s' % (triangles.shape,))
    if colors is not None:
        colors = np.ascontiguousarray(colors)
        if colors.dtype != np.uint8 or colors.shape != vertices.shape:
            raise ValueError('colors must be uint8 %s, got %s %s' % (vertices.shape, colors.dtype, colors.shape))
    return vertices, triangles, colors


class Renderer(object):
    """kfn_render with its buffers: the model is uploaded once; render(poses) takes n <= batch camera-to-world poses and
    returns (labels [n,h,w,4] float32, depth [n,h,w] uint16, frames [n,h,w,3] uint8, stats [n,5] int32), device tensors that
    the next call overwrites; nothing waits for the device.  `zbuf` [batch,h,w] int64 holds the keys of the last call."""

    moments = DepthLabeler.moments

    def __init__(self, vertices, triangles, colors=None, image_size=(480, 640), batch=16, stride=8, camera=None, near=0.05,
                 device='cuda:0'):
        import torch
        if batch < 1:
            raise ValueError('batch must be >= 1')
        H, W = image_size
        check_size(H, W, 'the height and width of rendered images')
        if stride not in (1, 8):
            raise ValueError('stride must be 1 or 8')
        if not near > 0.0:
            raise ValueError('near must be positive, got %r' % (near,))
        vertices, triangles, colors = check_mesh(vertices, triangles, colors)
        self.lib = _lib.load()
        self.torch, self.device = torch, torch.device(device)
        self.shape, self.stride, self.near = (batch, H, W), stride, float(near)
        self.camera = DepthCamera() if camera is None else camera
        self.counts = (len(vertices), len(triangles))
        h, w = H // stride, W // stride
        size = C.c_size_t()
        _lib.check(self.lib.kfn_render_scratch_bytes(C.byref(self.descriptor(batch)), C.byref(size)), 'kfn_render_scratch_bytes')
        assert size.value == batch * h * w * 8
        with torch.cuda.device(self.device):
            self.vertices = torch.from_numpy(vertices).to(self.device)
            self.triangles = torch.from_numpy(triangles).to(self.device)
            self.colors = None if colors is None else torch.from_numpy(colors).to(self.device)
            self.poses = torch.zeros((batch, 12), dtype=torch.float32, device=self.device)
            self.zbuf = torch.zeros((batch, h, w), dtype=torch.int64, device=self.device)
            self.labels = torch.zeros((batch, h, w, 4), dtype=torch.float32, device=self.device)
            self.depth = torch.zeros((batch, h, w), dtype=torch.int16, device=self.device)        # the uint16 bits
            self.frames = torch.zeros((batch, h, w, 3), dtype=torch.uint8, device=self.device)
            self.stats = torch.zeros((batch, 5), dtype=torch.int32, device=self.device)

    def descriptor(self, n):
        B, H, W = self.shape
        return render_descriptor(self.camera, n, self.counts[0], self.counts[1], H, W, self.stride, self.near)

    def render(self, poses):
        torch = self.torch
        if torch.is_tensor(poses) and poses.dtype == torch.float32 and poses.dim() == 2 and poses.shape[1] == 12:
            ps = poses
        else:
            ps = torch.from_numpy(pose_rows(poses.cpu().numpy() if torch.is_tensor(poses) else poses))
        n = ps.shape[0]
        if not 1 <= n <= self.shape[0]:
            raise ValueError('%d poses for a batch of %d' % (n, self.shape[0]))
        with torch.cuda.device(self.device):
            self.poses[:n].copy_(ps, non_blocking=True)
        return self.launch(n)

    def launch(self, n):
        """kfn_render over the first n rows of self.poses as they stand on the device: the three launches alone, on the
        current stream, so a captured graph can hold them."""
        torch = self.torch
        with torch.cuda.device(self.device):
            d = self.descriptor(n)
            _lib.check(self.lib.kfn_render(C.byref(d), self.vertices.data_ptr(), None if self.colors is None else self.colors.data_ptr(),
                                           self.triangles.data_ptr(), self.poses.data_ptr(), self.zbuf.data_ptr(),
                                           self.labels.data_ptr(), self.depth.data_ptr(), self.frames.data_ptr(),
                                           self.stats.data_ptr(), current_stream(self.device)), 'kfn_render')
        return self.labels[:n], self.depth[:n].view(torch.uint16), self.frames[:n], self.stats[:n]

    def winners(self, n):
        """The triangle index per sample of the last call's first n frames, -1 where nothing was hit (a host array)."""
        keys = self.zbuf[:n].cpu().numpy()
        return np.where(keys == -1, -1, keys & 0xFFFFFFFF)


# ---- the program --------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(prog='python -m kfnet_amd.render', description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='command')
    mk = sub.add_parser('make', help='lists, transform.txt, label files, depth maps and frames from a mesh and poses')
    mk.add_argument('--model', default='', help='the scene: a PLY file with faces')
    mk.add_argument('--poses', default='', help='a list of 4x4 camera-to-world pose files, one path per line')
    mk.add_argument('--sequence', action='append', default=[], help='a sequence folder, for its poses and colour images')
    mk.add_argument('--output_folder', default='')
    mk.add_argument('--stride', type=int, default=1, help='of the label files: 1 (what training reads) or 8')
    mk.add_argument('--depth_png', action='store_true', help='also write 16-bit depth maps and depth_list.txt')
    mk.add_argument('--frames', action='store_true', help='also write the rendered colour frames and image_list.txt')
    add_camera_flags(mk)
    mk.add_argument('--height', type=int, default=480)
    mk.add_argument('--width', type=int, default=640)
    mk.add_argument('--batch', type=int, default=16)
    mk.add_argument('--gpu', type=int, default=0)
    mk.add_argument('--near', type=float, default=0.05)
    return ap


def _write_list(folder, name, paths):
    with open(os.path.join(folder, name), 'w') as f:
        f.write(''.join(p + '\n' for p in paths))


def make(a):
    def refuse(text):
        print(text, file=sys.stderr)
        return 1
    if not a.model:
        return refuse('render make: --model is required')
    if bool(a.poses) == bool(a.sequence):
        return refuse('render make: give either --poses or --sequence')
    if not a.output_folder:
        return refuse('render make: --output_folder is required')
    if a.batch < 1:
        return refuse('--batch must be >= 1')
    if a.stride not in (1, 8):
        return refuse('--stride must be 1 or 8')
    if not a.near > 0.0:
        return refuse('--near must be positive')
    try:
        check_size(a.height, a.width, '--height and --width')
        camera = camera_of(a)
        if camera.register:
            raise ValueError('the --depth_* flags describe a depth camera: a rendered depth map is the colour camera\'s own')
        if not os.path.isfile(a.model):
            raise ValueError('%s is not a file' % a.model)
        images = None
        if a.poses:
            if not os.path.isfile(a.poses):
                raise ValueError('%s is not a file' % a.poses)
            pose_paths = [x for x in read_lines(a.poses) if x]
            for p in pose_paths:
                if not os.path.exists(p):
                    raise ValueError('%s is missing' % p)
        else:
            triples = []
            for s in a.sequence:
                triples += read_sequence(s)
            images, pose_paths = [t[0] for t in triples], [t[2] for t in triples]
        if not pose_paths:
            raise ValueError('no poses to render')
        vertices, colors, triangles = read_ply(a.model)
        vertices, triangles, colors = check_mesh(vertices, triangles, colors)
        if a.frames and colors is None:
            raise ValueError('%s has no vertex colours (red green blue): --frames has nothing to draw' % a.model)
        poses = read_poses(pose_paths)
    except ValueError as e:
        return refuse(str(e))
    pose_paths = [os.path.abspath(p) for p in pose_paths]
    keep = [k for k in range(len(poses)) if np.isfinite(poses[k]).all()]
    for k in range(len(poses)):
        if k not in keep:
            print('%s: the pose is not finite: the frame is left out' % pose_paths[k], flush=True)
    if not keep:
        return refuse('no finite pose to render')
    count, H, W = len(keep), a.height, a.width
    print('%d vertices, %d triangles, %d frames; writing to %s' % (len(vertices), len(triangles), count, a.output_folder), flush=True)
    import torch
    if not torch.cuda.is_available():
        return refuse('render make needs a GPU: the images are rendered on the device')
    out = a.output_folder
    os.makedirs(os.path.join(out, 'labels'), exist_ok=True)
    for flag, name in ((a.depth_png, 'depth'), (a.frames, 'frames')):
        if flag:
            os.makedirs(os.path.join(out, name), exist_ok=True)
    device = 'cuda:%d' % a.gpu
    grid = Renderer(vertices, triangles, colors, (H, W), a.batch, 8, camera, a.near, device)
    full = Renderer(vertices, triangles, colors, (H, W), a.batch, 1, camera, a.near, device) \
        if (a.stride == 1 or a.depth_png or a.frames) else None
    total, pivot = None, None
    label_paths, depth_paths, frame_paths = [], [], []
    try:
        for lo in range(0, count, a.batch):
            part = poses[keep[lo:lo + a.batch]]
            if pivot is None:
                pivot = part[0, :3, 3].copy()              # the first frame's camera centre, as in labels make
            glabels = grid.render(part)[0]
            total = add_frames(total, grid.moments(glabels, pivot).cpu().numpy())
            host = glabels.cpu().numpy() if a.stride == 8 else None
            if full is not None:
                flabels, fdepth, fframes, _ = full.render(part)
                if a.stride == 1:
                    host = flabels.cpu().numpy()
                fdepth = fdepth.cpu().numpy() if a.depth_png else None
                fframes = fframes.cpu().numpy() if a.frames else None
            for k in range(len(part)):
                i = lo + k
                label_paths.append(os.path.abspath(os.path.join(out, 'labels', 'label_%d.bin' % i)))
                host[k].tofile(label_paths[-1])
                if a.depth_png:
                    depth_paths.append(os.path.abspath(os.path.join(out, 'depth', 'frame-%06d.depth.png' % i)))
                    write_png(depth_paths[-1], fdepth[k])
                if a.frames:
                    frame_paths.append(os.path.abspath(os.path.join(out, 'frames', 'frame-%06d.color.png' % i)))
                    write_png(frame_paths[-1], fframes[k])
        M = decorrelating_transform(total, pivot)
    except ValueError as e:
        return refuse(str(e))
    _write_list(out, 'pose_list.txt', [pose_paths[k] for k in keep])
    _write_list(out, 'label_list.txt', label_paths)
    if a.depth_png:
        _write_list(out, 'depth_list.txt', depth_paths)
    if a.frames:
        _write_list(out, 'image_list.txt', frame_paths)
    elif images is not None:
        _write_list(out, 'image_list.txt', [os.path.abspath(images[k]) for k in keep])
    write_transform(os.path.join(out, 'transform.txt'), M)
    print('%d valid label points at stride 8; transform.txt and %d label files written to %s' % (int(total[0]), count, out))
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
