"""Microbenchmark of fusion and mesh extraction: ms per Volume.integrate call (kfn_fuse_integrate with its
three staging copies, and the launch alone) and per mesh(), with kfn_fuse_extract_count and kfn_fuse_extract separately, on
depth and colour rendered from synthetic_scene.

    python tools/mb_fuse.py [--dim 256 --height 480 --width 640 --batch 16 --cells 32 --reps 200 --blocks 5]

Every figure is the median of `blocks` timed windows of `reps` calls, with the lowest and highest window beside it.  Beside
each stands the time the bytes that must cross memory would take at 8 TB/s: for integrate the volume read once and written
once plus the depth maps and frames; for count the tsdf read once and the scratch written, scanned and read; for emit the
scratch and tsdf read once and the mesh written."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8e12


def timed(torch, fn, reps, blocks):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out)), min(out), max(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--dim', type=int, default=256)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--cells', type=int, default=32)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--blocks', type=int, default=5)
    a = ap.parse_args(argv)
    import ctypes as C
    import torch
    from kfnet_amd import _lib, fuse, render, synth
    from kfnet_amd.labels import DepthCamera
    from kfnet_amd.staging import current_stream
    B, H, W, n = a.batch, a.height, a.width, a.dim
    cam = DepthCamera(525. * W / 640., 525. * W / 640., W / 2., H / 2.)
    v, c, t = synth.synthetic_scene(1, a.cells)
    poses = synth.synthetic_trajectory(B, 1)
    r = render.Renderer(v, t, c, (H, W), B, 1, cam)
    _, depth, frames, _ = r.render(poses)
    depth, frames = depth.clone(), frames.clone()
    voxel = (max(synth.ROOM) + 0.2) / (n - 1)
    vol = fuse.Volume((n, n, n), (-0.1, -0.1, -0.1), voxel, None, cam, (H, W), B)
    points = n ** 3
    print('%d^3 voxels of %.4f m, %d frames of %dx%d a call; median of %d windows of %d calls (lowest .. highest)' %
          (n, voxel, B, H, W, a.blocks, a.reps))
    line = '%-52s %9.3f ms (%.3f .. %.3f)   floor %.3f ms   ratio %.1f'

    def report(name, ms, floor_bytes):
        floor = floor_bytes / HBM * 1e3
        print(line % (name, ms[0], ms[1], ms[2], floor, ms[0] / floor))
    volume_bytes = points * (8 + 16)
    input_bytes = B * H * W * (2 + 3)
    report('Volume.integrate (three copies ride)', timed(torch, lambda: vol.integrate(depth, poses, frames), a.reps, a.blocks),
           2 * volume_bytes + input_bytes)
    d = vol.descriptor(B)

    def launch():
        _lib.check(vol.lib.kfn_fuse_integrate(C.byref(d), vol.tsdf_volume.data_ptr(), vol.color_volume.data_ptr(), vol.depth.data_ptr(),
                                              vol.frames.data_ptr(), vol.poses.data_ptr(), current_stream(vol.device)), 'kfn_fuse_integrate')
    report('kfn_fuse_integrate alone, %d frames' % B, timed(torch, launch, a.reps, a.blocks), 2 * volume_bytes + input_bytes)
    one = vol.descriptor(1)

    def launch_one():
        _lib.check(vol.lib.kfn_fuse_integrate(C.byref(one), vol.tsdf_volume.data_ptr(), vol.color_volume.data_ptr(), vol.depth.data_ptr(),
                                              vol.frames.data_ptr(), vol.poses.data_ptr(), current_stream(vol.device)), 'kfn_fuse_integrate')
    report('kfn_fuse_integrate alone, 1 frame', timed(torch, launch_one, a.reps, a.blocks), 2 * volume_bytes + input_bytes // B)
    # a fresh volume for the mesh: the timed calls above have integrated the same frames many times (the weights are capped)
    vol.tsdf_volume.zero_()
    vol.color_volume.zero_()
    vol.integrate(depth, poses, frames)
    vertices, colors, triangles = vol.mesh(2.0)
    V, N = len(vertices), len(triangles)
    print('mesh at min_weight 2: %d vertices, %d triangles' % (V, N))
    report('Volume.mesh (count, read totals, emit, copy back)', timed(torch, lambda: vol.mesh(2.0), max(1, a.reps // 10), a.blocks),
           points * (8 + 9 + 9 + 8) + V * 15 + N * 12)
    report('kfn_fuse_extract_count', timed(torch, lambda: vol.count(2.0), a.reps, a.blocks), points * (8 + 9 + 8 + 8))
    dv = torch.zeros((V, 3), dtype=torch.float32, device=vol.device)
    dc = torch.zeros((V, 3), dtype=torch.uint8, device=vol.device)
    dt = torch.zeros((N, 3), dtype=torch.int32, device=vol.device)
    report('kfn_fuse_extract', timed(torch, lambda: vol.emit(dv, dc, dt, 2.0), a.reps, a.blocks), points * 9 + V * (15 + 48) + N * 12)
    return 0


if __name__ == '__main__':
    sys.exit(main())
