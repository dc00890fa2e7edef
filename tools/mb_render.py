"""Microbenchmark of the mesh renderer: ms per frame of Renderer.launch (kfn_render: clear, rasterise,
resolve) at strides 8 and 1 on synthetic_scene(cells), beside DepthLabeler.labels on the depth maps it rendered (the old
route to the same labels) and beside what `render make` spends per frame on the host writing the label file and two PNGs.

    python tools/mb_render.py [--height 480 --width 640 --batch 16 --cells 32 128 --reps 200 --blocks 5]

Every figure is the median of `blocks` timed windows of `reps` launches, with the lowest and highest window beside it.
The three kernels separately come from a kernel trace of this program, taken in a run of its own."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, fn, reps, blocks):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
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
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--cells', type=int, nargs='+', default=[32, 128])
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--blocks', type=int, default=5)
    a = ap.parse_args(argv)
    import torch
    from kfnet_amd import render, synth
    from kfnet_amd.labels import DepthCamera, DepthLabeler, pose_rows
    B, H, W = a.batch, a.height, a.width
    cam = DepthCamera(525. * W / 640., 525. * W / 640., W / 2., H / 2.)
    poses = synth.synthetic_trajectory(B, 1)
    print('%dx%d, %d frames a launch; median of %d windows of %d launches (lowest .. highest)' % (H, W, B, a.blocks, a.reps))
    print('%-44s %12s %26s' % ('', 'ms / frame', 'ms / launch'))
    full = None
    for cells in a.cells:
        v, c, t = synth.synthetic_scene(1, cells)
        for stride in (8, 1):
            r = render.Renderer(v, t, c, (H, W), B, stride, cam)
            r.poses.copy_(torch.from_numpy(pose_rows(poses)))
            ms, lo, hi = timed(torch, lambda: r.launch(B), a.reps, a.blocks)
            print('%-44s %12.4f %10.3f (%.3f .. %.3f)' % ('kfn_render stride %d, %d triangles' % (stride, len(t)), ms / B, ms, lo, hi))
            if stride == 1:
                full = r
    labels, depth, frames, _ = full.launch(B)
    dposes = full.poses.clone()
    for stride in (8, 1):
        lab = DepthLabeler(B, H, W, stride, cam)
        ms, lo, hi = timed(torch, lambda: lab.labels(depth, dposes), a.reps, a.blocks)
        print('%-44s %12.4f %10.3f (%.3f .. %.3f)' % ('DepthLabeler.labels stride %d (two copies ride)' % stride, ms / B, ms, lo, hi))
    # what the program does per frame on the host once the images are back
    host_l, host_d, host_f = labels.cpu().numpy(), depth.cpu().numpy(), frames.cpu().numpy()
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        for k in range(B):
            host_l[k].tofile(os.path.join(tmp, 'label_%d.bin' % k))
        t1 = time.perf_counter()
        for k in range(B):
            render.write_png(os.path.join(tmp, 'd%d.png' % k), host_d[k])
        t2 = time.perf_counter()
        for k in range(B):
            render.write_png(os.path.join(tmp, 'f%d.png' % k), host_f[k])
        t3 = time.perf_counter()
    print('host, per frame: label file %.2f ms, depth PNG %.2f ms, frame PNG %.2f ms' %
          ((t1 - t0) * 1e3 / B, (t2 - t1) * 1e3 / B, (t3 - t2) * 1e3 / B))
    return 0


if __name__ == '__main__':
    sys.exit(main())
