"""Microbenchmark of the label kernels: ms and GB/s of kfn_depth_labels and kfn_label_moments at strides 1 and
8, without and with registration, on synthetic depth maps and poses.

    python tools/mb_labels.py [--height 480 --width 640 --batch 4 --reps 50]

Bytes: the label kernel reads 2 bytes per depth pixel it touches (the whole map at stride 1, one pixel in 64 at stride 8) and
writes 16 per output pixel; the moments kernel reads 16 per label pixel.  Both are launch-latency-sized at these shapes."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--reps', type=int, default=50)
    a = ap.parse_args(argv)
    import torch
    from kfnet_amd.labels import DepthCamera, DepthLabeler, pose_rows
    B, H, W = a.batch, a.height, a.width
    rng = np.random.default_rng(0)
    depth = torch.from_numpy(rng.integers(0, 65536, size=(B, H, W)).astype(np.uint16).view(np.int16)).cuda()
    poses = torch.from_numpy(pose_rows(np.tile(np.eye(4), (B, 1, 1)))).cuda()
    print('%dx%d batch %d, %d launches each' % (H, W, B, a.reps))
    print('%-34s %9s %9s %9s' % ('launch', 'ms', 'MB', 'GB/s'))
    for stride in (1, 8):
        for name, cam in (('', DepthCamera()), (', registered', DepthCamera(depth_fx=585., depth_fy=585.))):
            lab = DepthLabeler(B, H, W, stride, cam)
            pixels = B * (H // stride) * (W // stride)
            nbytes = (B * H * W * 2 if stride == 1 else pixels * 2) + pixels * 16
            ms = timed(torch, lambda: lab.labels(depth, poses), a.reps)      # two small device copies ride along
            print('%-34s %9.4f %9.2f %9.1f' % ('kfn_depth_labels stride %d%s' % (stride, name), ms, nbytes / 1e6, nbytes / ms / 1e6))
        out = lab.labels(depth, poses)
        ms = timed(torch, lambda: lab.moments(out, (0.0, 0.0, 0.0)), a.reps)
        print('%-34s %9.4f %9.2f %9.1f' % ('kfn_label_moments stride %d' % stride, ms, pixels * 16 / 1e6, pixels * 16 / ms / 1e6))
    return 0


if __name__ == '__main__':
    sys.exit(main())
