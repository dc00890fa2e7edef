"""Microbenchmark of tracking against the volume: ms per Tracker.push and per launch group alone -- the live
maps, the ray casts of the levels, the iterations (sums, reduce, update), the commit, the integration -- on depth rendered
from synthetic_scene, with the volume fused from 16 frames under their true poses.

    python tools/mb_track.py [--dim 256 --voxel 0.02 --height 480 --width 640 --cells 32 --reps 50 --blocks 5] [--reloc]

With --reloc: ms per push with the relocaliser (kfn_reloc_*) off and on, window by window in turns, and its four launches alone.

Every figure is the median of `blocks` timed windows of `reps` calls, with the lowest and highest window beside it.  Beside
the ray cast stand two floors at 8 TB/s: the maps it must write (32 bytes a pixel), and those plus the whole tsdf read once,
which bounds from above what any set of rays can need."""
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


def slow_trajectory(count, step=0.03):
    """synthetic_trajectory's path walked at a quarter of its speed."""
    rng = np.random.default_rng([1, 0x7a9ec])
    phase = rng.uniform(0.0, 2.0 * np.pi, size=6)
    out = np.zeros((count, 4, 4))
    for i in range(count):
        a = step * i
        pos = np.array([1.05 + 0.5 * np.sin(a + phase[0]), 1.5 + 0.85 * np.sin(0.7 * a + phase[1]), 1.3 + 0.3 * np.sin(0.5 * a + phase[2])])
        target = np.array([3.0 + 0.2 * np.sin(0.3 * a + phase[3]), 1.5 + 0.5 * np.sin(0.4 * a + phase[4]), 0.6 + 0.2 * np.sin(0.6 * a + phase[5])])
        fwd = (target - pos) / np.linalg.norm(target - pos)
        right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
        right /= np.linalg.norm(right)
        out[i, :3, 0], out[i, :3, 1], out[i, :3, 2], out[i, :3, 3] = right, np.cross(fwd, right), fwd, pos
        out[i, 3, 3] = 1.0
    return out


def reloc_timings(a, torch, track, vol, plain, poses, depth, line):
    """Two trackers on one volume, one with the relocaliser (defaults: 500 ferns, 1024 keyframe slots, 16 of them filled with the
    fused frames' codes): a window of pushes of the one, then of the other, `blocks` times; then the four launches alone."""
    B = len(poses)
    frames = (a.reps + 2) * (a.blocks + 2) * 2 + 8
    plain = track.Tracker(vol, max_frames=frames)
    with_reloc = track.Tracker(vol, max_frames=frames, reloc=True)
    rc = with_reloc.reloc
    for trk in (plain, with_reloc):
        trk.set_state(poses[B - 2])
        trk.first, trk.pushed = poses[B - 2].copy(), 0
        trk.vol.poses[:1].copy_(torch.from_numpy(track.pose_rows(poses[B - 2:B - 1])))
    for k in range(B - 1):                                             # a store of keyframes: the fused frames, harvested or not
        with_reloc._stage(depth[k], None)
        with_reloc.live_maps()
        rc.encode()
        rc.codes[k].copy_(rc.code)
        rc.key_poses[k].copy_(torch.from_numpy(poses[k][:3].reshape(12)))
    st = rc.state()
    st.n = B - 1
    rc.set_state(st)
    plain._stage(depth[B - 1], None)

    def window(trk):
        a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a0.record()
        for _ in range(a.reps):
            trk.push(depth[B - 1])
        b0.record()
        torch.cuda.synchronize()
        return a0.elapsed_time(b0) / a.reps
    for trk in (plain, with_reloc):
        trk.push(depth[B - 1])
    torch.cuda.synchronize()
    off, on = [], []
    for _ in range(a.blocks):
        off.append(window(plain))
        on.append(window(with_reloc))
    print(line % ('Tracker.push, relocaliser off', float(np.median(off)), min(off), max(off)), ' lost %d' % int(plain.trajectory()[1].sum()))
    print(line % ('Tracker.push, relocaliser on', float(np.median(on)), min(on), max(on)),
          ' lost %d, %d keyframes; +%.1f %% of the push' % (int(with_reloc.trajectory()[1].sum()), with_reloc.relocalisation()[1],
                                                            100.0 * (np.median(on) / np.median(off) - 1.0)))
    print(line % (('kfn_reloc_encode, %d ferns' % rc.ferns,) + timed(torch, rc.encode, a.reps, a.blocks)))
    print(line % (('kfn_reloc_search, %d slots' % rc.capacity,) + timed(torch, rc.search, a.reps, a.blocks)))
    print(line % (('kfn_reloc_seed',) + timed(torch, rc.seed, a.reps, a.blocks)))
    print(line % (('kfn_reloc_settle',) + timed(torch, rc.settle, a.reps, a.blocks)))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--dim', type=int, default=256)
    ap.add_argument('--voxel', type=float, default=0.02)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--cells', type=int, default=32)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--reloc', action='store_true', help='instead: the push with and without the relocaliser in turns, and its four launches alone')
    a = ap.parse_args(argv)
    import torch
    from kfnet_amd import fuse, render, synth, track
    from kfnet_amd.labels import DepthCamera
    H, W, n, B = a.height, a.width, a.dim, 16
    cam = DepthCamera(525. * W / 640., 525. * W / 640., W / 2., H / 2.)
    v, c, t = synth.synthetic_scene(1, a.cells)
    poses = slow_trajectory(B)
    r = render.Renderer(v, t, c, (H, W), B, 1, cam)
    _, depth, _, _ = r.render(poses)
    depth = depth.clone()
    vol = fuse.Volume((n, n, n), (-0.1, -0.1, -0.1), a.voxel, None, cam, (H, W), B, False)
    vol.integrate(depth[:B - 1], poses[:B - 1])
    trk = track.Tracker(vol, max_frames=(a.reps + 2) * a.blocks * 2 + 8)
    print('%s; %d^3 voxels of %.4f m, %dx%d, levels %s, iterations %s; median of %d windows of %d calls (lowest .. highest)' %
          (torch.cuda.get_device_name(0), n, a.voxel, H, W, [s[:2] for s in trk.sizes], trk.iterations, a.blocks, a.reps))
    line = '%-52s %9.3f ms (%.3f .. %.3f)'

    def reset():
        trk.set_state(poses[B - 2])
        trk.first, trk.pushed = poses[B - 2].copy(), 0
        trk.vol.poses[:1].copy_(torch.from_numpy(track.pose_rows(poses[B - 2:B - 1])))

    def iterate():
        for l in range(trk.levels - 1, -1, -1):
            for _ in range(trk.iterations[l]):
                trk.icp_sums(l)
                trk.update(l)

    def casts():
        for l in range(trk.levels):
            trk.raycast(l)
    if a.reloc:
        return reloc_timings(a, torch, track, vol, trk, poses, depth, line)
    reset()
    trk._stage(depth[B - 1], None)
    ms = timed(torch, lambda: trk.push(depth[B - 1]), a.reps, a.blocks)
    poses_out, lost, diag = trk.trajectory()
    print(line % ('Tracker.push (one staging copy rides)', ms[0], ms[1], ms[2]), ' lost %d of %d' % (int(lost.sum()), len(lost)))
    reset()
    print(line % (('kfn_track_live_maps, %d levels' % trk.levels,) + timed(torch, trk.live_maps, a.reps, a.blocks)))
    ms = timed(torch, casts, a.reps, a.blocks)
    pixels = sum(h * w for h, w, _ in trk.sizes)
    low, high = pixels * 32 / HBM * 1e3, (pixels * 32 + n ** 3 * 8) / HBM * 1e3
    print(line % ('kfn_track_raycast, %d levels' % trk.levels, ms[0], ms[1], ms[2]),
          '  floors %.4f / %.4f ms   ratios %.0f / %.1f' % (low, high, ms[0] / low, ms[0] / high))
    ms0 = timed(torch, lambda: trk.raycast(0), a.reps, a.blocks)
    print(line % ('kfn_track_raycast, level 0 alone', ms0[0], ms0[1], ms0[2]))
    print(line % (('%d x (kfn_track_icp_sums + kfn_track_update)' % sum(trk.iterations),) + timed(torch, iterate, a.reps, a.blocks)))
    print(line % (('kfn_track_icp_sums + update, level 0, once',) + timed(torch, lambda: (trk.icp_sums(0), trk.update(0)), a.reps, a.blocks)))
    print(line % (('kfn_fuse_integrate, 1 frame, no colour',) + timed(torch, trk.integrate, a.reps, a.blocks)))
    print(line % (('kfn_track_commit',) + timed(torch, trk.commit, a.reps, a.blocks)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
