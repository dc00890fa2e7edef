"""Times `process()` of SCoordNetEngine, OFlowNetEngine and KFNetEngine on the same synthetic frames (device events, after
warm-up) and prints one JSON line with frames/s per engine and batch.

    python tools/mb_modes.py [--batch 4 [8 16 ...]] [--frames 64] [--reps 3] [--warmup 1] [--height 480 --width 640]

Every engine is built with random weights and max_chunk = --frames; a timed repetition is one process() of the whole
resident chunk (KFNetEngine: heavy phase on two streams + the Kalman scan; the single-network engines: their network +
the record launch).  Several --batch values show where an engine stops scaling with the batch.

`--engines pose` times the pose stage instead: ms per PnPSolver.solve of --frames records on a 60x80 grid (20 % outliers,
per-cell sigma 0.5-4 cm) against solve_unc unweighted and weighted, in the same JSON line under "pose_ms"; and, under
"pose_sampling_ms", solve with uniform sampling at 256 hypotheses against guided sampling (both weights) at 256 and at 64,
the five taken in turns; and, under "pose_depth_ms", KabschSolver.solve and its weighted solve_unc on the same records with
their camera points (5 mm depth noise) against PnPSolver's, the four taken in turns; and, under "pose_track_ms", ms per call of PoseFilter.run and of PoseTracker.run (both models,
with and without the backward pass) at S x T = 1 x 1000, 8 x 500 and 64 x 64, the five taken in turns.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def _pose_records(frames, h, w):
    """`frames` synthetic h x w records on the device: 20 % outliers, per-cell sigma 0.5-4 cm, confidence 1 / sigma."""
    import numpy as np
    import torch
    rng = np.random.default_rng(0)
    rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    z = rng.uniform(0.5, 5.0, size=(frames, h, w))
    rec = np.stack([(cc * 8 - 320.) / 525. * z, (rr * 8 - 240.) / 525. * z, z, z], axis=-1)     # camera = scene frame
    sigma = np.exp(rng.uniform(np.log(0.005), np.log(0.04), size=(frames, h, w)))
    rec[..., :3] += rng.normal(size=rec[..., :3].shape) * sigma[..., None]
    out = rng.random((frames, h, w)) < 0.2
    rec[..., :3][out] = rng.uniform(-5, 5, size=(int(out.sum()), 3))
    rec[..., 3] = 1.0 / sigma
    return torch.from_numpy(rec.astype(np.float32)).cuda()


def time_pose_sampling(frames, reps, warmup, h=60, w=80, hypotheses=256):
    """ms per call of PnPSolver.solve with uniform sampling at `hypotheses` and with each guided sampling at `hypotheses`
    and at a quarter of it, on _pose_records; the calls take turns, each timed with its own pair of events, and the mean
    over `reps` turns is reported."""
    import torch
    from kfnet_amd.KFNet.pnp import PnPSolver
    dev = _pose_records(frames, h, w)
    calls = {'uniform_%d' % hypotheses: PnPSolver(h, w, hypotheses=hypotheses).solve}
    for sampling in ('confidence', 'confidence2'):
        for H in (hypotheses, max(1, hypotheses // 4)):
            calls['%s_%d' % (sampling, H)] = PnPSolver(h, w, hypotheses=H, sampling=sampling).solve
    total = {name: 0.0 for name in calls}
    for turn in range(max(warmup, 1) + reps):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(dev)
            e1.record()
            e1.synchronize()
            if turn >= max(warmup, 1):
                total[name] += e0.elapsed_time(e1)
    return {name: round(v / reps, 3) for name, v in total.items()}


def _pose_cam_points(frames, h, w):
    """The camera points [frames,h,w,4] of _pose_records' frames (its first draw is the depth; camera = scene frame), with
    5 mm of noise in depth, mask 1."""
    import numpy as np
    import torch
    z = np.random.default_rng(0).uniform(0.5, 5.0, size=(frames, h, w))
    z = z + np.random.default_rng(1).normal(scale=0.005, size=z.shape)
    rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    cam = np.stack([(cc * 8 - 320.) / 525. * z, (rr * 8 - 240.) / 525. * z, z, np.ones_like(z)], axis=-1)
    return torch.from_numpy(cam.astype(np.float32)).cuda()


def time_pose_depth(frames, reps, warmup, h=60, w=80):
    """ms per call of KabschSolver.solve / solve_unc (weighted) and of PnPSolver's on the same records, resident on the
    device with their camera points; the four calls take turns, each timed with its own pair of events, and the mean over
    `reps` turns is reported."""
    import torch
    from kfnet_amd.KFNet.kabsch import KabschSolver
    from kfnet_amd.KFNet.pnp import PnPSolver
    dev, cam = _pose_records(frames, h, w), _pose_cam_points(frames, h, w)
    kabsch, kabsch_w = KabschSolver(h, w), KabschSolver(h, w, weighted=True)
    pnp, pnp_w = PnPSolver(h, w), PnPSolver(h, w, weighted=True)
    calls = {'pnp_solve': lambda: pnp.solve(dev), 'kabsch_solve': lambda: kabsch.solve(dev, cam),
             'pnp_solve_unc_weighted': lambda: pnp_w.solve_unc(dev),
             'kabsch_solve_unc_weighted': lambda: kabsch_w.solve_unc(dev, cam)}
    total = {name: 0.0 for name in calls}
    for turn in range(max(warmup, 1) + reps):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if turn >= max(warmup, 1):
                total[name] += e0.elapsed_time(e1)
    return {name: round(v / reps, 3) for name, v in total.items()}


def time_pose_stage(frames, reps, warmup, h=60, w=80):
    """ms per call of solve / solve_unc (weighted 0, 1) on `frames` synthetic 60x80 records resident on the device."""
    import torch
    from kfnet_amd.KFNet.pnp import PnPSolver
    dev = _pose_records(frames, h, w)
    calls = {'solve': PnPSolver(h, w).solve, 'solve_unc': PnPSolver(h, w).solve_unc,
             'solve_unc_weighted': PnPSolver(h, w, weighted=True).solve_unc}
    ms = {}
    for name, call in calls.items():
        for _ in range(max(warmup, 1)):
            call(dev)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call(dev)
        e1.record()
        e1.synchronize()
        ms[name] = round(e0.elapsed_time(e1) / reps, 3)
    return ms


def time_pose_track(reps, warmup, shapes=((1, 1000), (8, 500), (64, 64))):
    """{'SxT': {call: ms}}: kfn_pose_filter and kfn_pose_track on S random-walk sequences of T frames (1 cm per frame,
    measurements of 2 cm and 0.3 degrees that all pass the gate), resident on the device; the calls take turns, each
    timed with its own pair of events, and the mean over `reps` turns is reported."""
    import numpy as np
    import torch
    from kfnet_amd.KFNet.pose_filter import PoseFilter, PoseTracker
    rng = np.random.default_rng(0)
    out = {}
    for S, T in shapes:
        poses = np.tile(np.eye(4, dtype=np.float32), (S, T, 1, 1))
        poses[..., :3, 3] = np.cumsum(rng.normal(scale=0.01, size=(S, T, 3)), axis=1) + rng.normal(scale=0.02, size=(S, T, 3))
        cov = np.tile(np.diag([0.005 ** 2] * 3 + [0.02 ** 2] * 3).astype(np.float32), (S, T, 1, 1))
        p, c = torch.from_numpy(poses).cuda(), torch.from_numpy(cov).cuda()
        trackers = {'%s%s' % (m, '+rts' if sm else ''): PoseTracker(m, smooth=sm)
                    for m in ('walk', 'velocity') for sm in (False, True)}

        def tracked(tr):
            tr.reset()
            return tr.run(p, c)
        calls = {'pose_filter': lambda: PoseFilter().run(p, c)}
        calls.update({name: (lambda tr=tr: tracked(tr)) for name, tr in trackers.items()})
        total = {name: 0.0 for name in calls}
        for turn in range(max(warmup, 1) + reps):
            for name, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                if turn >= max(warmup, 1):
                    total[name] += e0.elapsed_time(e1)
        out['%dx%d' % (S, T)] = {name: round(v / reps, 3) for name, v in total.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, nargs='+', default=[4])
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--engines', nargs='+', default=['scoordnet', 'oflownet', 'kfnet'])
    a = ap.parse_args()
    import numpy as np
    import torch
    from kfnet_amd.engine import KFNetEngine, OFlowNetEngine, SCoordNetEngine
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    from kfnet_amd.weights import synthetic_weights
    W = synthetic_weights(1234)
    size = (a.height, a.width)
    frames = synthetic_sequence(a.frames, a.height, a.width)
    T4 = np.linalg.inv(synthetic_transform())
    makers = {
        'scoordnet': lambda B: SCoordNetEngine(W, image_size=size, batch=B, transform=T4, max_chunk=a.frames),
        'oflownet': lambda B: OFlowNetEngine(W, image_size=size, batch=B, max_chunk=a.frames),
        'kfnet': lambda B: KFNetEngine(W, image_size=size, batch=B, transform=T4, max_chunk=a.frames),
    }
    out = {'frames': a.frames, 'image': list(size), 'reps': a.reps, 'fps': {}}
    if 'pose' in a.engines:
        a.engines.remove('pose')
        out['pose_ms'] = time_pose_stage(a.frames, a.reps, a.warmup)
        out['pose_sampling_ms'] = time_pose_sampling(a.frames, a.reps, a.warmup)
        out['pose_depth_ms'] = time_pose_depth(a.frames, a.reps, a.warmup)
        out['pose_track_ms'] = time_pose_track(a.reps, a.warmup)
    for name in a.engines:
        out['fps'][name] = {}
        for B in a.batch:
            eng = makers[name](B)
            dev = eng.upload_frames(frames)
            for _ in range(a.warmup):
                eng.process(dev)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                eng.process(dev)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / a.reps
            out['fps'][name][str(B)] = round(a.frames / (ms * 1e-3), 1)
            del eng, dev
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
