"""Times `process()` of SCoordNetEngine, OFlowNetEngine and KFNetEngine on the same synthetic frames (device events, after
warm-up) and prints one JSON line with frames/s per engine and batch.

    python tools/mb_modes.py [--batch 4 [8 16 ...]] [--frames 64] [--reps 3] [--warmup 1] [--height 480 --width 640]

Every engine is built with random weights and max_chunk = --frames; a timed repetition is one process() of the whole
resident chunk (KFNetEngine: heavy phase on two streams + the Kalman scan; the single-network engines: their network +
the record launch).  Several --batch values show where an engine stops scaling with the batch.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


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
