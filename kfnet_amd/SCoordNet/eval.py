"""SCoordNet's single-frame scene coordinates with the reference README's "Test SCoordNet" command line:

    python -m kfnet_amd.SCoordNet.eval --input_folder I --output_folder O --model_folder M --scene S

I holds image_list.txt (+ optional label_list.txt) and transform.txt; for every image one `coord_<i>.npy` float32 [h,w,4] =
(T.x, 1/sigma) of SCoordNet's measurement is written to O -- the file contract of kfnet_amd.KFNet.eval, and bit for bit
the record KFNet writes on a reset frame (kfn_coord_records).  Only SCoordNet runs (kfnet_amd.engine.SCoordNetEngine); the
model folder's newest snapshot (a TF checkpoint model.ckpt-<step> or a kfnet_weights*.npz) may hold just the ScoreNet/*
scope.  `--synthetic T` / `--random_weights` replace the images / the checkpoint; `--pose` also writes pose_<i>.txt
(kfnet_amd.KFNet.eval.write_poses).
With label_list.txt every frame's median distance error d_m (cm) is printed, then the median / mean / stddev over d_m.

Under `python -m torch.distributed.run --nproc-per-node N -m kfnet_amd.SCoordNet.eval ...` every rank processes a
contiguous chunk of the frames and writes its own files, bit-identical to a single-process run.  With labels or --pose
each rank also computes its frames' d_m and poses on its GPU (modes.run_shard) and writes their pose_<i>.txt; a process
group is started only then, and rank 0 gathers the per-frame results and prints the single-process run's d_m lines and
summary.
"""
import argparse
import os
import sys

import numpy as np

from .. import modes
from ..KFNet.eval import SCENES, get_transform, read_inputs, refuse_unlaunched, write_poses

FORMAT = '%d, frame %d, d_m = %.3f'


def eval(image_paths, transform, weights, output_folder, image_size=(480, 640), batch=4, frames=None, chunk=256,
         verbose=True, label_paths=None, labels=None, device=None, engine=None, decode_workers=None):
    """Runs the sequence and writes coord_<i>.npy files; returns the records [T,h,w,4].  With label maps (label_list.txt,
    or `labels` [T,H,W,4] in memory) every frame's d_m line and the summary are printed and (records, metrics) returned;
    d_m is reduced on the device by kfn_eval_metrics with the measurement in the meas / temp / KF roles and label pair
    (i, i)."""
    from ..engine import SCoordNetEngine
    from ..KFNet import metrics as M
    want_metrics = label_paths is not None or labels is not None
    if device is None:
        import torch
        device = 'cuda:%d' % torch.cuda.current_device()
    T = len(image_paths) if frames is None else frames.shape[0]
    eng = engine if engine is not None else SCoordNetEngine(weights, image_size=image_size, batch=batch, transform=transform,
                                                            max_chunk=max(1, min(chunk, T)), emit_metrics=want_metrics,
                                                            device=device)
    if want_metrics and not eng.emit_metrics:
        raise ValueError('labels given, but the engine was built without emit_metrics')
    dm = M.DeviceMetrics(eng) if want_metrics else None
    all_metrics, plan = [], {}

    def label_grid(i):
        if labels is not None:
            return M.resize_nearest(labels[i], (eng.h, eng.w))
        return M.read_label_grid(label_paths[i], image_size, (eng.h, eng.w))

    def after_process(k, lo, n):
        rows = np.stack([label_grid(i) for i in range(lo, lo + n)])
        local = np.repeat(np.arange(n)[:, None], 2, axis=1)
        dm.launch(k & 1, lo, n, rows, local)
        plan[k] = (lo, n, local + lo)

    def on_chunk(k, lo, rec):
        if want_metrics:
            first, n, pairs = plan.pop(k)
            for m in dm.collect(k & 1, first, n, pairs):
                all_metrics.append(m)
                if verbose:
                    print(FORMAT % (m['i'], m['i'], m['d_m']))
        elif verbose:
            print('frames %d~%d done' % (lo, lo + rec.shape[0] - 1))

    records = modes.run_streamed(eng, frames if frames is not None else image_paths, image_size, output_folder, 'coord',
                                 chunk=chunk, after_process=after_process if want_metrics else None, on_chunk=on_chunk,
                                 in_flight=2 if want_metrics else 3, decode_workers=decode_workers)
    if not want_metrics:
        return records
    if verbose and all_metrics:
        for name, fn in (('Median dist error: ', np.median), ('Mean dist error: ', np.mean), ('stddev error: ', np.std)):
            print(name, fn([m['d_m'] for m in all_metrics]))
    return records, all_metrics


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--input_folder', default='')
    ap.add_argument('--output_folder', default='')
    ap.add_argument('--model_folder', default='')
    ap.add_argument('--scene', default='')
    modes.add_project_flags(ap)
    ap.add_argument('--pose', action='store_true', help='also write pose_<i>.txt (RANSAC-PnP on the device)')
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    rank, world, local = modes.sharded_env()
    if a.scene not in SCENES:
        print('Invalid scene:', a.scene)
        return 1
    from ..dist import launched
    if world > 1 and a.pose and not launched():
        return refuse_unlaunched('--pose', world, 'kfnet_amd.SCoordNet.eval')
    W = modes.load_weights(a)
    if W is None:
        return 1
    import torch
    size = (a.height, a.width)
    if a.synthetic > 0:
        from ..synth import synthetic_transform
        transform = np.linalg.inv(synthetic_transform())
        T, paths, label_paths = a.synthetic, None, None
        frames_of = modes.synthetic_frames_of(a.height, a.width)
    else:
        try:        # on every rank of a sharded run, before any engine or collective
            paths, label_paths = read_inputs(a.input_folder)
        except (OSError, ValueError) as e:
            print(e, file=sys.stderr)
            return 1
        if world > 1 and label_paths is not None and not launched():
            return refuse_unlaunched('label_list.txt', world, 'kfnet_amd.SCoordNet.eval')
        transform = get_transform(os.path.join(a.input_folder, 'transform.txt'))
        T = len(paths)
        frames_of = modes.image_frames_of(paths, size)
        if rank == 0:
            print('----------------------------------')
            print('scene: ', a.scene)
            print('image number: ', T)
            print('----------------------------------')
    if world > 1:
        return _main_sharded(a, W, size, rank, world, local, T, transform, frames_of, label_paths)
    torch.cuda.set_device(a.gpu)
    device = 'cuda:%d' % a.gpu
    out = eval(paths, transform, W, a.output_folder, image_size=size, batch=a.batch,
               frames=frames_of(0, T) if paths is None else None, label_paths=label_paths, device=device)
    if a.pose:
        write_poses(out[0] if label_paths is not None else out, a.output_folder)
    return 0


def _main_sharded(a, W, size, rank, world, local, T, transform, frames_of, label_paths):
    """One rank of torch.distributed.run: its contiguous chunk through modes.run_shard.  No rank talks to another unless
    labels or --pose ask for the per-frame results on rank 0: only then is a process group started (backend as
    kfnet_amd.KFNet.eval's sharded run)."""
    import torch
    from ..engine import SCoordNetEngine
    from ..dist import chunk_bounds, init_group
    ndev = torch.cuda.device_count()
    dev_index = local % max(ndev, 1)
    torch.cuda.set_device(dev_index)
    lo, hi = chunk_bounds(T, world, rank)
    if label_paths is None and not a.pose:
        eng = SCoordNetEngine(W, image_size=size, batch=a.batch, transform=transform, max_chunk=max(hi - lo, 1),
                              device='cuda:%d' % torch.cuda.current_device())
        modes.run_shard(eng, frames_of, T, rank, world, a.output_folder, 'coord')
        torch.cuda.synchronize()
        return 0
    import torch.distributed as dist
    from ..KFNet.eval import report_sharded
    init_group(dist, rank, world, dev_index, ndev)
    try:
        eng = SCoordNetEngine(W, image_size=size, batch=a.batch, transform=transform, max_chunk=max(hi - lo, 1),
                              emit_metrics=label_paths is not None, device='cuda:%d' % torch.cuda.current_device())
        part = modes.run_shard(eng, frames_of, T, rank, world, a.output_folder, 'coord', label_paths=label_paths,
                               pose=a.pose)
        report_sharded(dist, [part], T, rank, (lambda m: FORMAT % (m['i'], m['i'], m['d_m']))
                       if label_paths is not None else None, summary_keys=('d_m',), pose=a.pose)
        torch.cuda.synchronize()
        dist.barrier()
    finally:
        dist.destroy_process_group()
    return 0


if __name__ == '__main__':
    sys.exit(main())
