"""SCoordNet's single-frame scene coordinates with the reference README's "Test SCoordNet" command line:

    python -m kfnet_amd.SCoordNet.eval --input_folder I --output_folder O --model_folder M --scene S

I holds image_list.txt (+ optional label_list.txt) and transform.txt; for every image one `coord_<i>.npy` float32 [h,w,4] =
(T.x, 1/sigma) of SCoordNet's measurement is written to O -- the file contract of kfnet_amd.KFNet.eval, and bit for bit
the record KFNet writes on a reset frame (kfn_coord_records).  Only SCoordNet runs (kfnet_amd.engine.SCoordNetEngine); the
model folder's newest snapshot (a TF checkpoint model.ckpt-<step> or a kfnet_weights*.npz) may hold just the ScoreNet/*
scope.  `--synthetic T` / `--random_weights` replace the images / the checkpoint; `--pose` also writes pose_<i>.txt
(modes.write_poses); `--pose_weighted` is --pose with the refinement weighted by the records' uncertainty, and also writes
pose_cov_<i>.txt; `--pose_smooth` (single-process runs) is --pose_weighted, and at the end the poses are tracked under
`--pose_motion` (walk) and smoothed backwards in sequences of `--pose_sequence_length` frames (default: the whole run), into
pose_smooth_<i>.txt (modes.write_smoothed_poses); `--pose_sampling confidence | confidence2 [--pose_confidence_cap]` draws
--pose's hypotheses by the records' confidence (DESIGN.md 5c "Guided sampling"), in the sharded runs too; `--pose_depth`
implies --pose and solves every frame from its records and its depth map of depth_list.txt in --input_folder (RANSAC-Kabsch,
DESIGN.md 5c "Poses with depth"), composing with --pose_weighted and --pose_smooth, sharded runs included.
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

FORMAT = '%d, frame %d, d_m = %.3f'


def format_line(m):
    return FORMAT % (m['i'], m['i'], m['d_m'])


def _engine(weights, transform, image_size, batch, max_chunk, emit_metrics, device):
    import torch
    from ..engine import SCoordNetEngine
    if device is None:
        device = 'cuda:%d' % torch.cuda.current_device()
    return SCoordNetEngine(weights, image_size=image_size, batch=batch, transform=transform, max_chunk=max_chunk,
                           emit_metrics=emit_metrics, device=device)


def eval(image_paths, transform, weights, output_folder, image_size=(480, 640), batch=4, frames=None, chunk=256,
         verbose=True, label_paths=None, labels=None, device=None, engine=None, decode_workers=None):
    """Runs the sequence and writes coord_<i>.npy files; returns the records [T,h,w,4].  With label maps (label_list.txt,
    or `labels` [T,H,W,4] in memory) every frame's d_m line and the summary are printed and (records, metrics) returned;
    d_m is reduced on the device by kfn_eval_metrics with the measurement in the meas / temp / KF roles and label pair
    (i, i)."""
    want_metrics = label_paths is not None or labels is not None
    T = len(image_paths) if frames is None else frames.shape[0]
    eng = engine if engine is not None else _engine(weights, transform, image_size, batch, max(1, min(chunk, T)),
                                                    want_metrics, device)
    if want_metrics and not eng.emit_metrics:
        raise ValueError('labels given, but the engine was built without emit_metrics')
    outs = modes.chunk_outputs(eng, T, None, label_paths, modes.diagonal_pairs, labels=labels)
    records, metrics = modes.run_streamed(eng, frames if frames is not None else image_paths, image_size, output_folder,
                                          'coord', chunk=chunk, outputs=outs, metric_format=format_line,
                                          summary_keys=('d_m',), verbose=verbose, decode_workers=decode_workers)
    return (records, metrics) if want_metrics else records


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--input_folder', default='')
    ap.add_argument('--output_folder', default='')
    ap.add_argument('--model_folder', default='')
    ap.add_argument('--scene', default='')
    modes.add_project_flags(ap)
    modes.add_pose_flags(ap)
    return ap


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    pose = modes.pose_argument(a, ap)
    rank, world, local = modes.sharded_env()
    if world > 1 and a.pose_smooth:
        return modes.refuse_sharded_smooth(world)
    if a.scene not in modes.SCENES:
        print('Invalid scene:', a.scene)
        return 1
    from ..dist import launched
    if world > 1 and a.pose and not launched():
        return modes.refuse_unlaunched('--pose', world, 'kfnet_amd.SCoordNet.eval')
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
            paths, label_paths = modes.read_inputs(a.input_folder)
        except (OSError, ValueError) as e:
            print(e, file=sys.stderr)
            return 1
        if world > 1 and label_paths is not None and not launched():
            return modes.refuse_unlaunched('label_list.txt', world, 'kfnet_amd.SCoordNet.eval')
        transform = modes.get_transform(os.path.join(a.input_folder, 'transform.txt'))
        T = len(paths)
        frames_of = modes.image_frames_of(paths, size)
        if rank == 0:
            modes.print_banner(T, a.scene)
    if world > 1:
        return _main_sharded(a, W, size, rank, world, local, T, transform, frames_of, label_paths, pose)
    torch.cuda.set_device(a.gpu)
    out = eval(paths, transform, W, a.output_folder, image_size=size, batch=a.batch,
               frames=frames_of(0, T) if paths is None else None, label_paths=label_paths, device='cuda:%d' % a.gpu)
    if a.pose:
        smooth = dict(motion=a.pose_motion, sequence_length=a.pose_sequence_length or 0) if a.pose_smooth else None
        modes.write_poses(out[0] if label_paths is not None else out, a.output_folder, pose=pose, smooth=smooth)
    return 0


def _main_sharded(a, W, size, rank, world, local, T, transform, frames_of, label_paths, pose=False):
    """One rank of torch.distributed.run: its contiguous chunk through modes.run_shard.  No rank talks to another unless
    labels or --pose ask for the per-frame results on rank 0: only then is a process group started (modes.rank_group)."""
    import torch
    from ..dist import chunk_bounds
    lo, hi = chunk_bounds(T, world, rank)

    def run():
        eng = _engine(W, transform, size, a.batch, max(hi - lo, 1), label_paths is not None, None)
        outs = modes.chunk_outputs(eng, T, a.output_folder, label_paths, modes.diagonal_pairs, pose)
        return modes.run_shard(eng, frames_of, T, rank, world, a.output_folder, 'coord', outputs=outs)

    if label_paths is None and not a.pose:
        modes.rank_device(local)
        run()
        torch.cuda.synchronize()
        return 0
    with modes.rank_group(rank, world, local) as (dist, _):
        modes.report_sharded(dist, [run()], T, rank, format_line if label_paths is not None else None,
                             summary_keys=('d_m',), pose=a.pose)
    return 0


if __name__ == '__main__':
    sys.exit(main())
