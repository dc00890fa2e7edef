"""Per-sequence prediction entry point with the reference's `KFNet/eval.py` command line
and output contract (README.md:126-130, KFNet/eval.py:31-177):

    python -m kfnet_amd.KFNet.eval --input_folder I --output_folder O --model_folder M --scene S [--NIS]

I holds image_list.txt (+ optional label_list.txt) and transform.txt; for every image one
`coord_<index>.npy` float32 [h,w,4] = concat(T.x_KF, 1/sigma_KF) is written to O.
`--synthetic T` replaces the image list by a seeded synthetic sequence (no dataset is
reachable from the build environment); `--random_weights` replaces the checkpoint.

Launched under `python -m torch.distributed.run --nproc-per-node N -m kfnet_amd.KFNet.eval ...`
the sequence is frame-sharded (BASELINE config 4): rank r processes its contiguous chunk on
GPU LOCAL_RANK (falling back to sharing GPUs over gloo when there are fewer GPUs than ranks),
receives the Kalman state from rank r-1 just before its scan and writes its own
coord_<i>.npy files -- bit-identical to a single-process run (kfnet_amd/dist.py).  With labels
and / or --pose every rank also computes its own frames' metrics and poses on its GPU (modes.ChunkOutputs)
and writes their pose_<i>.txt; rank 0 gathers the per-frame results and prints the same metric
lines, summary and pose count as the single-process run (modes.report_sharded).

Host loop semantics kept from eval.py: sequence_length = 500 irrespective of --scene
(KFNetDataSpec() is built with the default scene), reset at i % 500 == 0,
raw (untransformed, ungated) KF state fed back, NIS gate on the output only.
When label_list.txt is present the reference's per-frame log line (losses, accuracies, median
distance errors in cm, NIS-in-band fraction) and the final summary are printed
(kfnet_amd/KFNet/metrics.py).  Not reproduced: --show plotting.
`--pose_weighted` is `--pose` with the refinement weighted by the records' uncertainty; it also writes `pose_cov_<i>.txt`.
`--pose_smooth` (single-process runs) is `--pose_weighted`, and at the end the poses are cut into sequences of
`--pose_sequence_length` frames (default: the reset period, 500), tracked under `--pose_motion` (walk) and smoothed backwards
(kfnet_amd/KFNet/pose_filter.py PoseTracker); it writes `pose_smooth_<i>.txt`.
`--pose` also solves every frame's camera pose on the device (kfnet_amd/KFNet/pnp.py) and writes `pose_<i>.txt` next to
each `coord_<i>.npy`.  `--pose_sampling confidence | confidence2 [--pose_confidence_cap]` draws its hypotheses by the
records' confidence (DESIGN.md 5c "Guided sampling"), in the sharded runs too.  `--pose_depth` implies `--pose` and solves
every frame as a 3-D/3-D alignment of its records with its depth map, read from `depth_list.txt` in `--input_folder` (what
`labels make` writes; kfnet_amd/KFNet/kabsch.py, DESIGN.md 5c "Poses with depth"); it composes with `--pose_weighted` and
`--pose_smooth`, and in the sharded runs every rank decodes its own frames' depth.
"""
import argparse
import os
import sys

import numpy as np

from .. import modes
from ..modes import SCENES, get_transform, load_images  # noqa: F401  (callers reach them through this module)
from . import metrics as M

# eval.py's host loop resets the filter every `spec.sequence_length` frames, and KFNetDataSpec() is built with
# the default scene there: 500 whatever --scene says.  ONE constant for every caller.
RESET_PERIOD = 500


def _engine(weights, transform, nis, image_size, batch, sequence_length, max_chunk, emit_metrics, device):
    import torch
    from ..engine import KFNetEngine
    if device is None:   # --gpu N: everything (buffers, streams, launches) lives on the CURRENT device
        device = 'cuda:%d' % torch.cuda.current_device()
    return KFNetEngine(weights, image_size=image_size, batch=batch, transform=transform, reset_period=sequence_length,
                       nis_gate=7.815 if nis else 0.0, max_chunk=max_chunk, emit_metrics=emit_metrics, device=device)


def _outputs(eng, T, output_folder, label_paths, metrics_sequence_length, pose=False, labels=None):
    return modes.chunk_outputs(eng, T, output_folder, label_paths,
                               lambda lo, n: M.pair_schedule(lo, n, T, metrics_sequence_length), pose, labels)


def eval_sharded(frames_of, total_frames, transform, weights, output_folder, rank, world, link, nis=False,
                 image_size=(480, 640), batch=4, sequence_length=RESET_PERIOD, verbose=True, device=None, label_paths=None,
                 metrics_sequence_length=1000, pose=False):
    """Frame-sharded prediction (modes.run_shard): this rank's contiguous chunk of the `total_frames` frames
    `frames_of(a, b)` returns (uint8 host [b-a,H,W,3]: modes.image_frames_of / synthetic_frames_of), the Kalman state over
    `link`.  Returns (first_frame, records [n,h,w,4]).
    `label_paths` (the whole sequence's label_list.txt) / `pose` (True, or a PnPSolver): the chunk's metrics and poses
    as well; then returns (first_frame, records, results) with modes.ChunkOutputs.add's results."""
    from ..dist import chunk_bounds
    lo, hi = chunk_bounds(total_frames, world, rank)
    eng = _engine(weights, transform, nis, image_size, batch, sequence_length, max(hi - lo, 1), label_paths is not None, device)
    outs = _outputs(eng, total_frames, output_folder, label_paths, metrics_sequence_length, pose)
    return modes.run_shard(eng, frames_of, total_frames, rank, world, output_folder, 'coord', verbose, outs, link)


def eval_sharded_cyclic(frames_of, total_frames, transform, weights, output_folder, rank, world, link, block, nis=False,
                        image_size=(480, 640), batch=4, sequence_length=RESET_PERIOD, verbose=True, device=None,
                        label_paths=None, metrics_sequence_length=1000, pose=False):
    """Block-cyclic frame sharding (modes.run_shard_cyclic), arguments as eval_sharded.  Same records, bit for bit, as
    eval_sharded and as a single process.  Returns [(first_frame, records [n,h,w,4])] of this rank's blocks, with
    `label_paths` / `pose` [(first_frame, records, results)]."""
    eng = _engine(weights, transform, nis, image_size, batch, sequence_length, max(int(block), 1), label_paths is not None,
                  device)
    outs = _outputs(eng, total_frames, output_folder, label_paths, metrics_sequence_length, pose)
    return modes.run_shard_cyclic(eng, frames_of, total_frames, block, rank, world, link, output_folder, 'coord', verbose, outs)


def eval(image_paths, transform, weights, output_folder, nis=False, image_size=(480, 640), batch=4,
         frames=None, sequence_length=RESET_PERIOD, chunk=256, verbose=True, label_paths=None, labels=None,
         decode_workers=None, device=None, metrics_sequence_length=1000, engine=None, save_workers=2, stats=None, ramp=None):
    """Runs the sequence and writes coord_<i>.npy files; returns the [T,h,w,4] records.
    With label maps (label_list.txt, or `labels` [T,H,W,4] in memory) the reference's per-frame
    log line and final median/mean/std summary are printed (KFNet/eval.py:113-118,162-164);
    returns (records, metrics) in that case.  `engine`: a ready KFNetEngine to run on (its batch / max_chunk / transform
    are used; bench.py times the path without the one-off graph build); `save_workers`: threads that write the
    coord_<i>.npy files behind the consumer loop; `stats`, `ramp`, `decode_workers`: as modes.run_streamed."""
    T = len(image_paths) if frames is None else frames.shape[0]
    want_metrics = label_paths is not None or labels is not None
    eng = engine
    if engine is None:
        eng = _engine(weights, transform, nis, image_size, batch, sequence_length, chunk, want_metrics, device)
    else:
        # a supplied engine carries its own settings; an argument that DISAGREES with them must not be dropped silently
        # (eval(..., nis=True, engine=eng_without_gate) used to return ungated records)
        if want_metrics and not eng.emit_metrics:
            raise ValueError('labels given, but the engine was built without emit_metrics')
        if bool(nis) != (eng.nis_gate > 0.0):
            raise ValueError('eval(nis=%r) disagrees with the engine (nis_gate=%g)' % (nis, eng.nis_gate))
        if int(sequence_length) != int(eng.reset_period):
            raise ValueError('eval(sequence_length=%d) disagrees with the engine (reset_period=%d)'
                             % (sequence_length, eng.reset_period))
        if tuple(image_size) != (eng.H, eng.W):
            raise ValueError('eval(image_size=%r) disagrees with the engine (%dx%d)' % (tuple(image_size), eng.H, eng.W))
        t_arg = None if transform is None else np.asarray(transform, dtype=np.float32)
        if (t_arg is None) != (eng.transform is None) or (t_arg is not None and not np.array_equal(t_arg, eng.transform)):
            raise ValueError('eval(transform=...) disagrees with the transform the engine was built with')
    outs = _outputs(eng, T, None, label_paths, metrics_sequence_length, labels=labels)
    records, metrics = modes.run_streamed(eng, frames if frames is not None else image_paths, image_size, output_folder,
                                          'coord', chunk=chunk, outputs=outs, metric_format=M.format_line, verbose=verbose,
                                          save_workers=save_workers, decode_workers=decode_workers, ramp=ramp, stats=stats)
    return (records, metrics) if want_metrics else records


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--input_folder', default='')
    ap.add_argument('--output_folder', default='')
    ap.add_argument('--model_folder', default='')
    ap.add_argument('--scene', default='')
    ap.add_argument('--NIS', action='store_true')
    modes.add_project_flags(ap)
    ap.add_argument('--sharding', choices=['contiguous', 'cyclic'], default='contiguous',
                    help='multi-process runs: contiguous chunks per rank, or blocks of --block frames dealt round-robin')
    ap.add_argument('--block', type=int, default=32, help='--sharding cyclic: frames per block')
    modes.add_pose_flags(ap)
    a = ap.parse_args(argv)
    pose = modes.pose_argument(a, ap)
    rank, world, local = modes.sharded_env()
    if world > 1 and a.pose_smooth:
        return modes.refuse_sharded_smooth(world)
    if a.scene not in SCENES:
        print('Invalid scene:', a.scene)   # KFNet/train.py:142-144
        return 1
    from ..dist import launched
    if world > 1 and a.pose and not launched():
        return modes.refuse_unlaunched('--pose', world, 'kfnet_amd.KFNet.eval')
    inputs = None
    if world > 1 and a.synthetic <= 0:
        # every rank checks its inputs before any engine or collective: a bad folder fails every rank alike
        try:
            inputs = modes.read_inputs(a.input_folder)
        except (OSError, ValueError) as e:
            print(e, file=sys.stderr)
            return 1
        if inputs[1] is not None and not launched():
            return modes.refuse_unlaunched('label_list.txt', world, 'kfnet_amd.KFNet.eval')
    W = modes.load_weights(a)
    if W is None:
        return 1
    size = (a.height, a.width)
    if a.synthetic > 0:
        from ..synth import synthetic_transform
        T, image_paths, label_paths = a.synthetic, None, None
        transform = np.linalg.inv(synthetic_transform())
        frames_of = modes.synthetic_frames_of(a.height, a.width)
    else:
        image_paths, label_paths = inputs if inputs is not None else modes.read_inputs(a.input_folder, check=False)
        T = len(image_paths)
        frames_of = modes.image_frames_of(image_paths, size)
        if world == 1:
            modes.print_banner(T, a.scene)
            if label_paths is not None:
                assert len(image_paths) == len(label_paths)   # KFNet/eval.py:37
        transform = get_transform(os.path.join(a.input_folder, 'transform.txt'))
    kw = dict(image_size=size, batch=a.batch, label_paths=label_paths,
              metrics_sequence_length=M.TEST_SEQUENCE_LENGTH.get(a.scene, 1000))
    if world > 1:
        if a.gpu != 0 and rank == 0:
            print('WARNING: --gpu %d is ignored under torch.distributed.run: rank r uses device LOCAL_RANK' % a.gpu,
                  file=sys.stderr)
        with modes.rank_group(rank, world, local, state_link=True) as (dist, link):
            if a.sharding == 'cyclic':
                parts = eval_sharded_cyclic(frames_of, T, transform, W, a.output_folder, rank, world, link, a.block, a.NIS,
                                            pose=pose, **kw)
            else:
                parts = [eval_sharded(frames_of, T, transform, W, a.output_folder, rank, world, link, a.NIS, pose=pose,
                                      **kw)]
            if label_paths is not None or a.pose:
                modes.report_sharded(dist, parts, T, rank, M.format_line if label_paths is not None else None, pose=a.pose)
        return 0
    import torch
    torch.cuda.set_device(a.gpu)
    out = eval(image_paths, transform, W, a.output_folder, a.NIS, frames=frames_of(0, T) if image_paths is None else None,
               device='cuda:%d' % a.gpu, **kw)
    if a.pose:
        smooth = dict(motion=a.pose_motion, sequence_length=a.pose_sequence_length or RESET_PERIOD) if a.pose_smooth else None
        modes.write_poses(out[0] if label_paths is not None else out, a.output_folder, pose=pose, smooth=smooth)
    return 0


if __name__ == '__main__':
    sys.exit(main())
