"""Host side shared by the single-network programs, `python -m kfnet_amd.SCoordNet.eval` and `python -m kfnet_amd.OFlowNet.eval`
(the reference README's "Test SCoordNet" and "Test OFlowNet"): output file names, the streamed single-process
run and the frame-sharded run.  The engines are kfnet_amd.engine.SCoordNetEngine / OFlowNetEngine.

File contracts (float32 .npy, one per frame, [h,w,C] on the label grid h = ceil(H/8), w = ceil(W/8)):
  coord_<i>.npy  [h,w,4] = (T.x, 1/sigma) of SCoordNet's measurement -- KFNet eval's contract
  flow_<i>.npy   [h,w,3] = (u, v, 1/sigma_trans) for the pair (i-1, i), i = 1..N-1: cell (r, c) of frame i comes from
                 cell (r + v, c + u) of frame i-1 (grid cells); flow_list.txt lists them in order, so line k pairs with
                 images k and k+1 of image_list.txt (vis/vis_optical_flow_list.py's arguments)
"""
import os
import sys

import numpy as np

FLOW_LIST = 'flow_list.txt'


def coord_name(i):
    return 'coord_%d.npy' % i


def flow_name(i):
    return 'flow_%d.npy' % i


def output_files(kind, lo, n):
    """[(frame, file name)] written for the records of frames [lo, lo + n): every frame for 'coord'; for 'flow' every
    frame but the sequence's first, whose row has no predecessor."""
    if kind == 'coord':
        return [(i, coord_name(i)) for i in range(lo, lo + n)]
    if kind == 'flow':
        return [(i, flow_name(i)) for i in range(max(lo, 1), lo + n)]
    raise ValueError('unknown record kind %r' % kind)


def flow_list_lines(output_folder, total_frames):
    """The lines of flow_list.txt: the flow files of frames 1..total_frames-1, in order, as absolute paths."""
    folder = os.path.abspath(output_folder)
    return [os.path.join(folder, flow_name(i)) for i in range(1, total_frames)]


def write_flow_list(output_folder, total_frames):
    path = os.path.join(output_folder, FLOW_LIST)
    with open(path, 'w') as f:
        for line in flow_list_lines(output_folder, total_frames):
            f.write(line + '\n')
    return path


def save_records(output_folder, kind, lo, rec):
    """Write the files of records rec [n,h,w,C] of frames [lo, lo + n)."""
    for i, name in output_files(kind, lo, rec.shape[0]):
        np.save(os.path.join(output_folder, name), np.ascontiguousarray(rec[i - lo], dtype=np.float32))


def _decode_workers():
    return max(4, min(32, (os.cpu_count() or 8) // 2))


def run_streamed(eng, source, image_size, output_folder, kind, chunk=256, after_process=None, on_chunk=None, in_flight=3,
                 save_workers=2, decode_workers=None, ramp=(8, 16)):
    """One process: `source` (image paths or a uint8 [T,H,W,3] array) through ChunkLoader -> StreamedSequence -> `eng`;
    the record files are written behind the loop when `output_folder` is a directory.  `after_process(k, lo, n)` is
    called behind chunk k's compute (on the compute stream), `on_chunk(k, lo, rec)` when its records are on the host.
    Returns the records [T,h,w,C]."""
    from concurrent.futures import ThreadPoolExecutor
    from .pipeline import ChunkLoader, StreamedSequence
    chunk = min(int(chunk), eng.max_chunk)
    saver = ThreadPoolExecutor(max(1, int(save_workers))) if (output_folder and os.path.isdir(output_folder)) else None
    pending, records = [], []
    loader = ChunkLoader(source if isinstance(source, np.ndarray) else list(source), image_size, chunk,
                         workers=decode_workers or _decode_workers(), first_chunk=[r for r in ramp if r < chunk],
                         depth=in_flight + 1)
    seq = StreamedSequence(eng, chunk, depth=in_flight)
    try:
        for k, (lo, rec) in enumerate(seq.run(loader, after_process=after_process)):
            rec = rec.copy()
            records.append(rec)
            if saver is not None:
                pending.append(saver.submit(save_records, output_folder, kind, lo, rec))
            if on_chunk is not None:
                on_chunk(k, lo, rec)
        for f in pending:
            f.result()          # re-raise write errors; every file is on disk on return
    finally:
        if saver is not None:
            saver.shutdown()
    if records:
        return np.concatenate(records)
    return np.zeros((0, eng.h, eng.w, eng.record_channels), np.float32)


def run_shard(eng, frames_of, total_frames, rank, world, output_folder, kind, verbose=True, label_paths=None, pose=False):
    """Frame-sharded run (contiguous chunks, kfnet_amd.dist.chunk_bounds): this rank processes [lo, hi) through
    dist.run_chunk -- which primes an OFlowNetEngine with frame lo - 1 -- and writes its own files.  No rank talks to
    another: neither network carries state from frame to frame.  `frames_of(a, b)` returns uint8 frames [a, b).
    Returns (lo, records [hi-lo,h,w,C]).
    SCoordNet (kind 'coord') only: `label_paths` (the whole sequence's list; the engine built with emit_metrics) and / or
    `pose` (True, or a PnPSolver) add the chunk's d_m metrics -- label pair (i, i), as SCoordNet.eval -- and poses
    (kfnet_amd.KFNet.eval.ShardOutputs, right behind the records launch) and return (lo, records, results)."""
    from .dist import chunk_bounds, handoff_period, needs_state, run_chunk
    lo, hi = chunk_bounds(total_frames, world, rank)
    outs = None
    if label_paths is not None or pose:
        if kind != 'coord':
            raise ValueError('label metrics and poses need coordinate records, not %r' % kind)
        from .KFNet.eval import ShardOutputs
        outs = ShardOutputs(eng, total_frames, output_folder, label_paths,
                            lambda a, n: np.repeat(np.arange(a, a + n)[:, None], 2, axis=1), pose)
    res = None
    need_prev = 1 if (hi > lo and needs_state(lo, handoff_period(eng))) else 0
    if hi > lo:
        dev = eng.upload_frames(frames_of(lo - need_prev, hi))
        rec = run_chunk(eng, dev[need_prev:], lo, rank, world, None, dev[0] if need_prev else None)
        if outs is not None:
            res = outs.add(lo, rec)
        rec = rec.cpu().numpy().copy()
    else:
        rec = np.zeros((0, eng.h, eng.w, eng.record_channels), np.float32)
        if outs is not None:
            res = outs.add(lo, rec)
    if output_folder and os.path.isdir(output_folder):
        save_records(output_folder, kind, lo, rec)
    if verbose:
        print('rank %d/%d: frames %d~%d done' % (rank, world, lo, hi - 1))
    return (lo, rec) if outs is None else (lo, rec, res)


def sharded_env():
    """(rank, world, device index) under torch.distributed.run; (0, 1, None) otherwise."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    return rank, world, (local if world > 1 else None)


def synthetic_frames_of(height, width):
    """frames_of(a, b) of the seeded synthetic sequence (frame t depends on (seed, t) alone: a rank makes only its own)."""
    from .synth import synthetic_sequence

    def frames_of(a, b):
        return synthetic_sequence(b - a, height, width, start=a)
    return frames_of


def image_frames_of(image_paths, image_size):
    from .KFNet.eval import load_images

    def frames_of(a, b):
        return load_images(image_paths[a:b], image_size)
    return frames_of


def add_project_flags(ap):
    """The flags this project adds to the reference's command lines (as kfnet_amd.KFNet.eval has them)."""
    ap.add_argument('--gpu', type=int, default=0)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--synthetic', type=int, default=0, help='use a seeded synthetic sequence of this many frames')
    ap.add_argument('--random_weights', action='store_true')
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)


def load_weights(a):
    """--random_weights, or the newest snapshot of --model_folder (tools.io.get_snapshot): a kfnet_weights*.npz container
    or a TF V2 checkpoint model.ckpt-<step>, holding the full KFNet or only the program's own scope.  None, after a
    message on stderr, when there is none or it cannot be read."""
    from .tools.io import get_snapshot
    from .weights import load_snapshot, synthetic_weights
    if a.random_weights:
        return synthetic_weights(1234)
    snapshot, _ = get_snapshot(a.model_folder)
    if snapshot is None:
        print('no kfnet_weights*.npz or model.ckpt-*.index in', a.model_folder)
        return None
    try:
        return load_snapshot(snapshot, verbose=os.environ.get('RANK', '0') == '0')
    except (ValueError, OSError) as e:       # checkpoint.CheckpointError is a ValueError
        print('cannot restore %s: %s' % (snapshot, e), file=sys.stderr)
        return None
