"""Host side of the three eval programs, `python -m kfnet_amd.{KFNet,SCoordNet,OFlowNet}.eval` (the reference README's
KFNet prediction, "Test SCoordNet" and "Test OFlowNet"): reading an input folder, output file names, the
streamed single-process run, the frame-sharded runs with their per-rank set-up, and what a run computes from its records
besides the files (label metrics, poses).  The engines are kfnet_amd.engine.KFNetEngine / SCoordNetEngine / OFlowNetEngine.

File contracts (float32 .npy, one per frame, [h,w,C] on the label grid h = ceil(H/8), w = ceil(W/8)):
  coord_<i>.npy  [h,w,4] = (T.x, 1/sigma): KFNet's filtered estimate, or SCoordNet's measurement
  flow_<i>.npy   [h,w,3] = (u, v, 1/sigma_trans) for the pair (i-1, i), i = 1..N-1: cell (r, c) of frame i comes from
                 cell (r + v, c + u) of frame i-1 (grid cells); flow_list.txt lists them in order, so line k pairs with
                 images k and k+1 of image_list.txt (vis/vis_optical_flow_list.py's arguments)
  pose_<i>.txt   --pose: the camera-to-world pose solved from coord_<i>.npy (kfnet_amd/KFNet/pnp.py); --pose_depth: from
                 coord_<i>.npy and the frame's depth map of depth_list.txt (kfnet_amd/KFNet/kabsch.py)
  pose_cov_<i>.txt   --pose_weighted: that pose refined with the records' uncertainty as weights, and its 6x6 covariance
  pose_smooth_<i>.txt   --pose_smooth: the --pose_weighted poses tracked and smoothed in time (single-process runs)
"""
import contextlib
import os
import sys
import time

import numpy as np

from .tools.io import read_lines

SCENES = ('chess', 'fire', 'heads', 'office', 'pumpkin', 'redkitchen', 'stairs')
FLOW_LIST = 'flow_list.txt'
POSE_BATCH = 64     # frames per kfn_pnp_ransac launch (--pose)


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


def _is_dir(output_folder):
    return bool(output_folder) and os.path.isdir(output_folder)


def save_records(output_folder, kind, lo, rec):
    """Write the files of records rec [n,h,w,C] of frames [lo, lo + n) (the reference eval loop, eval.py:121-126)."""
    rec = np.ascontiguousarray(rec, dtype=np.float32)       # once per chunk, not per frame: the writer threads share the GIL
    for i, name in output_files(kind, lo, rec.shape[0]):
        np.save(os.path.join(output_folder, name), rec[i - lo])


def _decode_workers():
    """Decode threads of the library (kfn_decode_png_rgb8): a chunk's files side by side."""
    return max(4, min(32, (os.cpu_count() or 8) // 2))


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def get_transform(transform_file=None):
    """KFNet/train.py:49-58."""
    if transform_file:
        transform = np.loadtxt(transform_file, dtype=np.float32)
        return np.linalg.inv(transform)
    return np.eye(4, dtype=np.float32)


def load_images(paths, image_size, workers=None):
    """tf.image.decode_png(channels=3) replacement (KFNet/train.py:213-217): the library's threaded decoder
    (kfn_decode_png_rgb8 through pipeline.decode_png_batch), PIL where the library is not built."""
    from .pipeline import _native_png_available, decode_image, decode_png_batch
    H, W = image_size
    out = np.empty((len(paths), H, W, 3), dtype=np.uint8)
    if _native_png_available():
        decode_png_batch(list(paths), out, image_size, workers or _decode_workers())
        return out
    for i, p in enumerate(paths):
        out[i] = decode_image(p, image_size)
    return out


def read_inputs(input_folder, check=True):
    """(image paths, label paths or None) of an input folder: image_list.txt, and label_list.txt when it is there, which
    must then list one label per image (the reference eval loop, eval.py:37); ValueError otherwise, unless `check` is off."""
    image_paths = read_lines(os.path.join(input_folder, 'image_list.txt'))
    label_list = os.path.join(input_folder, 'label_list.txt')
    label_paths = read_lines(label_list) if os.path.exists(label_list) else None
    if check and label_paths is not None and len(label_paths) != len(image_paths):
        raise ValueError('%s lists %d labels for %d images' % (label_list, len(label_paths), len(image_paths)))
    return image_paths, label_paths


def synthetic_frames_of(height, width):
    """frames_of(a, b) of the seeded synthetic sequence (frame t depends on (seed, t) alone: a rank makes only its own)."""
    from .synth import synthetic_sequence

    def frames_of(a, b):
        return synthetic_sequence(b - a, height, width, start=a)
    return frames_of


def image_frames_of(image_paths, image_size, workers=None):
    def frames_of(a, b):
        return load_images(image_paths[a:b], image_size, workers)
    return frames_of


def print_banner(total_frames, scene=None):
    print('----------------------------------')
    if scene is not None:
        print('scene: ', scene)
    print('image number: ', total_frames)
    print('----------------------------------')


# ----------------------------------------------------------------------------------------------------------------------
# what a run computes from its records besides the record files
# ----------------------------------------------------------------------------------------------------------------------
POSE_WEIGHTED = 'weighted'     # the `pose` argument of the run functions for --pose_weighted (True: --pose)


def add_pose_flags(ap):
    ap.add_argument('--pose', action='store_true', help='also write pose_<i>.txt (RANSAC-PnP on the device)')
    ap.add_argument('--pose_weighted', action='store_true',
                    help='--pose with the refinement weighted by the records\' uncertainty; also writes pose_cov_<i>.txt')
    ap.add_argument('--pose_smooth', action='store_true',
                    help='--pose_weighted, and at the end the poses are tracked and smoothed backwards in time '
                         '(kfn_pose_track); writes pose_smooth_<i>.txt.  Single-process runs only')
    ap.add_argument('--pose_motion', choices=['walk', 'velocity'], default=None,
                    help='--pose_smooth: the tracker\'s motion model (walk)')
    ap.add_argument('--pose_sequence_length', type=int, default=None,
                    help='--pose_smooth: frames per tracked sequence (the run\'s Kalman reset period where the program '
                         'has one, otherwise the whole run)')
    ap.add_argument('--pose_sampling', choices=['uniform', 'confidence', 'confidence2'], default=None,
                    help='--pose: draw every hypothesis\' cells uniformly (the default), or in proportion to the records\' '
                         'confidence above the threshold (confidence) or to its square (confidence2)')
    ap.add_argument('--pose_confidence_cap', type=float, default=None,
                    help='--pose_sampling confidence / confidence2: confidences above it weigh as it does (1000)')
    ap.add_argument('--pose_depth', action='store_true',
                    help='--pose from the records and the frames\' depth maps (RANSAC-Kabsch, KFNet/kabsch.py): reads '
                         'depth_list.txt from --input_folder, as `labels make` writes it')


class DepthPoseOptions(object):
    """The run functions' `pose` for a --pose_depth run: the run's depth maps, one path per frame."""

    def __init__(self, weighted, depth_paths):
        self.weighted, self.depth_paths = bool(weighted), list(depth_paths)


class DepthPoseSolver(object):
    """--pose_depth's solver: a KabschSolver (KFNetDataSpec intrinsics) over a run's depth list, with PnPSolver's calling
    shape.  The frames of a call are the global frames t0, t0 + 1, ..: their depth maps are decoded here, by whichever
    process solves them, so a sharded rank reads its own frames' depth alone."""

    def __init__(self, h, w, depth_paths, weighted=False):
        from .KFNet.KFNet import KFNetDataSpec
        from .KFNet.kabsch import KabschSolver
        from .labels import DepthCamera
        spec = KFNetDataSpec()
        self.solver = KabschSolver(h, w, DepthCamera(spec.focal_x, spec.focal_y, spec.u, spec.v), weighted=weighted)
        self.weighted, self.depth_paths = bool(weighted), list(depth_paths)

    def _depth(self, n, t0):
        from .labels import load_depth
        if t0 + n > len(self.depth_paths):
            raise ValueError('depth_list.txt lists %d depth maps; frame %d has none' % (len(self.depth_paths), t0 + n - 1))
        return load_depth(self.depth_paths[t0:t0 + n], (8 * self.solver.h, 8 * self.solver.w))

    def solve(self, records, t0=0):
        return self.solver.solve(records, self._depth(int(records.shape[0]), t0), t0=t0)

    def solve_unc(self, records, t0=0):
        return self.solver.solve_unc(records, self._depth(int(records.shape[0]), t0), t0=t0)


class PoseOptions(object):
    """The run functions' `pose` for a --pose run with guided sampling: what pose_solver needs besides the grid."""

    def __init__(self, weighted, sampling, confidence_cap):
        self.weighted, self.sampling, self.confidence_cap = bool(weighted), sampling, float(confidence_cap)


def pose_argument(a, ap=None):
    """The parsed flags -> the run functions' `pose`; --pose_smooth implies --pose_weighted, which implies --pose (a.pose
    is set).  With the parser `ap`, --pose_motion / --pose_sequence_length without --pose_smooth, and --pose_sampling /
    --pose_confidence_cap without --pose or one of its stronger forms, are argparse errors.  The sampling counter is the
    global frame index, so the sharded runs take the two sampling flags unchanged."""
    guided = getattr(a, 'pose_sampling', None) not in (None, 'uniform')
    depth_paths = None
    if getattr(a, 'pose_depth', False):
        a.pose = True
        path = os.path.join(getattr(a, 'input_folder', '') or '', 'depth_list.txt')
        problem = ('--pose_depth draws three cells uniformly: --pose_sampling %s belongs to PnP' % a.pose_sampling if guided
                   else None if os.path.isfile(path) else '--pose_depth needs depth_list.txt in --input_folder (%s)' % path)
        if problem is not None:
            if ap is None:
                raise ValueError(problem)
            ap.error(problem)
        depth_paths = [p for p in read_lines(path) if p]
    if ap is not None:
        for name in ('pose_sampling', 'pose_confidence_cap'):
            if getattr(a, name) is not None and not (a.pose or a.pose_weighted or a.pose_smooth):
                ap.error('--%s needs --pose' % name)
        if a.pose_confidence_cap is not None and not guided:
            ap.error('--pose_confidence_cap needs --pose_sampling confidence or confidence2')
        if guided:
            try:
                pose_solver(1, 1, sampling=a.pose_sampling,
                            confidence_cap=1000. if a.pose_confidence_cap is None else a.pose_confidence_cap)
            except ValueError as e:
                ap.error('--pose_confidence_cap: %s' % e)
        for name in ('pose_motion', 'pose_sequence_length'):
            if getattr(a, name) is not None and not a.pose_smooth:
                ap.error('--%s needs --pose_smooth' % name)
        if a.pose_sequence_length is not None and a.pose_sequence_length < 1:
            ap.error('--pose_sequence_length must be >= 1')
    if a.pose_smooth:
        a.pose_weighted = True
    if a.pose_weighted:
        a.pose = True
    if depth_paths is not None:
        return DepthPoseOptions(a.pose_weighted, depth_paths)
    if guided and a.pose:
        return PoseOptions(a.pose_weighted, a.pose_sampling,
                           1000. if a.pose_confidence_cap is None else a.pose_confidence_cap)
    return POSE_WEIGHTED if a.pose_weighted else a.pose


def refuse_sharded_smooth(world):
    """Exit status 1, after one line, for --pose_smooth in a sharded run (WORLD_SIZE > 1): the tracker runs over whole
    sequences, which no rank holds.  Called before any device is initialised."""
    print('--pose_smooth is not supported in the sharded run (WORLD_SIZE=%d): run one process, or smooth the written '
          'poses with python -m kfnet_amd.KFNet.pnp --smooth --rts' % world, file=sys.stderr)
    return 1


def pose_solver(h, w, weighted=False, sampling='uniform', confidence_cap=1000.):
    """--pose's RANSAC-PnP solver for an h x w record grid: the KFNetDataSpec intrinsics."""
    from .KFNet.KFNet import KFNetDataSpec
    from .KFNet.pnp import PnPSolver
    spec = KFNetDataSpec()
    return PnPSolver(h, w, spec.focal_x, spec.focal_y, spec.u, spec.v, weighted=weighted, sampling=sampling,
                     confidence_cap=confidence_cap)


def solver_of(pose, h, w):
    """The run functions' `pose` -> its solver: True or POSE_WEIGHTED or a PoseOptions (pose_solver), a DepthPoseOptions
    (DepthPoseSolver), a PnPSolver (itself), anything false (None)."""
    if isinstance(pose, DepthPoseOptions):
        return DepthPoseSolver(h, w, pose.depth_paths, pose.weighted)
    if isinstance(pose, PoseOptions):
        return pose_solver(h, w, pose.weighted, pose.sampling, pose.confidence_cap)
    if pose is True or pose == POSE_WEIGHTED:
        return pose_solver(h, w, pose == POSE_WEIGHTED)
    return pose or None


def write_smoothed_poses(poses, cov, output_folder, motion=None, sequence_length=0):
    """--pose_smooth of a single-process run: the run's poses [T,4,4] and covariances [T,6,6] (the 52 floats per frame that
    --pose_weighted writes) cut into sequences of `sequence_length` frames (0: one), each tracked from a fresh state and
    smoothed backwards (PoseTracker(motion, smooth=True)); pose_smooth_<i>.txt.  Returns the smoothed poses [T,4,4]."""
    from .KFNet.pnp import smooth_in_sequences, write_pose
    from .KFNet.pose_filter import PoseTracker
    smooth = smooth_in_sequences(PoseTracker(motion or 'walk', smooth=True), poses, cov, sequence_length or 0)[4]
    if _is_dir(output_folder):
        for i in range(poses.shape[0]):
            write_pose(os.path.join(output_folder, 'pose_smooth_%d.txt' % i), smooth[i])
    return smooth


def write_poses(records, output_folder, batch=POSE_BATCH, pose=True, smooth=None):
    """--pose of a single-process run: camera-to-world poses of the in-memory records [T,h,w,4] (KFNetDataSpec
    intrinsics), pose_<i>.txt next to coord_<i>.npy; pose = POSE_WEIGHTED: the weighted refinement, and pose_cov_<i>.txt;
    `smooth` (with POSE_WEIGHTED): write_smoothed_poses' keyword arguments for --pose_smooth.
    Returns (poses [T,4,4], info [T,4])."""
    from .KFNet.pnp import solve_in_batches, solve_unc_in_batches, write_covariance, write_pose
    solver = solver_of(pose, records.shape[1], records.shape[2])
    if solver.weighted:
        poses, cov, _, info = solve_unc_in_batches(solver, records, batch)
    else:
        poses, info = solve_in_batches(solver, records, batch)
    if _is_dir(output_folder):
        for i in range(records.shape[0]):
            write_pose(os.path.join(output_folder, 'pose_%d.txt' % i), poses[i])
            if solver.weighted:
                write_covariance(os.path.join(output_folder, 'pose_cov_%d.txt' % i), cov[i])
    print('poses: %d of %d frames solved' % (int((info[:, 0] == 0).sum()), records.shape[0]))
    if smooth is not None:
        if not solver.weighted:
            raise ValueError('smoothing needs the covariances of pose = POSE_WEIGHTED')
        write_smoothed_poses(poses, cov, output_folder, **smooth)
    return poses, info


def diagonal_pairs(lo, n):
    """SCoordNet's label pairs: frame i against label i."""
    return np.repeat(np.arange(lo, lo + n)[:, None], 2, axis=1)


class ChunkOutputs(object):
    """What a run computes on the device from a chunk's frames, right behind its scan and before the next heavy phase
    reuses the engine's buffers: the label metrics (kfn_eval_metrics over the engine's c_meas / c_temp / c_kf / c_nis; the
    engine is built with emit_metrics) and, in the sharded runs, the --pose camera poses (kfn_pnp_ransac on the device
    records view, POSE_BATCH frames per launch with t0 = the global frame index, as write_poses).  Both are per frame and
    deterministic, so a frame's numbers do not depend on how the sequence was cut.
    Labels: `label_paths` (label_list.txt of the whole sequence) or `labels` [T,H,W,4] in memory; `pairs_of(lo, n)`: the
    label pairs (global indices) of frames [lo, lo + n) -- every label row they refer to is read here, a neighbouring
    chunk's or rank's included.  `pose`: True or POSE_WEIGHTED (pose_solver) or a PnPSolver; a solver with `weighted` set
    goes through solve_unc and also writes pose_cov_<i>.txt.  The files go to `output_folder` when it is a directory.
    The streamed run double-buffers the metrics (`launch` into slot k & 1 from StreamedSequence's after_process, `collect`
    of that slot when chunk k's records are out); a sharded rank does everything for a chunk at once (`add`, slot 0)."""

    def __init__(self, eng, total_frames, output_folder=None, label_paths=None, pairs_of=None, pose=False, labels=None):
        from .KFNet import metrics as M
        self.eng, self.T, self.output_folder = eng, int(total_frames), output_folder
        self.label_paths, self.labels, self.pairs_of = label_paths, labels, pairs_of
        self.has_metrics = label_paths is not None or labels is not None
        self.dm = M.DeviceMetrics(eng) if self.has_metrics else None
        self.solver = solver_of(pose, eng.h, eng.w)
        self.plan = {}      # slot -> (first, n, global pairs) of the launch it holds

    def _label_grid(self, i):
        from .KFNet import metrics as M
        if self.labels is not None:
            return M.resize_nearest(self.labels[i], (self.eng.h, self.eng.w))
        return M.read_label_grid(self.label_paths[i], (self.eng.H, self.eng.W), (self.eng.h, self.eng.w))

    def launch(self, slot, lo, n):
        """Right behind the scan of frames [lo, lo + n): label grids of the frames their pairs refer to -> device,
        kfn_eval_metrics, results -> pinned host slot `slot`."""
        from .KFNet.metrics import label_rows
        pairs = self.pairs_of(lo, n)
        rows, local = label_rows(lo, pairs, self.T, self._label_grid)
        self.dm.launch(slot, lo, n, rows, local)
        self.plan[slot] = (lo, n, pairs)

    def collect(self, slot):
        """One dict per frame of the launch in `slot` (metrics.DeviceMetrics.collect)."""
        lo, n, pairs = self.plan.pop(slot)
        return self.dm.collect(slot, lo, n, pairs)

    def add(self, lo, rec):
        """Frames [lo, lo + n) whose scan has just been enqueued; `rec` = the engine's device records view [n,h,w,4].
        Returns {'metrics': [one dict per frame] or None, 'poses': [n,4,4] float32 or None, 'info': [n,4] int32
        (PnPSolver.solve) or None} and writes pose_<i>.txt."""
        from .KFNet.pnp import write_covariance, write_pose
        n = int(rec.shape[0])
        res = {'metrics': None, 'poses': None, 'info': None}
        if self.has_metrics and n:
            self.launch(0, lo, n)
        if self.solver is not None:
            res['poses'] = np.zeros((0, 4, 4), np.float32)
            res['info'] = np.zeros((0, 4), np.int32)
            cov = None
            if n and self.solver.weighted:
                torch = self.eng.torch
                parts = [self.solver.solve_unc(rec[k:k + POSE_BATCH], t0=lo + k) for k in range(0, n, POSE_BATCH)]
                res['poses'] = torch.cat([p[0] for p in parts]).cpu().numpy()
                res['info'] = torch.cat([p[3] for p in parts]).cpu().numpy()
                cov = torch.cat([p[1] for p in parts]).cpu().numpy()
            elif n:
                torch = self.eng.torch
                parts = [self.solver.solve(rec[k:k + POSE_BATCH], t0=lo + k) for k in range(0, n, POSE_BATCH)]
                res['poses'] = torch.cat([p for p, _ in parts]).cpu().numpy()
                res['info'] = torch.cat([i for _, i in parts]).cpu().numpy()
            if _is_dir(self.output_folder):
                for k in range(n):
                    write_pose(os.path.join(self.output_folder, 'pose_%d.txt' % (lo + k)), res['poses'][k])
                    if cov is not None:
                        write_covariance(os.path.join(self.output_folder, 'pose_cov_%d.txt' % (lo + k)), cov[k])
        if self.has_metrics:
            res['metrics'] = self.collect(0) if n else []
        return res


def chunk_outputs(eng, total_frames, output_folder, label_paths, pairs_of, pose=False, labels=None):
    """ChunkOutputs, or None when there are neither labels nor --pose."""
    if label_paths is None and labels is None and not pose:
        return None
    return ChunkOutputs(eng, total_frames, output_folder, label_paths, pairs_of, pose, labels)


def print_metrics(metrics, metric_format):
    for m in metrics:
        print(metric_format(m))


# ----------------------------------------------------------------------------------------------------------------------
# the runs
# ----------------------------------------------------------------------------------------------------------------------
def run_streamed(eng, source, image_size, output_folder, kind, chunk=256, outputs=None, metric_format=None,
                 summary_keys=('d_m', 'd_t', 'd_kf'), verbose=True, save_workers=2, decode_workers=None, ramp=None,
                 stats=None):
    """One process: `source` (image paths or a uint8 [T,H,W,3] array) through ChunkLoader (decode thread + pinned staging:
    the reference's queue runners, KFNet/train.py:195-239) -> StreamedSequence (uploads / compute / downloads overlapped
    on three streams) -> `eng`; the record files are written behind the loop when `output_folder` is a directory.
    `outputs`: a ChunkOutputs with labels; every frame's metric line (`metric_format`, a function of a metrics dict) and
    the closing summary over `summary_keys` are printed, a `frames a~b done` line per chunk otherwise (`verbose`).
    `ramp`: lengths of the first chunks (default (8, 16) in front of chunks of >= 32 frames: the first decode is exposed,
    keep it short, and let each ramp chunk's compute cover the next one's decode -- pipeline.ChunkLoader).  `stats`: a
    dict that receives where the consumer thread's wall time went (StreamedSequence.stats + `emit` and `saves_wait`
    seconds + the loader's `producer` times).
    Returns (records [T,h,w,C], metrics: one dict per frame, or None without labels)."""
    from concurrent.futures import ThreadPoolExecutor
    from .KFNet.metrics import summary_lines
    from .pipeline import ChunkLoader, StreamedSequence
    chunk = min(int(chunk), eng.max_chunk)
    want_metrics = outputs is not None and outputs.has_metrics
    # written off the consumer thread: the next chunk's records can be fetched while the previous chunk's 76.8 KB files are
    # still going to disk (np.save releases the GIL in the file write)
    saver = ThreadPoolExecutor(max(1, int(save_workers))) if _is_dir(output_folder) else None
    pending, records, metrics = [], [], ([] if want_metrics else None)
    # chunks in flight on the GPU: 3 (a second chunk queued behind the running one); the metrics reduction double-buffers
    # its results, so it keeps 2.  The loader rotates one host buffer more than that: a buffer is recycled only after the
    # records of the chunk that was uploaded from it have been handed out, i.e. its upload is complete.
    in_flight = 2 if want_metrics else 3
    loader = ChunkLoader(source if isinstance(source, np.ndarray) else list(source), image_size, chunk,
                         workers=decode_workers or _decode_workers(),
                         first_chunk=[r for r in ((8, 16) if ramp is None else ramp) if r < chunk], depth=in_flight + 1)
    seq = StreamedSequence(eng, chunk, depth=in_flight)
    after_process = (lambda k, lo, n: outputs.launch(k & 1, lo, n)) if want_metrics else None
    t_emit = 0.0
    try:
        for k, (lo, rec) in enumerate(seq.run(loader, after_process=after_process)):
            t_e = time.perf_counter()
            rec = rec.copy()
            records.append(rec)
            if saver is not None:
                pending.append(saver.submit(save_records, output_folder, kind, lo, rec))
            t_emit += time.perf_counter() - t_e
            if want_metrics:
                ms = outputs.collect(k & 1)
                metrics += ms
                if verbose:
                    print_metrics(ms, metric_format)
            elif verbose:
                print('frames %d~%d done' % (lo, lo + rec.shape[0] - 1))
        t_e = time.perf_counter()
        for f in pending:
            f.result()          # re-raise write errors; every file is on disk on return
        if stats is not None:
            stats.update(getattr(seq, 'stats', {}), emit=t_emit, saves_wait=time.perf_counter() - t_e,
                         producer={key: round(v, 4) for key, v in getattr(loader, 'stats', {}).items()})
    finally:
        if saver is not None:   # also when the loop raised: no writer thread outlives the call
            saver.shutdown()
    records = np.concatenate(records) if records else np.zeros((0, eng.h, eng.w, eng.record_channels), np.float32)
    if verbose and metrics:
        for line in summary_lines(metrics, summary_keys):
            print(line)
    return records, metrics


def run_shard(eng, frames_of, total_frames, rank, world, output_folder, kind, verbose=True, outputs=None, link=None):
    """Frame-sharded run (BASELINE config 4; contiguous chunks, kfnet_amd.dist.chunk_bounds): this rank runs [lo, hi)
    through dist.run_chunk -- the state-independent heavy phase at once, primed with frame lo - 1 where the engine's pairing
    rule asks for it; a KFNetEngine then receives the [h,w,4] Kalman state from rank - 1 over `link` (unless its chunk
    starts on a reset frame), scans and sends the state on; the single-network engines carry no state and need no link
    -- and writes the files of its own frames.  `frames_of(a, b)` returns uint8 host frames [a, b).
    Returns (lo, records [hi-lo,h,w,C]); with `outputs` (a ChunkOutputs: the chunk's metrics and poses, right behind the
    scan) (lo, records, results) with ChunkOutputs.add's results."""
    from .dist import chunk_bounds, handoff_period, needs_state, run_chunk
    lo, hi = chunk_bounds(total_frames, world, rank)
    if outputs is not None and kind != 'coord':
        raise ValueError('label metrics and poses need coordinate records, not %r' % kind)
    need_prev = 1 if (hi > lo and needs_state(lo, handoff_period(eng))) else 0
    if hi > lo:
        dev = eng.upload_frames(frames_of(lo - need_prev, hi))
    else:       # an empty chunk still forwards the state it receives
        dev = eng.torch.empty((0, eng.H, eng.W, 3), dtype=eng.torch.uint8, device=eng.device)
    rec = run_chunk(eng, dev[need_prev:], lo, rank, world, link, dev[0] if need_prev else None)
    res = outputs.add(lo, rec) if outputs is not None else None
    rec = rec.cpu().numpy().copy()
    if _is_dir(output_folder):
        save_records(output_folder, kind, lo, rec)
    if verbose:
        print('rank %d/%d: frames %d~%d done' % (rank, world, lo, hi - 1))
    return (lo, rec) if outputs is None else (lo, rec, res)


def run_shard_cyclic(eng, frames_of, total_frames, block, rank, world, link, output_folder, kind, verbose=True,
                     outputs=None):
    """Block-cyclic frame sharding (kfnet_amd.dist.run_cyclic): blocks of `block` frames dealt round-robin, block j on rank
    j % world; the Kalman state hops rank -> rank+1 once per block, so a rank scans its block while the others are still in
    the heavy phase of theirs.  Same records, bit for bit, as run_shard and as a single process.  `frames_of` as in
    run_shard: only this rank's blocks (+ the frame in front of each) are ever decoded / uploaded.
    Returns [(first_frame, records [n,h,w,C])] of this rank's blocks; with `outputs` (each block's metrics and poses,
    computed inside on_block, before the next block's heavy phase reuses the engine's buffers)
    [(first_frame, records, results)]."""
    from .dist import run_cyclic
    out = []

    def on_block(lo, rec):
        res = outputs.add(lo, rec) if outputs is not None else None
        r = rec.cpu().numpy().copy()
        if _is_dir(output_folder):
            save_records(output_folder, kind, lo, r)
        out.append((lo, r) if outputs is None else (lo, r, res))

    run_cyclic(eng, lambda a, b: eng.upload_frames(frames_of(a, b)), total_frames, int(block), rank, world, link,
               on_block=on_block)
    if verbose:
        print('rank %d/%d: %d blocks of %d frames done (block-cyclic)' % (rank, world, len(out), block))
    return out


def report_sharded(dist, parts, total, rank, metric_format=None, summary_keys=('d_m', 'd_t', 'd_kf'), pose=False):
    """What the single-process run prints behind its records, printed by rank 0 of a sharded run from the per-frame
    results of every rank (dist.gather_frames, one collective that every rank joins): each frame's metric line in frame
    order and the summary (`metric_format`, a function of a metrics dict), then the pose count (`pose`).  `parts`: this
    rank's [(first_frame, records, ChunkOutputs.add results)]."""
    from .dist import gather_frames
    from .KFNet.metrics import summary_lines
    items = []
    for lo, rec, res in parts:
        for k in range(rec.shape[0]):
            items.append((lo + k, (res['metrics'][k] if res['metrics'] is not None else None,
                                   int(res['info'][k, 0]) if res['info'] is not None else None)))
    got = gather_frames(dist, items)
    if rank != 0:
        return
    if len(got) != total:
        raise RuntimeError('gathered the results of %d frames, expected %d' % (len(got), total))
    if metric_format is not None:
        ms = [m for m, _ in got]
        print_metrics(ms, metric_format)
        if ms:
            for line in summary_lines(ms, summary_keys):
                print(line)
    if pose:
        print('poses: %d of %d frames solved' % (sum(1 for _, st in got if st == 0), total))


# ----------------------------------------------------------------------------------------------------------------------
# one process per GPU under torch.distributed.run
# ----------------------------------------------------------------------------------------------------------------------
def sharded_env():
    """(rank, world, device index) under torch.distributed.run; (0, 1, None) otherwise."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    return rank, world, (local if world > 1 else None)


def refuse_unlaunched(what, world, module):
    """Exit status 2 for a sharded run (WORLD_SIZE > 1) that needs a process group to gather per-frame results onto rank
    0 -- `what` = '--pose' or 'label_list.txt' -- but was not started by torch.distributed.run (dist.launched)."""
    print('%s is not supported in the sharded run without torch.distributed.run (WORLD_SIZE=%d, but MASTER_PORT is '
          'unset): rank 0 gathers the per-frame results over torch.distributed.  Start it with python -m '
          'torch.distributed.run --nproc-per-node N -m %s ...' % (what, world, module), file=sys.stderr)
    return 2


def rank_device(local):
    """Make GPU LOCAL_RANK current (ranks share GPUs when there are fewer GPUs than ranks).  Returns (device index,
    number of GPUs)."""
    import torch
    ndev = torch.cuda.device_count()
    dev_index = local % max(ndev, 1)
    torch.cuda.set_device(dev_index)
    return dev_index, ndev


@contextlib.contextmanager
def rank_group(rank, world, local, state_link=False):
    """The process group of a torch.distributed.run rank on its device (rank_device, dist.init_group), with the Kalman state
    link of KFNet's hand-over when `state_link` (dist.make_link, KFN_STATE_LINK).  Yields (torch.distributed, link or
    None); a body that ends without an error is followed by a device synchronize and a barrier, and the link and the group
    are closed in any case."""
    import torch
    import torch.distributed as dist
    from .dist import init_group, make_link
    dev_index, ndev = rank_device(local)
    init_group(dist, rank, world, dev_index, ndev)
    link = make_link(dist, rank, world, dev_index, prefer=os.environ.get('KFN_STATE_LINK', 'auto')) if state_link else None
    try:
        yield dist, link
        torch.cuda.synchronize()
        dist.barrier()
    finally:
        if link is not None:
            link.close()
        dist.destroy_process_group()


def add_project_flags(ap):
    """The flags this project adds to the reference's command lines."""
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
