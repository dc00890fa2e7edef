"""Host-side file helpers with the semantics of the reference's tools/io.py."""
import glob
import os
import re


def read_lines(filepath):
    """tools/io.py:208-212: one stripped line per entry."""
    with open(filepath) as fin:
        lines = fin.readlines()
    return [line.strip() for line in lines]


def snapshot_step(path):
    """The step of a snapshot: the last number in the base name of the .npz file or the checkpoint's `.index` file
    without its extension (tools/io.py:166-183, sorted_ls_by_num), i.e. of a checkpoint prefix as it is; 0 when there
    is none."""
    base = os.path.basename(path)
    if base.endswith(('.npz', '.index')):
        base = os.path.splitext(base)[0]
    nums = re.findall(r'\d+', base)
    return int(nums[-1]) if nums else 0


def get_snapshot(folder):
    """tools/io.py:185-196 picks the newest `model.ckpt-N` (and chdir()s -- not reproduced).
    Here a model folder holds TF V2 checkpoints `model.ckpt-<step>.index` (+ `.data-*`, read by kfnet_amd.checkpoint)
    and/or this project's containers `kfnet_weights.npz` / `kfnet_weights-<step>.npz` keyed by TF variable names
    (kfnet_amd/weights.py).  The highest step over both kinds wins; on a tie the .npz does.  Returns (path, step): the
    .npz file, or for a checkpoint its prefix `.../model.ckpt-<step>` as the reference returns it; (None, 0) when the
    folder holds neither."""
    npz = glob.glob(os.path.join(folder, 'kfnet_weights*.npz'))
    ckpt = [p[:-len('.index')] for p in glob.glob(os.path.join(folder, 'model.ckpt-*.index'))]
    if not npz and not ckpt:
        return None, 0
    best = max([(snapshot_step(p), 1, p) for p in npz] + [(snapshot_step(p), 0, p) for p in ckpt],
               key=lambda c: c[:2])
    return best[2], best[0]


def confident_points(npy_file, thres=20.0):
    """What the downstream consumers do with a `coord_<i>.npy` record
    (vis/vis_scene_coordinate_map.py:10-26, and the PnP step of README.md:132-138): load the
    float32 [h,w,4] map, split scene coordinates (channels 0-2) from the confidence
    (channel 3 = 1/sigma) and keep the points whose confidence exceeds `thres`.
    Returns (points [n,3], pixel indices [n,2] as (row, col))."""
    import numpy as np
    rec = np.load(npy_file)
    if rec.ndim != 3 or rec.shape[2] != 4:
        raise ValueError('%s: expected a [h,w,4] scene-coordinate map, got %s' % (npy_file, rec.shape))
    keep = rec[:, :, 3] > thres
    return rec[:, :, 0:3][keep], np.argwhere(keep)
