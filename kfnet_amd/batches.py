"""Where the batches of `python -m kfnet_amd.SCoordNet.train` come from: seeded synthetic data, image and label files, or
images with depth maps and poses.  The three sources are plain classes with one shape: `count` frames, `transform` (the 4x4
of transform.txt itself), `poses` ([count,4,4] camera to world, or None: what the reprojection term reads) and
batch(indices, full_resolution) -> (frames uint8 [n,H,W,3], labels [n,H,W,4] if full_resolution
else [n,H/8,W/8,4]).  Which labels a step needs is the trainer's to say (SCoordNetTrainer.needs_full_resolution).  Opening a
source touches no device: a missing list or a label file of the wrong size is refused before torch initialises one."""
import os

import numpy as np

from . import labels as L, modes
from .KFNet.metrics import read_label_grid
from .train import synthetic_labels


def _grid(size):
    return size[0] // 8, size[1] // 8


class SyntheticSource(object):
    """`count` frames of kfnet_amd.synth's sequence with train.synthetic_labels, for runs without data."""

    def __init__(self, count, size):
        from .synth import synthetic_poses, synthetic_sequence, synthetic_transform
        self.count, self.size = count, size
        self.transform = synthetic_transform()
        self.poses = synthetic_poses(count)
        self.frames = synthetic_sequence(count, size[0], size[1])
        self._labels = {}          # full_resolution -> [count,h,w,4], made when first asked for

    def batch(self, indices, full_resolution):
        if full_resolution not in self._labels:
            self._labels[full_resolution] = synthetic_labels(self.count, self.size if full_resolution else _grid(self.size))
        return self.frames[indices], self._labels[full_resolution][indices]


class LabelFileSource(object):
    """image_list.txt, label_list.txt (one [H,W,4] float32 file per image) and transform.txt of an input folder."""

    def __init__(self, input_folder, size, needs_transform=True, needs_poses=False):
        self.paths, self.label_paths = modes.read_inputs(input_folder)
        if self.label_paths is None:
            raise ValueError('%s has no label_list.txt: training needs labels' % input_folder)
        self.poses = None
        if needs_poses:
            from .reproj import read_pose_list
            self.poses = read_pose_list(input_folder)
            if len(self.poses) != len(self.paths):
                raise ValueError('pose_list.txt of %s lists %d poses for %d images' % (input_folder, len(self.poses), len(self.paths)))
        # stage 2's loss is invariant under the rigid transform: OFlowNet.train neither needs nor reads the file
        self.transform = np.loadtxt(os.path.join(input_folder, 'transform.txt'), dtype=np.float32) if needs_transform else None
        self.count, self.size = len(self.paths), size

    def label(self, i, full_resolution):
        """Label i: the pixels the loss reads, or the whole file, between whose pixels augmentation interpolates."""
        path, (H, W) = self.label_paths[i], self.size
        if not full_resolution:
            return read_label_grid(path, self.size, _grid(self.size))
        lab = np.fromfile(path, dtype=np.float32)
        if lab.size != H * W * 4:
            raise ValueError('%s holds %d floats, --augment needs the full-resolution label of %d' % (path, lab.size, H * W * 4))
        return lab.reshape(H, W, 4)

    def batch(self, indices, full_resolution):
        frames = modes.load_images([self.paths[i] for i in indices], self.size)
        return frames, np.stack([self.label(i, full_resolution) for i in indices])


class DepthSource(object):
    """image_list.txt, depth_list.txt, pose_list.txt and transform.txt of an input folder (what `python -m kfnet_amd.labels
    make --no_labels` writes): every batch's labels are made on the device from its 16-bit depth maps and poses (DESIGN.md
    6d), and stay there.  The DepthLabeler, and with it the device, is made at the first batch."""

    def __init__(self, input_folder, size, batch_size, camera, device):
        for name in L.LISTS + ('transform.txt',):
            if not os.path.exists(os.path.join(input_folder, name)):
                raise ValueError('%s has no %s: --depth needs %s and transform.txt' % (input_folder, name, ', '.join(L.LISTS)))
        self.triples = L.read_sequence(input_folder)
        self.transform = np.loadtxt(os.path.join(input_folder, 'transform.txt'), dtype=np.float32)
        self.poses = L.read_poses([t[2] for t in self.triples])
        self.count, self.size = len(self.triples), size
        self.batch_size, self.camera, self.device = batch_size, camera, device
        self._labelers = {}        # full_resolution -> DepthLabeler at stride 1 or 8

    def batch(self, indices, full_resolution):
        if full_resolution not in self._labelers:
            self._labelers[full_resolution] = L.DepthLabeler(self.batch_size, self.size[0], self.size[1],
                                                             1 if full_resolution else 8, self.camera, self.device)
        frames = modes.load_images([self.triples[i][0] for i in indices], self.size)
        depth = L.load_depth([self.triples[i][1] for i in indices], self.size)
        return frames, self._labelers[full_resolution].labels(depth, self.poses[indices])


def open_source(a, full_resolution, needs_transform=True, needs_poses=False):
    """The source that the parsed arguments of SCoordNet.train ask for (needs_transform = False: OFlowNet.train's, whose label
    files go without transform.txt; needs_poses: the run has the reprojection term on, so a folder of label files must hold
    pose_list.txt too).  ValueError or OSError, with the message for the
    user, when the arguments or the folder do not make one; with `full_resolution` the first label file is read here, so
    that grid-sized label files are refused at once."""
    size = (a.height, a.width)
    if a.depth and a.synthetic > 0:
        raise ValueError('--depth reads depth maps and poses from --input_folder: it does not go with --synthetic')
    if a.synthetic > 0:
        return SyntheticSource(a.synthetic, size)
    if a.depth:
        return DepthSource(a.input_folder, size, a.batch, L.camera_of(a), 'cuda:%d' % a.gpu)
    source = LabelFileSource(a.input_folder, size, needs_transform, needs_poses)
    if full_resolution:
        source.label(0, True)
    return source
