"""The camera tracked against the TSDF volume: RGB-D sequences fused without poses.

Someone who records a room with an RGB-D camera has frame-*.color.png and frame-*.depth.png and no frame-*.pose.txt.  This
module finds the poses: the volume `kfnet_amd.fuse` builds is the model, a ray cast from the last pose gives its surface, the
new depth map is aligned to it by projective point-to-plane ICP on a pyramid, and the frame is integrated under the pose
found -- KinectFusion's loop, every step a launch of csrc/kfn_track.hip or kfn_fuse_integrate, nothing read back in between.

    python -m kfnet_amd.track make --sequence S --output_folder O [--first_pose FILE] [--mesh scene.ply]
                                   [--voxel 0.02] [--trunc T] [--bounds x0 y0 z0 x1 y1 z1 | --extent 4.0] [--min_weight 2]
                                   [--no_color] [--focal_x 525 --focal_y 525 --u 320 --v 240]
                                   [--depth_focal_x F --depth_focal_y F --depth_u U --depth_v V]
                                   [--height 480 --width 640] [--gpu 0]
                                   [--dist_max 0.1] [--angle_max 20] [--levels 3] [--iterations 10 5 4]
                                   [--reloc [--reloc_ferns 500 --reloc_keyframes 1024 --reloc_harvest 0.2 --reloc_tries 3
                                             --reloc_seed 1 --reloc_min_share S --reloc_max_rms M]]

writes frame-<i>.pose.txt for every tracked frame, image_list.txt, depth_list.txt and pose_list.txt naming the tracked frames
(so O is a --sequence for `fuse make`, `labels make` and `render make`), track_report.txt and, with --mesh, the volume's mesh.
With --reloc a lost tracker is relocalised from fern-coded keyframes (csrc/kfn_reloc.hip): track_report.txt names a recovered
frame `relocalised`, reloc_report.txt lists every frame's nearest keyframe, and the summary line counts keyframes and recoveries.

    trk = Tracker(volume, levels=3, iterations=(10, 5, 4))     iterations finest to coarsest; the coarsest level runs first
    trk.start(first_pose, depth_u16, frame_u8)                 the committed pose, and frame 0 integrated under it
    trk.push(depth_u16, frame_u8)                              one frame: maps, ray casts, 19 iterations, commit, integrate
    poses, lost, diagnostics = trk.trajectory()                the one read
    trk = Tracker(volume, reloc=True)                          or reloc=dict(ferns=500, ...): Relocaliser's keywords
    rows, keyframes, key_poses = trk.relocalisation()          the relocaliser's one read

There is no fallback: a missing entry point or an unsupported shape raises.
"""
import argparse
import ctypes as C
import math
import os
import sys

import numpy as np

from . import _lib
from .labels import add_camera_flags, camera_of, load_depth, pose_rows, read_frames
from .staging import check_size, current_stream

DIAGNOSTICS = ('lost', 'pairs', 'share', 'rms', 'accepted', 'iterations', 'step_m', 'step_rad')
MAX_LEVELS = 4


def track_descriptor(camera, dims, origin, voxel, trunc, image_size, levels=3, level=0, near=0.05, far=8.0, min_weight=1.0,
                     pyr_dist=0.1, jump=0.1, dist_max=0.1, angle_max=20.0, min_pairs=50, pivot_floor=1e-10, min_share=0.1,
                     max_rms=0.04, max_step_m=0.3, max_step_rad=0.35, traj_rows=1, slot=0):
    """kfn_track_desc: every constant rounded from fp64 to fp32 once (ctypes does the rounding); cos_min from angle_max in
    degrees."""
    d = _lib.TrackDesc(nx=dims[0], ny=dims[1], nz=dims[2], H=image_size[0], W=image_size[1], levels=levels, level=level,
                       raw_min=camera.raw_min, raw_max=camera.raw_max, min_pairs=min_pairs, traj_rows=traj_rows, slot=slot)
    d.ox, d.oy, d.oz = origin
    d.voxel, d.trunc, d.near, d.far, d.scale, d.min_weight = voxel, trunc, near, far, camera.scale, min_weight
    d.dfx, d.dfy, d.du, d.dv = camera.depth_fx, camera.depth_fy, camera.depth_u, camera.depth_v
    d.pyr_dist, d.jump, d.dist_max, d.cos_min, d.pivot_floor = pyr_dist, jump, dist_max, math.cos(math.radians(angle_max)), pivot_floor
    d.min_share, d.max_rms, d.max_step_m, d.max_step_rad = min_share, max_rms, max_step_m, max_step_rad
    return d


def level_sizes(image_size, levels):
    """[(H_l, W_l, offset in quadruples)]: the size halves (floor)."""
    H, W = image_size
    out, off = [], 0
    for _ in range(levels):
        out.append((H, W, off))
        off += H * W
        H, W = H // 2, W // 2
    return out


def check_levels(image_size, levels, iterations):
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError('levels must lie in 1 .. %d, got %d' % (MAX_LEVELS, levels))
    iterations = tuple(int(x) for x in iterations)
    if len(iterations) != levels:
        raise ValueError('%d iteration counts for %d levels: one a level, finest first' % (len(iterations), levels))
    if min(iterations) < 0 or sum(iterations) < 1:
        raise ValueError('the iteration counts must be non-negative and not all zero, got %s' % (iterations,))
    H, W = image_size
    if H < 1 or W < 1 or (H >> (levels - 1)) < 2 or (W >> (levels - 1)) < 2:
        raise ValueError('%d levels leave the coarsest of %dx%d below 2x2' % (levels, H, W))
    return iterations


def pose_record(committed, estimate=None, frame=1):
    """kfn_track_state as the host writes it: both poses [4,4], [3,4] or [12], fp64."""
    def row(p):
        p = np.asarray(p, dtype=np.float64)
        p = p[:3, :] if p.shape == (4, 4) else p
        if p.size != 12:
            raise ValueError('a pose must be [4,4], [3,4] or [12], got %s' % (p.shape,))
        return p.reshape(12)
    st = _lib.TrackState()
    st.committed = (C.c_double * 12)(*row(committed))
    st.estimate = (C.c_double * 12)(*row(committed if estimate is None else estimate))
    st.frame = frame
    return st


def fern_table(seed, ferns, level_size, colour=False, depth_lo=0.5, depth_hi=4.0):
    """The fern table of kfn_reloc_encode, int32 [ferns, 4], from a seeded numpy Generator: a position (x, y) on the level of
    `level_size` = (H_l, W_l), the bits of a float32 depth threshold uniform in [depth_lo, depth_hi] metres, and -- with
    `colour` -- three uint8 thresholds packed R + 256 G + 65536 B (0 without)."""
    Hl, Wl = level_size
    if not 1 <= ferns <= _lib.RELOC_MAX_FERNS:
        raise ValueError('ferns must lie in 1 .. %d, got %r' % (_lib.RELOC_MAX_FERNS, ferns))
    if Hl < 1 or Wl < 1:
        raise ValueError('the level must hold a pixel, got %dx%d' % (Hl, Wl))
    if not 0.0 < depth_lo <= depth_hi < float('inf'):
        raise ValueError('the depth thresholds need 0 < depth_lo <= depth_hi, got %r .. %r' % (depth_lo, depth_hi))
    rng = np.random.default_rng([int(seed), 0xfe525])
    table = np.zeros((ferns, 4), dtype=np.int32)
    table[:, 0] = rng.integers(0, Wl, size=ferns)
    table[:, 1] = rng.integers(0, Hl, size=ferns)
    table[:, 2] = rng.uniform(depth_lo, depth_hi, size=ferns).astype(np.float32).view(np.int32)
    rgb = rng.integers(0, 256, size=(ferns, 3))
    if colour:
        table[:, 3] = rgb[:, 0] + 256 * rgb[:, 1] + 65536 * rgb[:, 2]
    return table


class Relocaliser(object):
    """The kfn_reloc_* launches with their buffers, attached to `tracker` (before its start()): the fern `table` [ferns, 4] int32,
    `code` [ferns] and `codes` [keyframes, ferns] uint8, `key_poses` [keyframes, 12] fp64, `dist` [keyframes] int32, `record`
    (kfn_reloc_state) and `rows` [max_frames, 8] int32 are device tensors.  `level` None is the tracker's coarsest; `min_share`
    and `max_rms` None are the tracker's own gates, so that verification adds no strictness."""

    def __init__(self, tracker, ferns=500, keyframes=1024, harvest_share=0.2, tries=3, seed=1, level=None, depth_range=(0.5, 4.0),
                 min_share=None, max_rms=None):
        torch = tracker.torch
        if tracker.first is not None:
            raise ValueError('the relocaliser must be attached before start(): frame 0 is keyframe 0')
        level = tracker.levels - 1 if level is None else level
        min_share = tracker.desc[0].min_share if min_share is None else min_share
        max_rms = tracker.desc[0].max_rms if max_rms is None else max_rms
        if not 1 <= ferns <= _lib.RELOC_MAX_FERNS:
            raise ValueError('ferns must lie in 1 .. %d, got %r' % (_lib.RELOC_MAX_FERNS, ferns))
        if not 1 <= keyframes <= _lib.RELOC_MAX_CAPACITY:
            raise ValueError('keyframes must lie in 1 .. %d, got %r' % (_lib.RELOC_MAX_CAPACITY, keyframes))
        if not 1 <= tries <= _lib.RELOC_MAX_TRIES:
            raise ValueError('tries must lie in 1 .. %d, got %r' % (_lib.RELOC_MAX_TRIES, tries))
        if not 0 <= level < tracker.levels:
            raise ValueError('level %r outside 0 .. %d' % (level, tracker.levels - 1))
        if not 0.0 <= harvest_share <= 1.0:
            raise ValueError('harvest_share must lie in 0 .. 1, got %r' % (harvest_share,))
        if not 0.0 <= min_share <= 1.0:
            raise ValueError('min_share must lie in 0 .. 1, got %r' % (min_share,))
        if not 0.0 < max_rms < float('inf'):
            raise ValueError('max_rms must be positive and finite, got %r' % (max_rms,))
        self.trk, self.lib, self.torch, self.device = tracker, tracker.lib, torch, tracker.device
        self.ferns, self.capacity, self.tries, self.level = int(ferns), int(keyframes), int(tries), int(level)
        self.harvest = int(math.floor(harvest_share * ferns))
        self.colour = tracker.vol.color_volume is not None
        Hl, Wl, _ = tracker.sizes[self.level]
        self.table_host = fern_table(seed, self.ferns, (Hl, Wl), self.colour, depth_range[0], depth_range[1])
        B, H, W = tracker.vol.shape
        self.desc = _lib.RelocDesc(H=H, W=W, levels=tracker.levels, reloc_level=self.level, ferns=self.ferns, capacity=self.capacity,
                                   tries=self.tries, harvest=self.harvest, rows=tracker.max_frames, traj_rows=tracker.max_frames, slot=0,
                                   first=0, colour=int(self.colour))
        self.desc.reloc_min_share, self.desc.reloc_max_rms = min_share, max_rms
        self.desc_first = _lib.RelocDesc.from_buffer_copy(bytes(self.desc))
        self.desc_first.first = 1
        with torch.cuda.device(self.device):
            self.table = torch.from_numpy(self.table_host).to(self.device)
            self.code = torch.zeros(self.ferns, dtype=torch.uint8, device=self.device)
            self.codes = torch.zeros((self.capacity, self.ferns), dtype=torch.uint8, device=self.device)
            self.key_poses = torch.zeros((self.capacity, 12), dtype=torch.float64, device=self.device)
            self.dist = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
            self.record = torch.zeros(C.sizeof(_lib.RelocState) // 8, dtype=torch.int64, device=self.device)
            self.rows = torch.zeros((tracker.max_frames, _lib.RELOC_ROW_LD), dtype=torch.int32, device=self.device)
        tracker.reloc = self

    def set_state(self, state):
        """Writes a _lib.RelocState into the record."""
        host = self.torch.frombuffer(bytearray(bytes(state)), dtype=self.torch.int64)
        self.record.copy_(host, non_blocking=False)

    def state(self):
        """The record read back (a wait): _lib.RelocState."""
        return _lib.RelocState.from_buffer_copy(self.record.cpu().numpy().tobytes())

    def encode(self):
        vol = self.trk.vol
        _lib.check(self.lib.kfn_reloc_encode(C.byref(self.desc), self.table.data_ptr(), self.trk.live_v.data_ptr(),
                                             vol.frames.data_ptr() if self.colour else None, self.code.data_ptr(),
                                             current_stream(self.device)), 'kfn_reloc_encode')

    def search(self):
        _lib.check(self.lib.kfn_reloc_search(C.byref(self.desc), self.code.data_ptr(), self.codes.data_ptr(), self.record.data_ptr(),
                                             self.dist.data_ptr(), current_stream(self.device)), 'kfn_reloc_search')

    def seed(self):
        _lib.check(self.lib.kfn_reloc_seed(C.byref(self.desc), self.record.data_ptr(), self.trk.record.data_ptr(),
                                           self.key_poses.data_ptr(), current_stream(self.device)), 'kfn_reloc_seed')

    def settle(self, first=False):
        trk = self.trk
        _lib.check(self.lib.kfn_reloc_settle(C.byref(self.desc_first if first else self.desc), self.record.data_ptr(),
                                             trk.record.data_ptr(), self.code.data_ptr(), self.codes.data_ptr(),
                                             self.key_poses.data_ptr(), trk.vol.poses.data_ptr(), trk.trajectory_rows.data_ptr(),
                                             self.rows.data_ptr(), current_stream(self.device)), 'kfn_reloc_settle')


class Tracker(object):
    """The kfn_track_* launches with their buffers around a `fuse.Volume` (its slot 0 carries the frame).  `live_v`, `live_n`,
    `model_v`, `model_n` [sum H_l W_l, 4], `sums` [32] fp64, `record` (kfn_track_state) and `trajectory_rows` [max_frames, 20]
    are device tensors.  `reloc` = True, or a dict of Relocaliser's keywords, attaches a Relocaliser; None leaves every launch
    as it is without one."""

    def __init__(self, volume, levels=3, iterations=(10, 5, 4), far=8.0, min_weight=1.0, pyr_dist=0.1, jump=0.1, dist_max=0.1,
                 angle_max=20.0, min_pairs=50, pivot_floor=1e-10, min_share=0.1, max_rms=0.04, max_step_m=0.3, max_step_rad=0.35,
                 max_frames=4096, reloc=None):
        torch = volume.torch
        B, H, W = volume.shape
        self.iterations = check_levels((H, W), levels, iterations)
        for name, x in (('far', far - volume.near), ('dist_max', dist_max), ('max_rms', max_rms), ('max_step_m', max_step_m),
                        ('max_step_rad', max_step_rad)):
            if not x > 0.0:
                raise ValueError('%s must be positive%s' % (name, ' beyond near' if name == 'far' else ''))
        if not 0.0 < angle_max <= 180.0:
            raise ValueError('angle_max must lie in 0 .. 180 degrees, got %r' % (angle_max,))
        if not min_weight >= 1.0:
            raise ValueError('min_weight must be at least 1, got %r' % (min_weight,))
        if min_pairs < 6 or max_frames < 2:
            raise ValueError('min_pairs must be at least 6 and max_frames at least 2')
        if min(volume.dims) < 2:
            raise ValueError('the volume needs two lattice points an axis or more')
        self.vol, self.levels, self.max_frames = volume, levels, max_frames
        self.lib, self.torch, self.device = volume.lib, torch, volume.device
        self.sizes = level_sizes((H, W), levels)
        kw = dict(levels=levels, near=volume.near, far=far, min_weight=min_weight, pyr_dist=pyr_dist, jump=jump, dist_max=dist_max,
                  angle_max=angle_max, min_pairs=min_pairs, pivot_floor=pivot_floor, min_share=min_share, max_rms=max_rms,
                  max_step_m=max_step_m, max_step_rad=max_step_rad, traj_rows=max_frames, slot=0)
        self.desc = [track_descriptor(volume.camera, volume.dims, volume.origin, volume.voxel, volume.trunc, (H, W), level=l, **kw)
                     for l in range(levels)]
        size = C.c_size_t()
        _lib.check(self.lib.kfn_track_scratch_bytes(C.byref(self.desc[0]), C.byref(size)), 'kfn_track_scratch_bytes')
        total = sum(h * w for h, w, _ in self.sizes)
        with torch.cuda.device(self.device):
            self.live_v, self.live_n, self.model_v, self.model_n = (torch.zeros((total, 4), dtype=torch.float32, device=self.device)
                                                                    for _ in range(4))
            self.scratch = torch.zeros(size.value // 8, dtype=torch.float64, device=self.device)
            self.sums = torch.zeros(_lib.TRACK_SUMS_LD, dtype=torch.float64, device=self.device)
            self.record = torch.zeros(C.sizeof(_lib.TrackState) // 8, dtype=torch.int64, device=self.device)
            self.trajectory_rows = torch.zeros((max_frames, _lib.TRACK_TRAJ_LD), dtype=torch.float64, device=self.device)
        self.first, self.pushed = None, 0
        self.reloc = None
        if reloc is not None and reloc is not False:
            Relocaliser(self, **(dict() if reloc is True else dict(reloc)))

    # -- the record -----------------------------------------------------------------------------------------------------------
    def set_state(self, committed, estimate=None, frame=1):
        st = pose_record(committed, estimate, frame)
        host = self.torch.frombuffer(bytearray(bytes(st)), dtype=self.torch.int64)
        self.record.copy_(host, non_blocking=False)

    def state(self):
        """The record read back (a wait): _lib.TrackState."""
        return _lib.TrackState.from_buffer_copy(self.record.cpu().numpy().tobytes())

    # -- the launches, one by one ---------------------------------------------------------------------------------------------
    def _stage(self, depth_u16, frame_u8):
        torch, vol = self.torch, self.vol
        B, H, W = vol.shape
        if torch.is_tensor(depth_u16):
            if depth_u16.dtype not in (torch.int16, torch.uint16):
                raise ValueError('depth must be uint16 (or its bits as int16), got %s' % depth_u16.dtype)
            dp = depth_u16.contiguous().view(torch.int16)
        else:
            dp = np.ascontiguousarray(depth_u16)
            if dp.dtype != np.uint16:
                raise ValueError('depth must be uint16, got %s' % dp.dtype)
            dp = torch.from_numpy(dp.view(np.int16))
        if tuple(dp.shape) != (H, W):
            raise ValueError('depth must be uint16 [%d,%d], got %s' % (H, W, tuple(dp.shape)))
        if (frame_u8 is None) != (vol.color_volume is None):
            raise ValueError('a frame goes with a colour volume: give both or neither')
        vol.depth[0].copy_(dp, non_blocking=True)
        if frame_u8 is not None:
            fr = frame_u8 if torch.is_tensor(frame_u8) else torch.from_numpy(np.ascontiguousarray(frame_u8))
            if fr.dtype != torch.uint8 or tuple(fr.shape) != (H, W, 3):
                raise ValueError('the frame must be uint8 [%d,%d,3], got %s %s' % (H, W, fr.dtype, tuple(fr.shape)))
            vol.frames[0].copy_(fr, non_blocking=True)

    def live_maps(self):
        _lib.check(self.lib.kfn_track_live_maps(C.byref(self.desc[0]), self.vol.depth.data_ptr(), self.live_v.data_ptr(),
                                                self.live_n.data_ptr(), current_stream(self.device)), 'kfn_track_live_maps')

    def raycast(self, level):
        _lib.check(self.lib.kfn_track_raycast(C.byref(self.desc[level]), self.vol.tsdf_volume.data_ptr(), self.record.data_ptr(),
                                              self.model_v.data_ptr(), self.model_n.data_ptr(), current_stream(self.device)),
                   'kfn_track_raycast')

    def icp_sums(self, level):
        _lib.check(self.lib.kfn_track_icp_sums(C.byref(self.desc[level]), self.live_v.data_ptr(), self.live_n.data_ptr(),
                                               self.model_v.data_ptr(), self.model_n.data_ptr(), self.record.data_ptr(),
                                               self.scratch.data_ptr(), self.sums.data_ptr(), current_stream(self.device)),
                   'kfn_track_icp_sums')

    def update(self, level):
        _lib.check(self.lib.kfn_track_update(C.byref(self.desc[level]), self.sums.data_ptr(), self.record.data_ptr(),
                                             current_stream(self.device)), 'kfn_track_update')

    def commit(self):
        _lib.check(self.lib.kfn_track_commit(C.byref(self.desc[0]), self.record.data_ptr(), self.vol.poses.data_ptr(),
                                             self.trajectory_rows.data_ptr(), current_stream(self.device)), 'kfn_track_commit')

    def integrate(self):
        """kfn_fuse_integrate on slot 0: the depth map staged and the pose row the commit (or start) wrote."""
        vol = self.vol
        d = vol.descriptor(1)
        _lib.check(self.lib.kfn_fuse_integrate(C.byref(d), vol.tsdf_volume.data_ptr(),
                                               None if vol.color_volume is None else vol.color_volume.data_ptr(), vol.depth.data_ptr(),
                                               None if vol.frames is None else vol.frames.data_ptr(), vol.poses.data_ptr(),
                                               current_stream(self.device)), 'kfn_fuse_integrate')

    # -- a sequence -----------------------------------------------------------------------------------------------------------
    def start(self, first_pose, depth_u16, frame_u8=None):
        """Sets the committed pose and integrates frame 0 under it."""
        first = np.asarray(first_pose, dtype=np.float64)
        if first.shape != (4, 4) or not np.isfinite(first).all():
            raise ValueError('the first pose must be a finite [4,4] camera-to-world matrix')
        with self.torch.cuda.device(self.device):
            self.set_state(first)
            self._stage(depth_u16, frame_u8)
            self.vol.poses[:1].copy_(self.torch.from_numpy(pose_rows(first[None])), non_blocking=True)
            if self.reloc is not None:                                   # frame 0 becomes keyframe 0
                self.live_maps()
                self.reloc.encode()
                self.reloc.search()
                self.reloc.settle(first=True)
            self.integrate()
        self.first, self.pushed = first.copy(), 0

    def push(self, depth_u16, frame_u8=None):
        """Queues one frame; reads nothing back."""
        if self.first is None:
            raise ValueError('push() before start(): there is no committed pose')
        if self.pushed + 2 > self.max_frames:
            raise ValueError('the trajectory buffer holds %d frames' % self.max_frames)
        with self.torch.cuda.device(self.device):
            self._stage(depth_u16, frame_u8)
            self.live_maps()
            if self.reloc is not None:
                self.reloc.encode()
                self.reloc.search()
                self.reloc.seed()
            for l in range(self.levels):
                self.raycast(l)
            for l in range(self.levels - 1, -1, -1):
                for _ in range(self.iterations[l]):
                    self.icp_sums(l)
                    self.update(l)
            self.commit()
            if self.reloc is not None:
                self.reloc.settle()
            self.integrate()
        self.pushed += 1

    def trajectory(self):
        """The one read: (poses [N,4,4] fp64, NaN where lost; lost bool [N]; diagnostics [N,8] in the order of DIAGNOSTICS).
        Frame 0 is the pose given to start()."""
        n = self.pushed + 1
        rows = self.trajectory_rows[:n].cpu().numpy()
        poses = np.zeros((n, 4, 4), dtype=np.float64)
        poses[:, 3, 3] = 1.0
        poses[:, :3, :] = rows[:, :12].reshape(n, 3, 4)
        poses[0] = self.first
        diag = rows[:, 12:20].copy()
        diag[0] = 0.0
        return poses, diag[:, 0] != 0, diag

    def relocalisation(self):
        """The relocaliser's one read: (rows int32 [N, 8] in the order of RELOC_ROW, the keyframe count, the keyframes' poses
        [count, 4, 4] fp64)."""
        if self.reloc is None:
            raise ValueError('relocalisation() needs a tracker made with reloc')
        n = self.pushed + 1
        rc = self.reloc
        packed = self.torch.cat([rc.record.view(self.torch.uint8), rc.rows[:n].reshape(-1).view(self.torch.uint8),
                                 rc.key_poses.reshape(-1).view(self.torch.uint8)]).cpu().numpy()
        size, rows_bytes = C.sizeof(_lib.RelocState), n * _lib.RELOC_ROW_LD * 4
        st = _lib.RelocState.from_buffer_copy(packed[:size].tobytes())
        count = min(max(st.n, 0), rc.capacity)
        rows = packed[size:size + rows_bytes].copy().view(np.int32).reshape(n, _lib.RELOC_ROW_LD)
        rows12 = packed[size + rows_bytes:].copy().view(np.float64).reshape(rc.capacity, 12)[:count]
        poses = np.zeros((count, 4, 4), dtype=np.float64)
        poses[:, 3, 3] = 1.0
        poses[:, :3, :] = rows12.reshape(count, 3, 4)
        return rows, count, poses


RELOC_ROW = ('min_d', 'nearest', 'seed_key', 'added', 'streak', 'candidates', 'demoted', 'reserved')


def box_in_front(first_pose, extent):
    """The default box: an axis-aligned cube of `extent` metres whose centre lies extent / 2 in front of the first camera."""
    P = np.asarray(first_pose, dtype=np.float64)
    centre = P[:3, 3] + P[:3, 2] * (0.5 * extent)
    return centre - 0.5 * extent, centre + 0.5 * extent


def write_report(path, names, lost, diag, rows=None):
    """track_report.txt; with the relocaliser's `rows` a tracked frame that was seeded from a keyframe is named `relocalised`."""
    with open(path, 'w') as f:
        f.write('# frame state ' + ' '.join(DIAGNOSTICS[1:]) + '\n')
        for k, name in enumerate(names):
            state = 'lost' if lost[k] else ('relocalised' if rows is not None and rows[k, 2] >= 0 else 'tracked')
            f.write('%s %s %d %.6f %.6e %d %d %.6e %.6e\n' % ((name, state, int(diag[k, 1]), diag[k, 2], diag[k, 3],
                                                               int(diag[k, 4]), int(diag[k, 5]), diag[k, 6], diag[k, 7])))


def write_reloc_report(path, names, rows):
    """reloc_report.txt: per frame the nearest keyframe and its distance in ferns, the keyframe ICP was seeded from, the keyframe
    the frame became, and the lost frames in a row after it (-1: none)."""
    with open(path, 'w') as f:
        f.write('# frame nearest distance seeded_key keyframe_added streak\n')
        for k, name in enumerate(names):
            f.write('%s %d %d %d %d %d\n' % (name, rows[k, 1], rows[k, 0], rows[k, 2], rows[k, 3], rows[k, 4]))


def write_outputs(folder, pairs, poses, lost, diag, reloc_rows=None):
    """The pose files of the tracked frames, the three lists naming them, and track_report.txt; with `reloc_rows` (the rows of
    Tracker.relocalisation()) also reloc_report.txt."""
    from .KFNet.pnp import write_pose
    os.makedirs(folder, exist_ok=True)
    cols = ([], [], [])
    for k, (colour, depth) in enumerate(pairs):
        if lost[k]:
            continue
        stem = os.path.basename(depth)
        stem = stem[:-len('.depth.png')] if stem.endswith('.depth.png') else 'frame-%06d' % k
        p = os.path.abspath(os.path.join(folder, stem + '.pose.txt'))
        write_pose(p, poses[k])
        for col, x in zip(cols, (os.path.abspath(colour), os.path.abspath(depth), p)):
            col.append(x)
    for name, col in zip(('image_list.txt', 'depth_list.txt', 'pose_list.txt'), cols):
        with open(os.path.join(folder, name), 'w') as f:
            f.write(''.join(x + '\n' for x in col))
    names = [os.path.basename(p[1]) for p in pairs]
    write_report(os.path.join(folder, 'track_report.txt'), names, lost, diag, reloc_rows)
    if reloc_rows is not None:
        write_reloc_report(os.path.join(folder, 'reloc_report.txt'), names, reloc_rows)


# ---- the program --------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(prog='python -m kfnet_amd.track', description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='command')
    mk = sub.add_parser('make', help='poses (and the mesh) of an RGB-D sequence without pose files')
    mk.add_argument('--sequence', default='', help='a folder of frame-*.color.png and frame-*.depth.png')
    mk.add_argument('--output_folder', default='')
    mk.add_argument('--first_pose', default='', help='a 4x4 camera-to-world pose file for frame 0 (the identity)')
    mk.add_argument('--mesh', default='', help='also write the volume\'s mesh to this PLY file')
    mk.add_argument('--voxel', type=float, default=0.02, help='metres between lattice points')
    mk.add_argument('--trunc', type=float, default=None, help='truncation distance in metres (4 voxels)')
    mk.add_argument('--bounds', type=float, nargs=6, default=None, metavar=('X0', 'Y0', 'Z0', 'X1', 'Y1', 'Z1'))
    mk.add_argument('--extent', type=float, default=None, help='without --bounds: a cube of this many metres in front of frame 0 (4.0)')
    mk.add_argument('--min_weight', type=float, default=2.0, help='for --mesh: a lattice point counts once this many frames saw it')
    mk.add_argument('--no_color', action='store_true', help='fuse depth only: the mesh is white')
    add_camera_flags(mk)
    mk.add_argument('--height', type=int, default=480)
    mk.add_argument('--width', type=int, default=640)
    mk.add_argument('--gpu', type=int, default=0)
    mk.add_argument('--dist_max', type=float, default=0.1, help='metres between a pair\'s points at most')
    mk.add_argument('--angle_max', type=float, default=20.0, help='degrees between a pair\'s normals at most')
    mk.add_argument('--levels', type=int, default=3)
    mk.add_argument('--iterations', type=int, nargs='+', default=None, help='per level, finest first (10 5 4)')
    mk.add_argument('--reloc', action='store_true', help='relocalise after a loss from fern-coded keyframes; writes reloc_report.txt')
    mk.add_argument('--reloc_ferns', type=int, default=500, help='binary tests a frame\'s code holds (1 .. 4096)')
    mk.add_argument('--reloc_keyframes', type=int, default=1024, help='keyframes kept at most (1 .. 65536)')
    mk.add_argument('--reloc_harvest', type=float, default=0.2, help='a tracked frame becomes a keyframe when more than this share of '
                    'its ferns differs from every keyframe\'s')
    mk.add_argument('--reloc_tries', type=int, default=3, help='nearest keyframes tried in turn after a loss (1 .. 4)')
    mk.add_argument('--reloc_seed', type=int, default=1, help='seed of the fern table')
    mk.add_argument('--reloc_min_share', type=float, default=None, help='share of pixels a relocalised frame must pair (the tracker\'s 0.1)')
    mk.add_argument('--reloc_max_rms', type=float, default=None, help='residual in metres a relocalised frame may leave (the tracker\'s 0.04)')
    return ap


def make(a):
    from .fuse import Volume, box_lattice, check_volume
    from .modes import load_images

    def refuse(text):
        print(text, file=sys.stderr)
        return 1
    if not a.sequence:
        return refuse('track make: --sequence is required')
    if not a.output_folder:
        return refuse('track make: --output_folder is required')
    if a.bounds is not None and a.extent is not None:
        return refuse('track make: --bounds and --extent exclude each other')
    extent = 4.0 if a.extent is None else a.extent
    trunc = 4.0 * a.voxel if a.trunc is None else a.trunc
    for name, x in (('--voxel', a.voxel), ('--trunc', trunc), ('--extent', extent), ('--dist_max', a.dist_max), ('--angle_max', a.angle_max)):
        if not x > 0.0:
            return refuse('%s must be positive' % name)
    if not a.min_weight >= 1.0:
        return refuse('--min_weight must be at least 1')
    iterations = (10, 5, 4) if a.iterations is None and a.levels == 3 else a.iterations
    if iterations is None:
        return refuse('--levels %d needs --iterations: one count a level, finest first' % a.levels)
    try:
        check_size(a.height, a.width, '--height and --width')
        iterations = check_levels((a.height, a.width), a.levels, iterations)
        camera = camera_of(a)
        pairs = read_frames(a.sequence)
        first = np.eye(4)
        if a.first_pose:
            from .KFNet.pnp import read_pose
            first = read_pose(a.first_pose)
            if not np.isfinite(first).all():
                raise ValueError('%s: the pose is not finite' % a.first_pose)
        lo, hi = (a.bounds[:3], a.bounds[3:]) if a.bounds is not None else box_in_front(first, extent)
        dims, origin = box_lattice(lo, hi, a.voxel)
        check_volume(dims, a.voxel, trunc)
    except (ValueError, OSError) as e:
        return refuse(str(e))
    size = (a.height, a.width)
    import torch
    if not torch.cuda.is_available():
        return refuse('track make needs a GPU: the camera is tracked on the device')
    device = 'cuda:%d' % a.gpu
    try:
        vol = Volume(dims, origin, a.voxel, trunc, camera, size, 1, not a.no_color, device=device)
        reloc = None
        if a.reloc:
            reloc = dict(ferns=a.reloc_ferns, keyframes=a.reloc_keyframes, harvest_share=a.reloc_harvest, tries=a.reloc_tries,
                         seed=a.reloc_seed, min_share=a.reloc_min_share, max_rms=a.reloc_max_rms)
        trk = Tracker(vol, a.levels, iterations, dist_max=a.dist_max, angle_max=a.angle_max, max_frames=max(len(pairs), 2), reloc=reloc)
        for k, (colour, depth) in enumerate(pairs):
            dp = load_depth([depth], size)[0]
            fr = None if a.no_color else load_images([colour], size)[0]
            if k == 0:
                trk.start(first, dp, fr)
            else:
                trk.push(dp, fr)
        poses, lost, diag = trk.trajectory()
        rows, keyframes, _ = trk.relocalisation() if a.reloc else (None, 0, None)
        write_outputs(a.output_folder, pairs, poses, lost, diag, rows)
        if a.mesh:
            from .render import write_ply
            vertices, colors, triangles = vol.mesh(a.min_weight)
            if not len(triangles):
                return refuse('the volume holds no surface: no mesh to write')
            write_ply(a.mesh, vertices, triangles, colors)
    except ValueError as e:
        return refuse(str(e))
    extra = ''
    if a.reloc:
        extra = '; %d keyframes, %d relocalised' % (keyframes, int(((rows[:, 2] >= 0) & ~lost).sum()))
    print('%d frames, %d tracked, %d lost; %d x %d x %d voxels of %g m from (%g, %g, %g)%s' %
          ((len(pairs), int((~lost).sum()), int(lost.sum())) + tuple(dims) + (a.voxel,) + tuple(origin) + (extra,)))
    return 0


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.command != 'make':
        ap.print_usage(sys.stderr)
        return 1
    return make(a)


if __name__ == '__main__':
    sys.exit(main())
