"""Restatement of the kfn_reloc_* launches (include/kfnet_hip.h) in numpy, written from the header's text: the
fern code of a frame, the search for the nearest keyframes, and the seed / settle state machine, with a Tracker that puts them
around the steps of tests/track_ref.py.  The records are dicts.  Nothing of the product path is imported.
"""
import numpy as np

import fuse_ref as F
import track_ref as T

f32 = np.float32
ROW_LD = 8
ROW = ('min_d', 'nearest', 'seed_key', 'added', 'streak', 'candidates', 'demoted', 'zero')


class Params(object):
    """The constants of kfn_reloc_desc; the two gates rounded to fp32 as the descriptor holds them."""

    def __init__(self, ferns=500, capacity=1024, tries=3, harvest=None, harvest_share=0.2, level=2, rows=64, traj_rows=64,
                 min_share=0.1, max_rms=0.04):
        self.ferns, self.capacity, self.tries, self.level, self.rows, self.traj_rows = ferns, capacity, tries, level, rows, traj_rows
        self.harvest = int(np.floor(harvest_share * ferns)) if harvest is None else int(harvest)
        self.min_share, self.max_rms = float(f32(min_share)), float(f32(max_rms))


def level_sizes(image_size, levels):
    H, W = image_size
    out, off = [], 0
    for _ in range(levels):
        out.append((H, W, off))
        off += H * W
        H, W = H // 2, W // 2
    return out


def encode(table, live_v, frame, image_size, level):
    """table int32 [ferns,4], live_v float32 [sum H_l W_l, 4], frame uint8 [H,W,3] or None -> code uint8 [ferns]."""
    table = np.asarray(table, dtype=np.int32)
    Hl, Wl, off = level_sizes(image_size, level + 1)[level]
    side = 1 << level
    code = np.zeros(len(table), dtype=np.uint8)
    for f, (x, y, bits, packed) in enumerate(table.tolist()):
        if not (0 <= x <= Wl - 1 and 0 <= y <= Hl - 1):
            continue
        v = live_v[off + y * Wl + x]
        thr = np.array([bits], dtype=np.int32).view(f32)[0]
        byte = 1 if (v[3] != 0 and v[2] > thr) else 0
        if frame is not None:
            block = np.asarray(frame)[y * side:(y + 1) * side, x * side:(x + 1) * side].astype(np.int64)
            assert block.shape == (side, side, 3)
            for c in range(3):
                if int(block[..., c].sum()) > ((packed >> (8 * c)) & 255) * side * side:
                    byte |= 2 << c
        code[f] = byte
    return code


def new_state():
    return dict(anchor=np.zeros(12), n=0, streak=0, seeded=0, seed_key=0, candidates=0, min_d=0, recovered=0, reserved=0,
                cand_d=[0, 0, 0, 0], cand_index=[0, 0, 0, 0])


def _clamp(v, lo, hi):
    return min(max(int(v), lo), hi)


def search(rs, code, codes, P):
    """kfn_reloc_search on the record `rs` (changed in place)."""
    n = _clamp(rs['n'], 0, P.capacity)
    pairs = sorted((int((np.asarray(codes[i]) != np.asarray(code)).sum()), i) for i in range(n))
    for r in range(4):
        rs['cand_d'][r], rs['cand_index'][r] = pairs[r] if r < min(P.tries, n) else (P.ferns + 1, -1)
    rs['candidates'] = min(P.tries, n)
    rs['min_d'] = rs['cand_d'][0]


def seed(rs, ts, key_poses, P):
    """kfn_reloc_seed: may set the tracker's two poses to a keyframe's."""
    n = _clamp(rs['n'], 0, P.capacity)
    c = _clamp(rs['candidates'], 0, min(P.tries, n))
    if rs['streak'] <= 0 or c <= 0:
        return
    i = rs['cand_index'][(rs['streak'] - 1) % c]
    if not 0 <= i < n:
        return
    ts['committed'], ts['estimate'] = key_poses[i].copy(), key_poses[i].copy()
    rs['seeded'], rs['seed_key'] = 1, i


def settle(rs, ts, code, codes, key_poses, pose_row, trajectory, rows, P, first=False):
    """kfn_reloc_settle: rs, ts, codes [capacity,ferns], key_poses [capacity,12], pose_row float32 [12], trajectory [traj_rows,20]
    and rows int32 [rows,8] are changed in place."""
    n = _clamp(rs['n'], 0, P.capacity)
    c = _clamp(rs['candidates'], 0, min(P.tries, n))
    streak = max(int(rs['streak']), 0)
    row = ts['frame'] - 1
    seeded = (not first) and rs['seeded'] == 1
    tracked = True if first else (0 <= row < P.traj_rows and trajectory[row, 12] == 0.0)
    min_d, nearest = rs['min_d'], (rs['cand_index'][0] if c > 0 else -1)
    added, demoted = -1, 0
    if tracked and seeded and not (ts['last_share'] >= P.min_share and ts['last_rms'] <= P.max_rms):
        demoted, tracked = 1, False
    if tracked:
        streak = 0
        if seeded:
            rs['recovered'] += 1
        elif (n == 0 or min_d > P.harvest) and n < P.capacity:
            codes[n], key_poses[n] = code, ts['committed']
            added, n = n, n + 1
    else:
        if demoted:
            pose_row[:] = np.nan
            if 0 <= row < P.traj_rows:
                trajectory[row, :12], trajectory[row, 12] = np.nan, 1.0
            ts['lost'] += 1
        if streak == 0 and not seeded:
            rs['anchor'] = ts['committed'].copy()
        streak += 1
        if seeded:
            ts['committed'], ts['estimate'] = rs['anchor'].copy(), rs['anchor'].copy()
    rs['n'], rs['streak'], rs['seeded'] = n, streak, 0
    if 0 <= row < P.rows:
        rows[row] = (min_d, nearest, rs['seed_key'] if seeded else -1, added, streak, c, demoted, 0)


class Tracker(object):
    """track_ref.Tracker's steps with the four launches around them: start(pose, depth), push(depth), trajectory(),
    relocalisation().  `reloc` = None leaves the plain tracker."""

    def __init__(self, S, Tp, P=None, table=None, exact_sums=False):
        self.S, self.T, self.P, self.table, self.exact = S, Tp, P, table, exact_sums
        self.tsdf = S.empty(False)[0]
        self.state, self.first, self.pushed = None, None, 0
        rows = 64 if P is None else P.traj_rows
        self.trajectory_rows = np.zeros((rows, T.TRAJ_LD))
        if P is not None:
            self.rs = new_state()
            self.codes = np.zeros((P.capacity, P.ferns), dtype=np.uint8)
            self.key_poses = np.zeros((P.capacity, 12))
            self.rows = np.zeros((P.rows, ROW_LD), dtype=np.int32)
            self.code = np.zeros(P.ferns, dtype=np.uint8)

    def _encode_search(self, live_v):
        self.code = encode(self.table, live_v, None, self.S.image_size, self.P.level)
        search(self.rs, self.code, self.codes, self.P)

    def start(self, pose, depth):
        self.first = np.asarray(pose, dtype=np.float64).reshape(4, 4).copy()
        self.state = T.new_state(self.first)
        if self.P is not None:
            self._encode_search(T.live_maps(depth, self.S, self.T)[0])
            settle(self.rs, self.state, self.code, self.codes, self.key_poses, np.zeros(12, dtype=f32), self.trajectory_rows, self.rows,
                   self.P, first=True)
        self.tsdf, _ = F.integrate(self.tsdf, None, np.asarray(depth)[None], None, self.first[None], self.S)

    def push(self, depth):
        S, Tp, st = self.S, self.T, self.state
        lv = T.levels_of(S, Tp.levels)
        live_v, live_n = T.live_maps(depth, S, Tp)
        if self.P is not None:
            self._encode_search(live_v)
            seed(self.rs, st, self.key_poses, self.P)
        mv, mn = np.zeros_like(live_v), np.zeros_like(live_n)
        for l, (H, W, off, _, _, _, _) in enumerate(lv):
            mv[off:off + H * W], mn[off:off + H * W] = T.raycast(self.tsdf, st['committed'], S, Tp, l)
        for l in range(Tp.levels - 1, -1, -1):
            for _ in range(Tp.iterations[l]):
                J, r = T.icp_rows(live_v, live_n, mv, mn, st['estimate'], st['committed'], S, Tp, l)
                T.update(T.icp_sums(J, r, self.exact)[0], st, lv[l][0] * lv[l][1], Tp)
        frame = st['frame']
        pose_row, row = T.commit(st, Tp)
        self.trajectory_rows[frame] = row
        if self.P is not None:
            settle(self.rs, st, self.code, self.codes, self.key_poses, pose_row, self.trajectory_rows, self.rows, self.P)
        self.tsdf, _ = F.integrate(self.tsdf, None, np.asarray(depth)[None], None, pose_row[None], S)
        self.pushed += 1
        return self.trajectory_rows[frame]

    def trajectory(self):
        """-> (poses [N,4,4] fp64 with frame 0 first, lost bool [N], diagnostics [N,8]) as track_ref.Tracker.trajectory."""
        n = self.pushed + 1
        rows = self.trajectory_rows[:n]
        poses = np.stack([self.first] + [T.pose_of(r[:12]) for r in rows[1:]])
        diag = rows[:, 12:20].copy()
        diag[0] = 0.0
        return poses, diag[:, 0] != 0, diag

    def relocalisation(self):
        """-> (rows int32 [N,8], keyframes, key_poses [keyframes,12])."""
        return self.rows[:self.pushed + 1].copy(), self.rs['n'], self.key_poses[:self.rs['n']].copy()


# ---- the shared scenario of the CPU and the GPU tests ------------------------------------------------------------------------------
# Phase A walks track_ref.sequence_trajectory; phase B is N_B all-zero depth maps; phase C reappears half a step behind frame
# REAPPEAR + 1 of phase A and walks on.  N_B and N_C are the least the scenario allows; N_A is the smallest for which
# tests/test_reloc_host.py's conditions hold: the camera moves 0.023 m a frame and the plain tracker's ICP converges from as
# far as its max_step_m = 0.3 m lets it commit, so the last frame of phase C (3.5 steps along) must lie more than 0.3 m from
# frame N_A - 1: N_A = 17 leaves 0.29 m there and the plain tracker recovers, N_A = 18 leaves 0.314 m.
# The depth-only code of this 64 x 96 scene changes by one or two ferns of 500 a frame (46 over 40 frames), so the default
# harvest_share of 0.2 would harvest nothing but frame 0 in any affordable phase A; the scenario harvests at 0.0225 (11
# ferns), which gives keyframes at frames 0, 8 and 12 and on no frame a distance equal to the threshold (10 ferns would meet
# frame 7's distance of exactly 10, which condition (d) excludes).
N_A, N_B, N_C, REAPPEAR = 18, 2, 4, 0
SCENARIO_FERNS, SCENARIO_HARVEST_SHARE, SCENARIO_TRIES, SCENARIO_SEED, SCENARIO_KEYFRAMES = 500, 0.0225, 3, 1, 64


def scenario_poses(n_a=None, n_c=None, reappear=None):
    """-> (poses [N_A + N_B + N_C, 4, 4], phase [N] of 'A' / 'B' / 'C'); phase B's poses are NaN."""
    n_a, n_c, reappear = N_A if n_a is None else n_a, N_C if n_c is None else n_c, REAPPEAR if reappear is None else reappear
    half = T.sequence_trajectory(2 * max(n_a, reappear + n_c + 1), step=0.5 * T.SEQ_PHASE_STEP)
    a, c = half[0:2 * n_a:2], half[2 * reappear + 1::2][:n_c]
    assert len(a) == n_a and len(c) == n_c
    return np.concatenate([a, np.full((N_B, 4, 4), np.nan), c]), 'A' * n_a + 'B' * N_B + 'C' * n_c


def scenario_params(rows=32):
    return Params(ferns=SCENARIO_FERNS, capacity=SCENARIO_KEYFRAMES, tries=SCENARIO_TRIES, harvest_share=SCENARIO_HARVEST_SHARE, level=2,
                  rows=rows, traj_rows=rows)


def scenario_depth(render, poses, phase):
    """The depth maps uint16 [N,H,W]: `render(poses [n,4,4]) -> depth [n,H,W]` for phases A and C, zeros for phase B."""
    seen = np.array([p != 'B' for p in phase])
    depth = np.zeros((len(phase), T.SEQ_H, T.SEQ_W), dtype=np.uint16)
    depth[seen] = render(poses[seen])
    return depth


def run_scenario(depth, first_pose, P=None, table=None):
    """The restated tracker (plain without P) through every frame -> the Tracker."""
    trk = Tracker(T.sequence_setup(), T.Params(), P, table)
    trk.start(first_pose, depth[0])
    for k in range(1, len(depth)):
        trk.push(depth[k])
    return trk
