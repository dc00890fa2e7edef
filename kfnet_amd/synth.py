"""Synthetic inputs for benchmarks / parity tests.

No 7-Scenes data or trained weights are reachable from this environment, so sequences
are a fixed random texture rolled by (t*dx, t*dy) pixels plus +-4 noise -- the rolled
texture gives OFlowNet's cost volume a non-trivial optimum so the soft-argmax flow is
not uniform.
"""
import numpy as np


def synthetic_sequence(T, H=480, W=640, seed=1, dx=3, dy=2, noise=4, start=0):
    """Frames [start, start+T) of the seeded sequence (frame t depends only on (seed, t),
    so ranks can generate their own chunk)."""
    rng = np.random.default_rng(seed)
    # low-frequency texture: upsampled coarse noise + fine noise, 0..255
    coarse = rng.integers(0, 256, size=(H // 8 + 2, W // 8 + 2, 3)).astype(np.float32)
    tex = np.kron(coarse, np.ones((8, 8, 1), dtype=np.float32))[:H, :W]
    tex = 0.75 * tex + 0.25 * rng.integers(0, 256, size=(H, W, 3)).astype(np.float32)
    frames = np.empty((T, H, W, 3), dtype=np.uint8)
    for k in range(T):
        t = start + k
        f = np.roll(tex, shift=(t * dy, t * dx), axis=(0, 1))
        f = f + np.random.default_rng([seed, t]).integers(-noise, noise + 1, size=f.shape)
        frames[k] = np.clip(f, 0, 255).astype(np.uint8)
    return frames


def synthetic_transform(seed=7):
    """Fixed seeded rigid 4x4 (what transform.txt would hold, KFNet/train.py:49-58)."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(3, 3))
    Q, _ = np.linalg.qr(A)
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    M = np.eye(4, dtype=np.float32)
    M[:3, :3] = Q.astype(np.float32)
    M[:3, 3] = rng.uniform(-1, 1, size=3).astype(np.float32)
    return M


def synthetic_poses(count, seed=11, start=0):
    """Seeded rigid camera-to-world poses [count,4,4] of frames [start, start + count): a small rotation about a fixed axis
    and a drift that grow with the frame index.  They belong to no scene: a reprojection loss on them is finite, not small."""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    drift = rng.uniform(-0.05, 0.05, size=3)
    out = np.zeros((count, 4, 4), dtype=np.float64)
    for i in range(count):
        a = 0.02 * (start + i)
        out[i, :3, :3] = np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)      # Rodrigues
        out[i, :3, 3] = np.array([0.3, -0.2, -1.0]) + drift * (start + i)
        out[i, 3, 3] = 1.0
    return out


ROOM = (4.0, 3.0, 2.5)      # synthetic_scene's room: x, y on the floor, z up, one corner at the origin


def synthetic_scene_boxes(seed):
    """The axis-aligned boxes [(lo xyz, hi xyz)] of synthetic_scene(seed): the room first, then the boxes standing in it."""
    rng = np.random.default_rng([seed, 0x5ce4e])
    boxes = [(np.zeros(3), np.array(ROOM))]
    for cx, cy in ((3.0, 0.6), (3.1, 1.5), (2.9, 2.4)):
        half = rng.uniform(0.2, 0.3, size=2)
        centre = np.array([cx, cy])                       # fixed places: the gaps between them stay above 0.3 m
        height = rng.uniform(0.5, 1.2)
        boxes.append((np.array([centre[0] - half[0], centre[1] - half[1], 0.0]),
                      np.array([centre[0] + half[0], centre[1] + half[1], height])))
    return boxes


def _box_surface(lo, hi, n):
    """A closed box surface, every face n x n quads of two triangles, the vertices on its edges shared by the faces."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing='ij')
    i, j = i.ravel(), j.ravel()
    lattice, quads = [], []
    for axis in range(3):
        for side in (0, n):
            ijk = [None, None, None]
            ijk[axis] = np.full_like(i, side)
            ijk[(axis + 1) % 3], ijk[(axis + 2) % 3] = i, j
            base = len(lattice) * (n + 1) * (n + 1)
            lattice.append(np.stack(ijk, axis=1))
            a, b = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
            p = base + (a * (n + 1) + b).ravel()
            q = np.stack([p, p + (n + 1), p + (n + 2), p + 1], axis=1)        # (a, b), (a+1, b), (a+1, b+1), (a, b+1)
            quads.append(q if side else q[:, ::-1])
    lattice, quads = np.concatenate(lattice), np.concatenate(quads)
    keys = (lattice[:, 0] * (n + 1) + lattice[:, 1]) * (n + 1) + lattice[:, 2]
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    quads = inverse[quads]
    tris = np.concatenate([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]])
    verts = lo + (hi - lo) * lattice[first] / float(n)
    return verts, tris


def synthetic_scene(seed, cells=32):
    """A closed box room of about 4 x 3 x 2.5 m with three boxes standing in it, every face tessellated into cells x cells
    quads: (vertices float32 [V,3], colors uint8 [V,3], triangles int32 [N,3]), N = 48 cells^2.  The colours are an integer
    hash of the vertex index and the seed, so rendered frames have texture."""
    verts, tris, base = [], [], 0
    for lo, hi in synthetic_scene_boxes(seed):
        v, t = _box_surface(lo, hi, int(cells))
        verts.append(v)
        tris.append(t + base)
        base += len(v)
    verts, tris = np.concatenate(verts), np.concatenate(tris)
    h = (np.arange(len(verts), dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed % (1 << 31)) * np.uint64(40503)) \
        & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    colors = np.stack([(h >> np.uint64(s)) & np.uint64(255) for s in (0, 8, 16)], axis=1).astype(np.uint8)
    return verts.astype(np.float32), colors, tris.astype(np.int32)


def synthetic_trajectory(count, seed):
    """Smooth camera-to-world poses [count,4,4] (x right, y down, z forward) inside synthetic_scene's room: the camera moves
    through the empty half of the room, at least 0.3 m from every surface, and looks at the boxes."""
    rng = np.random.default_rng([seed, 0x7a9ec])
    phase = rng.uniform(0.0, 2.0 * np.pi, size=6)
    out = np.zeros((count, 4, 4), dtype=np.float64)
    for i in range(count):
        a = 0.12 * i
        pos = np.array([1.05 + 0.5 * np.sin(a + phase[0]), 1.5 + 0.85 * np.sin(0.7 * a + phase[1]),
                        1.3 + 0.3 * np.sin(0.5 * a + phase[2])])
        target = np.array([3.0 + 0.2 * np.sin(0.3 * a + phase[3]), 1.5 + 0.5 * np.sin(0.4 * a + phase[4]),
                           0.6 + 0.2 * np.sin(0.6 * a + phase[5])])
        fwd = (target - pos) / np.linalg.norm(target - pos)
        right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        out[i, :3, 0], out[i, :3, 1], out[i, :3, 2], out[i, :3, 3] = right, down, fwd, pos
        out[i, 3, 3] = 1.0
    return out
