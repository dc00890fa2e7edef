"""Restatements of kfn_fuse_integrate and kfn_fuse_extract (include/kfnet_hip.h) in numpy, vectorised.

integrate(..., dtype=np.float32) and extract(..., dtype=np.float32) follow the header's fp32 operations one by one, in
their order, so they reproduce the device's bits.  With dtype=np.float64 they are the same definitions in fp64;
integrate(..., audit=True) then also marks every voxel-frame pair one of whose decisions (steps 3-6: Z against near, the
pixel chosen and with it the raw value, s against -trunc) lies within the margins below of its threshold, and returns the
bound of |D32 - D64| elsewhere.

The constants are the fp32-rounded ones in both runs (kfnet_amd.fuse.fuse_descriptor), so the two differ by the arithmetic
alone.

Margins (derived in DESIGN.md 6k from the stated operation sequence, eps = 2^-24), with L = |p|_1 + |t|_1, which bounds
every intermediate of steps 2 (the rows and columns of R have unit length):
    a camera coordinate is off by at most     mC = COORD_ULPS eps L        (p: 2 roundings, d: 1, three products, two sums)
    a projected coordinate by at most         mS = (f / Z) (1 + |q|) mC + PROJ_ULPS eps (|s| + |u|)
    s = dm - Z by at most                     mD = mC + DIST_ULPS eps (dm + |Z|)
    D, where every decision agreed, by        max over the frames of (mD / trunc + 2 eps) + 3 eps per frame applied:
                                              the update is a convex combination, so errors of f do not grow
"""
import numpy as np

EPS32 = 2.0 ** -24
COORD_ULPS = 10.0
PROJ_ULPS = 4.0
DIST_ULPS = 2.0

EDGE_CODE = (1, 2, 4, 3, 5, 6, 7)                  # the far ends of the seven owned edges, bit 0: +x, 1: +y, 2: +z
EDGE_INDEX = {1: 0, 2: 1, 4: 2, 3: 3, 5: 4, 6: 5, 7: 6}
PERMUTATIONS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))       # xyz xzy yxz yzx zxy zyx
TET = tuple((0, 1 << a, (1 << a) | (1 << b), 7) for a, b, c in PERMUTATIONS)
TET_ODD = tuple(int(np.linalg.det(np.eye(3)[list(p)]) < 0) for p in PERMUTATIONS)
POP = np.array([bin(k).count('1') for k in range(256)], dtype=np.int64)


def derive_table():
    """{inside mask: [triangle: three edges (p, q), p < q]} of a positively oriented tetrahedron, from the one rule: the
    vertices lie on the edges between an inside and an outside corner, and (v1 - v0) x (v2 - v0) points from inside to
    outside.  Decided with determinants on the tetrahedron (0,0,0) (1,0,0) (1,1,0) (1,1,1) cut at the edges' midpoints."""
    c = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]], dtype=np.float64)
    assert np.linalg.det(c[1:] - c[0]) > 0
    mid = lambda e: 0.5 * (c[e[0]] + c[e[1]])
    edge = lambda a, b: (min(a, b), max(a, b))
    table = dict()
    for m in range(16):
        ins = [j for j in range(4) if (m >> j) & 1]
        outs = [j for j in range(4) if not (m >> j) & 1]
        tris = []
        if len(ins) in (1, 3):
            i = (ins if len(ins) == 1 else outs)[0]
            j, k, l = outs if len(ins) == 1 else ins
            away = np.linalg.det(np.stack([c[j] - c[i], c[k] - c[i], c[l] - c[i]])) > 0      # the normal of (j k l) leaves i
            keep = away == (len(ins) == 1)
            tris = [[edge(i, j), edge(i, k), edge(i, l)] if keep else [edge(i, j), edge(i, l), edge(i, k)]]
        elif len(ins) == 2:
            (i, j), (k, l) = ins, outs
            quad = [edge(i, k), edge(i, l), edge(j, l), edge(j, k)]
            out_dir = c[outs].mean(axis=0) - c[ins].mean(axis=0)
            if np.dot(np.cross(mid(quad[1]) - mid(quad[0]), mid(quad[2]) - mid(quad[0])), out_dir) < 0:
                quad = [quad[0], quad[3], quad[2], quad[1]]
            tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
        for t in tris:
            n = np.cross(mid(t[1]) - mid(t[0]), mid(t[2]) - mid(t[0]))
            assert np.dot(n, c[outs].mean(axis=0) - c[ins].mean(axis=0)) > 0
        table[m] = tris
    return table


TABLE = derive_table()
TRI_COUNT = np.array([len(TABLE[m]) for m in range(16)], dtype=np.int64)


class Setup(object):
    """The constants of kfn_fuse_desc as floats that fp32 holds exactly.  The depth camera defaults to the colour camera."""

    def __init__(self, dims, origin, voxel, trunc=None, near=0.05, max_weight=64.0, fx=525., fy=525., u=320., v=240.,
                 dfx=None, dfy=None, du=None, dv=None, scale=0.001, raw_min=1, raw_max=65534, image_size=(480, 640)):
        r = lambda x: float(np.float32(x))
        self.dims = tuple(int(x) for x in dims)                   # nx, ny, nz
        self.origin = tuple(r(x) for x in origin)
        self.voxel = r(voxel)
        self.trunc = r(4.0 * voxel if trunc is None else trunc)
        self.near, self.max_weight, self.scale = r(near), r(max_weight), r(scale)
        self.fx, self.fy, self.u, self.v = r(fx), r(fy), r(u), r(v)
        self.dfx, self.dfy = r(fx if dfx is None else dfx), r(fy if dfy is None else dfy)
        self.du, self.dv = r(u if du is None else du), r(v if dv is None else dv)
        self.registered = all(x is None for x in (dfx, dfy, du, dv))
        self.raw_min, self.raw_max = int(raw_min), int(raw_max)
        self.image_size = tuple(image_size)

    def empty(self, color=True, dtype=np.float32):
        nx, ny, nz = self.dims
        return np.zeros((nz, ny, nx, 2), dtype=dtype), (np.zeros((nz, ny, nx, 4), dtype=dtype) if color else None)


def pose_rows32(poses):
    p = np.asarray(poses, dtype=np.float64)
    if p.ndim == 3:
        p = p[:, :3, :].reshape(p.shape[0], 12)
    return np.ascontiguousarray(p, dtype=np.float32)


def _lattice(S, f):
    nx, ny, nz = S.dims
    px = f(S.origin[0]) + np.arange(nx).astype(f) * f(S.voxel)
    py = f(S.origin[1]) + np.arange(ny).astype(f) * f(S.voxel)
    pz = f(S.origin[2]) + np.arange(nz).astype(f) * f(S.voxel)
    return px[None, None, :], py[None, :, None], pz[:, None, None]


def integrate(tsdf, color, depth, frames, poses, S, dtype=np.float32, audit=False):
    """One kfn_fuse_integrate call on copies: -> (tsdf [nz,ny,nx,2], color [nz,ny,nx,4] or None), and with audit (fp64)
    also dict(unclear [B,nz,ny,nx] bool, bound [nz,ny,nx] of |D32 - D64| where nothing is unclear)."""
    f = dtype
    assert (frames is None) == (color is None)
    H, W = S.image_size
    depth = np.asarray(depth)
    assert depth.dtype == np.uint16 and depth.shape[1:] == (H, W)
    P_all = pose_rows32(poses).astype(f)
    B = P_all.shape[0]
    tsdf = np.array(tsdf, dtype=f)
    D, Wt = tsdf[..., 0].copy(), tsdf[..., 1].copy()
    col = None if color is None else np.array(color, dtype=f)
    px, py, pz = _lattice(S, f)
    near, trunc, scale, maxw = f(S.near), f(S.trunc), f(S.scale), f(S.max_weight)
    one = f(1.0)
    if audit:
        unclear = np.zeros((B,) + D.shape, dtype=bool)
        bound = np.zeros(D.shape)
        p1 = np.abs(px) + np.abs(py) + np.abs(pz)
    old = np.seterr(all='ignore')
    try:
        for b in range(B):
            P = P_all[b]
            if not np.isfinite(P).all():
                continue
            dx, dy, dz = px - P[3], py - P[7], pz - P[11]
            X = (P[0] * dx + P[4] * dy) + P[8] * dz
            Y = (P[1] * dx + P[5] * dy) + P[9] * dz
            Z = (P[2] * dx + P[6] * dy) + P[10] * dz
            ok = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & ~(Z < near)
            qx, qy = X / Z, Y / Z
            sx, sy = qx * f(S.dfx) + f(S.du), qy * f(S.dfy) + f(S.dv)
            cf, rf = np.rint(sx), np.rint(sy)
            ok3 = ok
            ok = ok & (cf >= 0) & (cf <= f(W - 1)) & (rf >= 0) & (rf <= f(H - 1))
            c = np.where(ok, cf, 0).astype(np.int64)
            r = np.where(ok, rf, 0).astype(np.int64)
            raw = depth[b][r, c].astype(np.int64)
            ok = ok & (raw >= S.raw_min) & (raw <= S.raw_max)
            ok5 = ok
            dm = raw.astype(f) * scale
            s = dm - Z
            ok = ok & ~(s < -trunc)
            fv = np.minimum(s / trunc, one)
            Dn = (Wt * D + fv) / (Wt + one)
            D = np.where(ok, Dn, D)
            Wt = np.where(ok, np.minimum(Wt + one, maxw), Wt)
            if audit:
                mC = COORD_ULPS * EPS32 * (p1 + float(abs(P[3]) + abs(P[7]) + abs(P[11])))
                fin = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)
                u3 = fin & (np.abs(Z - near) <= mC)
                u4 = np.zeros(D.shape, dtype=bool)
                for sc, q, fl, pp, size in ((sx, qx, S.dfx, S.du, W), (sy, qy, S.dfy, S.dv, H)):
                    mS = (fl / np.maximum(Z, near)) * (1.0 + np.abs(q)) * mC + PROJ_ULPS * EPS32 * (np.abs(sc) + abs(pp))
                    around = (sc >= -1.0) & (sc <= size)
                    u4 |= ok3 & around & (np.abs(sc - np.floor(sc) - 0.5) <= mS)
                mD = mC + DIST_ULPS * EPS32 * (dm + np.abs(Z))
                u6 = ok5 & (np.abs(s + trunc) <= mD)
                unclear[b] = u3 | u4 | u6
                bound = np.where(ok, np.maximum(bound, mD / float(trunc) + 2.0 * EPS32), bound) + np.where(ok, 3.0 * EPS32, 0.0)
            if col is not None:
                xf, yf = np.rint(qx * f(S.fx) + f(S.u)), np.rint(qy * f(S.fy) + f(S.v))
                okc = ok & (s <= trunc) & (xf >= 0) & (xf <= f(W - 1)) & (yf >= 0) & (yf <= f(H - 1))
                xc = np.where(okc, xf, 0).astype(np.int64)
                yc = np.where(okc, yf, 0).astype(np.int64)
                wc = col[..., 3]
                w1 = wc + one
                for k in range(3):
                    pix = np.asarray(frames)[b][yc, xc, k].astype(f)
                    col[..., k] = np.where(okc, (wc * col[..., k] + pix) / w1, col[..., k])
                col[..., 3] = np.where(okc, np.minimum(w1, maxw), wc)
    finally:
        np.seterr(**old)
    out = np.stack([D, Wt], axis=-1)
    if audit:
        return out, col, dict(unclear=unclear, bound=bound)
    return out, col


def _shift(a, code):
    """out[z, y, x] = a[z + dz, y + dy, x + dx], zero (False) where that lies outside the grid."""
    dx, dy, dz = code & 1, (code >> 1) & 1, (code >> 2) & 1
    out = np.zeros_like(a)
    nz, ny, nx = a.shape
    out[:nz - dz, :ny - dy, :nx - dx] = a[dz:, dy:, dx:]
    return out


def extract(tsdf, color, S, min_weight=1.0, dtype=np.float32):
    """kfn_fuse_extract_count and kfn_fuse_extract: -> (vertices [V,3] dtype, colors [V,3] uint8, triangles [N,3] int32)."""
    f = dtype
    nx, ny, nz = S.dims
    tsdf = np.asarray(tsdf, dtype=f)
    D, Wt = tsdf[..., 0], tsdf[..., 1]
    assert D.shape == (nz, ny, nx)
    valid = Wt >= f(min_weight)
    inside = valid & (D < 0)
    n = nx * ny * nz
    off = lambda code: (code & 1) + ((code >> 1) & 1) * nx + ((code >> 2) & 1) * nx * ny
    mask = np.zeros((nz, ny, nx), dtype=np.int64)
    for e, code in enumerate(EDGE_CODE):
        carry = valid & _shift(valid, code) & (inside != _shift(inside, code))
        mask |= carry.astype(np.int64) << e
    mask = mask.ravel()
    vcnt = POP[mask]
    vscan = np.cumsum(vcnt) - vcnt
    V = int(vcnt.sum())
    vertices = np.zeros((V, 3), dtype=f)
    colors = np.full((V, 3), 255, dtype=np.uint8)
    Df = D.ravel()
    colf = None if color is None else np.asarray(color, dtype=f).reshape(n, 4)
    lin = np.arange(n)
    ixyz = (lin % nx, (lin // nx) % ny, lin // (nx * ny))
    old = np.seterr(all='ignore')
    try:
        for e, code in enumerate(EDGE_CODE):
            a = np.nonzero((mask >> e) & 1)[0]
            if not len(a):
                continue
            b = a + off(code)
            ids = vscan[a] + POP[mask[a] & ((1 << e) - 1)]
            t = Df[a] / (Df[a] - Df[b])
            for k in range(3):
                pa = f(S.origin[k]) + ixyz[k][a].astype(f) * f(S.voxel)
                pb = f(S.origin[k]) + (ixyz[k][a] + ((code >> k) & 1)).astype(f) * f(S.voxel)
                vertices[ids, k] = pa + t * (pb - pa)
            if colf is not None:
                both = (colf[a, 3] > 0) & (colf[b, 3] > 0)
                for k in range(3):
                    val = np.fmin(np.fmax(np.rint(colf[a, k] + t * (colf[b, k] - colf[a, k])), f(0)), f(255))
                    colors[ids, k] = np.where(both, val, f(255)).astype(np.uint8)
    finally:
        np.seterr(**old)
    # triangles
    cube = np.zeros((nz, ny, nx), dtype=bool)
    cube[:nz - 1, :ny - 1, :nx - 1] = True
    alls, ms = [], []
    for k in range(6):
        a_ok = cube.copy()
        m = np.zeros((nz, ny, nx), dtype=np.int64)
        for j, code in enumerate(TET[k]):
            a_ok &= _shift(valid, code)
            m |= _shift(inside, code).astype(np.int64) << j
        alls.append(a_ok.ravel())
        ms.append(m.ravel())
    tcnt = np.zeros(n, dtype=np.int64)
    for k in range(6):
        tcnt += np.where(alls[k], TRI_COUNT[ms[k]], 0)
    tscan = np.cumsum(tcnt) - tcnt
    N = int(tcnt.sum())
    triangles = np.zeros((N, 3), dtype=np.int32)
    before = np.zeros(n, dtype=np.int64)
    for k in range(6):
        for m in range(1, 15):
            sel = np.nonzero(alls[k] & (ms[k] == m))[0]
            if not len(sel):
                continue
            for j, tri in enumerate(TABLE[m]):
                ids = []
                for (p, q) in tri:
                    ca, cb = TET[k][p], TET[k][q]
                    owner = sel + off(ca)
                    e = EDGE_INDEX[ca ^ cb]
                    ids.append(vscan[owner] + POP[mask[owner] & ((1 << e) - 1)])
                if TET_ODD[k]:
                    ids = [ids[0], ids[2], ids[1]]
                triangles[tscan[sel] + before[sel] + j] = np.stack(ids, axis=1)
        before += np.where(alls[k], TRI_COUNT[ms[k]], 0)
    return vertices, colors, triangles


# ---- mesh properties -----------------------------------------------------------------------------------------------------------
def edge_uses(triangles):
    """{directed edge (a, b): count}."""
    import collections
    uses = collections.Counter()
    for a, b, c in np.asarray(triangles).tolist():
        for e in ((a, b), (b, c), (c, a)):
            uses[e] += 1
    return uses


def euler(vertices_used, triangles):
    und = set((min(a, b), max(a, b)) for a, b in edge_uses(triangles))
    return vertices_used - len(und) + len(triangles)


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[triangles[:, 0]], v[triangles[:, 1]], v[triangles[:, 2]]
    return float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)


def area(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[triangles[:, 0]], v[triangles[:, 1]], v[triangles[:, 2]]
    return float(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum())


def closed_surface_checks(vertices, triangles, components=1):
    """Every undirected edge in exactly two triangles, once in each direction; V - E + F = 2 per component; no unreferenced
    vertex; positive signed volume."""
    uses = edge_uses(triangles)
    assert set(uses.values()) == {1}, 'a directed edge is used twice'
    assert all((b, a) in uses for a, b in uses), 'an edge lacks its opposite'
    used = np.unique(triangles)
    assert len(used) == len(vertices), '%d of %d vertices are referenced' % (len(used), len(vertices))
    assert euler(len(vertices), triangles) == 2 * components
    assert signed_volume(vertices, triangles) > 0


# ---- the analytic fields and the shared cases ----------------------------------------------------------------------------------
def field_volume(S, distance, valid=None):
    """A volume written directly: D = distance(p) / trunc at every lattice point (fp64 evaluation, rounded once), W = 1 or 0."""
    px, py, pz = _lattice(S, np.float64)
    nx, ny, nz = S.dims
    X, Y, Z = np.broadcast_arrays(px, py, pz)
    tsdf = np.zeros((nz, ny, nx, 2), dtype=np.float32)
    tsdf[..., 0] = (distance(X, Y, Z) / S.trunc).astype(np.float32)
    tsdf[..., 1] = 1.0 if valid is None else valid(X, Y, Z).astype(np.float32)
    return tsdf


def sphere(centre, radius):
    return lambda X, Y, Z: np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - radius


SPHERE_SETUP = dict(dims=(24, 24, 24), origin=(0.0, 0.0, 0.0), voxel=0.125)
SPHERE_CENTRE, SPHERE_RADIUS = (1.43, 1.41, 1.47), 1.03
PLANE_OFFSET = 1.3125                                          # the plane z = 1.3125: between lattice layers 10 and 11
TILTED_NORMAL, TILTED_POINT = np.array([1.0, 2.0, 8.0]), np.array([1.4, 1.3, 1.45])       # leaves the box through its walls


def analytic_fields():
    """name -> (Setup, tsdf): the volumes the host tests and the GPU tests extract from."""
    S = Setup(**SPHERE_SETUP)
    two = lambda X, Y, Z: np.minimum(sphere((0.8, 0.8, 0.8), 0.55)(X, Y, Z), sphere((2.0, 2.0, 2.0), 0.6)(X, Y, Z))
    return {
        'plane': (S, field_volume(S, lambda X, Y, Z: PLANE_OFFSET - Z)),
        'tilted_plane': (S, field_volume(S, lambda X, Y, Z: (TILTED_NORMAL[0] * (X - TILTED_POINT[0]) + TILTED_NORMAL[1] * (Y - TILTED_POINT[1]) +
                                                             TILTED_NORMAL[2] * (Z - TILTED_POINT[2])) / np.linalg.norm(TILTED_NORMAL))),
        'sphere': (S, field_volume(S, sphere(SPHERE_CENTRE, SPHERE_RADIUS))),
        'two_spheres': (S, field_volume(S, two)),
        'cut_sphere': (S, field_volume(S, sphere(SPHERE_CENTRE, SPHERE_RADIUS), valid=lambda X, Y, Z: X < 1.7)),
    }


# The integrate cases on the 19 x 13 x 11 volume over synthetic_scene(seed, cells=4): name -> what differs from the plain run.
FUSE_DIMS, FUSE_ORIGIN, FUSE_VOXEL, FUSE_TRUNC = (19, 13, 11), (-0.3, -0.1, -0.1), 0.25, 0.5
FUSE_IMAGE = (16, 24)
INTEGRATE_CASES = ('plain', 'unregistered', 'no_color', 'nan_pose', 'window', 'cap')


def render_camera(H, W):
    """The camera the frames of a case are rendered with (the colour camera): render_ref.scene_camera's numbers."""
    return dict(fx=525. * W / 640., fy=525. * W / 640., u=W / 2., v=H / 2.)


def integrate_case(name, render, seed=5, frames=3):
    """-> (Setup, depth uint16 [B,H,W], frames uint8 [B,H,W,3] or None, poses [B,4,4]).  `render(vertices, colors, triangles,
    poses, H, W, camera kwargs)` gives (depth, frames) at stride 1: the host tests pass render_ref, the GPU tests the
    Renderer.  Part of the volume lies behind each camera and part outside each image in every case."""
    from kfnet_amd import synth
    H, W = FUSE_IMAGE
    v, c, t = synth.synthetic_scene(seed, 4)
    poses = synth.synthetic_trajectory(frames + 3, seed)[3:].copy()
    cam = render_camera(H, W)
    depth, images = render(v, c, t, poses, H, W, cam)
    depth, images = np.array(depth), np.array(images)
    kw = dict(dims=FUSE_DIMS, origin=FUSE_ORIGIN, voxel=FUSE_VOXEL, trunc=FUSE_TRUNC, image_size=(H, W), **cam)
    if name == 'unregistered':
        # the depth camera sees the same scene through other intrinsics: the depth map is rendered with them
        dcam = dict(fx=cam['fx'] * 1.0625, fy=cam['fy'] * 1.125, u=cam['u'] - 0.75, v=cam['v'] + 0.5)
        depth = np.array(render(v, c, t, poses, H, W, dcam)[0])
        kw.update(dfx=dcam['fx'], dfy=dcam['fy'], du=dcam['u'], dv=dcam['v'])
    if name == 'nan_pose':
        poses[1, 2, 3] = np.nan
    if name == 'window':
        kw.update(raw_min=1500, raw_max=3000)
        depth[0, :2, :] = 0
    if name == 'cap':
        kw.update(max_weight=2.0)
    return Setup(**kw), depth, (None if name == 'no_color' else images), poses


def wall_case():
    """A wall at z = 2.1 seen by three cameras side by side, every frame uniformly (200, 100, 50): -> (Setup, depth, frames,
    poses).  Every lattice point within trunc of the wall is painted by a frame, so every vertex has the colour."""
    S = Setup(dims=(12, 10, 12), origin=(-1.375, -1.125, 0.5), voxel=0.25, trunc=1.0, fx=8.0, fy=8.0, u=12.0, v=8.0,
              image_size=(16, 24))
    depth = np.full((3, 16, 24), 2100, dtype=np.uint16)
    frames = np.empty((3, 16, 24, 3), dtype=np.uint8)
    frames[...] = (200, 100, 50)
    poses = np.stack([np.eye(4)] * 3)
    poses[1, 0, 3], poses[2, 0, 3] = 0.25, -0.25
    return S, depth, frames, poses


def hand_case():
    """The identity pose and powers of two: -> (Setup, depth, frames, poses, {what: (ix, iy, iz)}).  voxel 0.5, origin
    (-2, -1, 0.5), fx = fy = 4, u = v = 8 on a 16 x 24 image, scale 1/4, near 0.5, trunc 1.  A voxel at (x, y, z) projects to
    sx = 4 x / z + 8, sy = 4 y / z + 8.  The depth map is 12 raw units (3.0) everywhere but at pixel (row 8, column 9), which
    is invalid: in the plane z = 4 the voxel x = 0.5 has sx = 8.5 and is taken iff the tie goes down to 8, x = 1.5 has
    sx = 9.5 and is taken iff the tie goes up to 10, and x = 1 (sx = 9) is skipped."""
    S = Setup(dims=(9, 5, 8), origin=(-2.0, -1.0, 0.5), voxel=0.5, trunc=1.0, near=0.5, fx=4.0, fy=4.0, u=8.0, v=8.0,
              scale=0.25, image_size=(16, 24), max_weight=8.0)
    depth = np.full((1, 16, 24), 12, dtype=np.uint16)
    depth[0, 8, 9] = 0
    frames = np.zeros((1, 16, 24, 3), dtype=np.uint8)
    frames[...] = (200, 100, 50)
    frames[0, 8, 10] = (10, 20, 30)
    where = {
        'near': (4, 2, 0),                 # p = (0, 0, 0.5): Z == near: taken; s = 2.5 > trunc: f = 1, no colour
        'minus_trunc': (4, 2, 7),          # p = (0, 0, 4): s == -trunc: taken, f = -1, colour of pixel (8, 8)
        'plus_trunc': (4, 2, 3),           # p = (0, 0, 2): s == trunc: f = 1 and the colour taken
        'tie_down': (5, 2, 7),             # p = (0.5, 0, 4): sx = 8.5 -> 8
        'tie_up': (7, 2, 7),               # p = (1.5, 0, 4): sx = 9.5 -> 10: the colour of pixel (8, 10)
        'between': (6, 2, 7),              # p = (1, 0, 4): sx = 9: the invalid pixel
        'behind': (4, 2, 1),               # p = (0, 0, 1): in front of near, s = 2: f = 1, no colour
    }
    return S, depth, frames, np.eye(4)[None], where
