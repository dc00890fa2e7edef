"""Restatements of kfn_render (include/kfnet_hip.h) in numpy.

render(..., dtype=np.float32) follows the header's fp32 operations one by one, in their order, so it reproduces the
device's bits.  render(..., dtype=np.float64, candidates=True) is the same definition in fp64, written for clarity as a
loop over triangles into a z-buffer; beside the image it keeps, per sample, every triangle that covers it or comes within
the margins below of covering it, sorted by depth: what the float32 run is judged against.

The camera constants are the fp32-rounded ones in both runs (kfnet_amd.render.render_descriptor), so the two differ by the
arithmetic alone.

Margins (derived in DESIGN.md 6j from the stated operation sequence, eps = 2^-24):
    a projected vertex is off by at most          dv = VERTEX_ULPS eps (f (|X| + |Y| + |Z|) / Z (1 + max(|x'|, |y'|)) + max(|u|, |v|))
    an edge function at a sample by at most       EDGE_ULPS eps (|ex| + |ey|) M + 2 (|ex| + |ey|) dv,  M the largest coordinate
                                                  of the polygon or the image
    a depth, relatively, by at most               DEPTH_ULPS eps (1 + D / L),  D the largest camera coordinate of the triangle,
                                                  L its shortest edge
"""
import numpy as np

EPS32 = 2.0 ** -24
VERTEX_ULPS = 8.0
EDGE_ULPS = 8.0
DEPTH_ULPS = 32.0
FLT_MAX = float(np.finfo(np.float32).max)


class Camera(object):
    """The constants of kfn_render_desc as floats that fp32 holds exactly."""

    def __init__(self, fx=525., fy=525., u=320., v=240., scale=0.001, raw_min=1, raw_max=65534, near=0.05):
        r = lambda x: float(np.float32(x))
        self.fx, self.fy, self.u, self.v = r(fx), r(fy), r(u), r(v)
        self.inv_fx, self.inv_fy = r(1.0 / fx), r(1.0 / fy)
        self.scale, self.near = r(scale), r(near)
        self.raw_min, self.raw_max = int(raw_min), int(raw_max)


def pose_rows32(poses):
    p = np.asarray(poses, dtype=np.float64)
    if p.ndim == 3:
        p = p[:, :3, :].reshape(p.shape[0], 12)
    return np.ascontiguousarray(p, dtype=np.float32)


def _to_camera(P, v):
    dx, dy, dz = v[:, 0] - P[3], v[:, 1] - P[7], v[:, 2] - P[11]
    X = (P[0] * dx + P[4] * dy) + P[8] * dz
    Y = (P[1] * dx + P[5] * dy) + P[9] * dz
    Z = (P[2] * dx + P[6] * dy) + P[10] * dz
    return np.stack([X, Y, Z], axis=1)


def _polygon(c, inside, cam, f):
    """The projected polygon of one triangle (scalars of type f): list of (sx, sy), ok, the vertex error bound."""
    near, fx, fy, u, v = f(cam.near), f(cam.fx), f(cam.fy), f(cam.u), f(cam.v)
    out, ok, dv = [], True, 0.0

    def emit(x, y, z):
        nonlocal ok, dv
        xn, yn = x / z, y / z
        sx, sy = xn * fx + u, yn * fy + v
        if not (np.isfinite(sx) and np.isfinite(sy)):
            ok = False
        else:
            dv = max(dv, VERTEX_ULPS * EPS32 * (max(cam.fx, cam.fy) * float((abs(x) + abs(y) + abs(z)) / z) *
                                                 (1.0 + max(abs(float(xn)), abs(float(yn)))) + max(abs(cam.u), abs(cam.v))))
        if out and sx == out[-1][0] and sy == out[-1][1]:
            return
        if len(out) < 4:
            out.append((sx, sy))

    for k in range(3):
        cur, nxt = c[k], c[(k + 1) % 3]
        ic, inx = inside[k], inside[(k + 1) % 3]
        if ic:
            emit(cur[0], cur[1], cur[2])
        if ic != inx:
            I, O = (cur, nxt) if ic else (nxt, cur)
            tt = (I[2] - near) / (I[2] - O[2])
            emit(I[0] + tt * (O[0] - I[0]), I[1] + tt * (O[1] - I[1]), near)
    if len(out) > 1 and out[-1][0] == out[0][0] and out[-1][1] == out[0][1]:
        out.pop()
    if len(out) < 3:
        ok = False
    return out, ok, dv


def _edges(q, f):
    """[(ax, ay, ex, ey, s, tie)] of a polygon, or None when an edge's reference vertex lies on it."""
    n, edges = len(q), []
    for k in range(n):
        j = (k + 1) % n
        m = (j + 1) % n
        swap = q[k][0] > q[j][0] or (q[k][0] == q[j][0] and q[k][1] > q[j][1])
        (ax, ay), (bx, by) = (q[j], q[k]) if swap else (q[k], q[j])
        ex, ey = bx - ax, by - ay
        g = ex * (q[m][1] - ay) - ey * (q[m][0] - ax)
        if not (g > 0 or g < 0):
            return None
        s = f(1.0) if g > 0 else f(-1.0)
        ga, gb = -s * ey, s * ex
        edges.append((ax, ay, ex, ey, s, bool(ga > 0 or (ga == 0 and gb > 0))))
    return edges


def render(vertices, colors, triangles, poses, H, W, stride, cam, dtype=np.float32, candidates=False):
    """-> dict(labels [B,h,w,4] dtype, depth uint16, frames uint8, stats int32 [B,5], winner int64 (-1: none), z dtype) and,
    with candidates, cand: {(b, r, c): [(z, t, clearly_inside, relative depth margin)] sorted}."""
    f = dtype
    vertices = np.asarray(vertices, dtype=np.float32).astype(f)
    triangles = np.asarray(triangles, dtype=np.int64)
    P_all = pose_rows32(poses).astype(f)
    B, V, N = P_all.shape[0], vertices.shape[0], triangles.shape[0]
    h, w, s = H // stride, W // stride, stride
    near = f(cam.near)
    zb = np.full((B, h, w), np.inf, dtype=f)
    win = np.full((B, h, w), -1, dtype=np.int64)
    stats = np.zeros((B, 5), dtype=np.int32)
    cand = dict()
    valid_ix = ((triangles >= 0) & (triangles < V)).all(axis=1)
    inv_s = f(1.0 / s)
    old = np.seterr(all='ignore')
    try:
        for b in range(B):
            P = P_all[b]
            if not np.isfinite(P).all():
                stats[b, 3] = 1
                continue
            stats[b, 4] = int((~valid_ix).sum())
            cv = _to_camera(P, vertices)                                    # [V,3]
            tri = np.where(valid_ix[:, None], triangles, 0)
            c = cv[tri]                                                     # [N,3 vertices,3]
            fin = np.isfinite(c).all(axis=(1, 2))
            inside = c[:, :, 2] >= near
            passed = valid_ix & fin & inside.any(axis=1)
            stats[b, 1] = int(passed.sum())
            stats[b, 2] = int((passed & ~inside.all(axis=1)).sum())
            e1, e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
            nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
            ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
            nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            d = (nx * c[:, 0, 0] + ny * c[:, 0, 1]) + nz * c[:, 0, 2]
            pa, pb, pc = nx / d, ny / d, nz / d
            plane_ok = (d != 0) & np.isfinite(pa) & np.isfinite(pb) & np.isfinite(pc)
            todo = passed & plane_ok
            # unclipped triangles whose box holds no sample are dropped here, by the same numbers as below
            sx = (c[:, :, 0] / c[:, :, 2]) * f(cam.fx) + f(cam.u)
            sy = (c[:, :, 1] / c[:, :, 2]) * f(cam.fy) + f(cam.v)
            pad = float(s) if candidates else 0.0
            lo_x, hi_x = np.maximum(sx.min(axis=1) - f(pad), f(0)), np.minimum(sx.max(axis=1) + f(pad), f(W - 1))
            lo_y, hi_y = np.maximum(sy.min(axis=1) - f(pad), f(0)), np.minimum(sy.max(axis=1) + f(pad), f(H - 1))
            empty = ~((np.ceil(lo_x * inv_s) <= np.floor(hi_x * inv_s)) & (np.ceil(lo_y * inv_s) <= np.floor(hi_y * inv_s)))
            todo &= ~(inside.all(axis=1) & empty & np.isfinite(sx).all(axis=1) & np.isfinite(sy).all(axis=1))
            for t in np.nonzero(todo)[0]:
                q, ok, dv = _polygon(c[t], inside[t], cam, f)
                if not ok:
                    continue
                edges = _edges(q, f)
                if edges is None:
                    continue
                xs, ys = [p[0] for p in q], [p[1] for p in q]
                mnx, mxx = max(min(xs) - f(pad), f(0)), min(max(xs) + f(pad), f(W - 1))
                mny, mxy = max(min(ys) - f(pad), f(0)), min(max(ys) + f(pad), f(H - 1))
                if not (mnx <= mxx and mny <= mxy):
                    continue
                c_lo, c_hi = int(np.ceil(mnx * inv_s)), int(np.floor(mxx * inv_s))
                r_lo, r_hi = int(np.ceil(mny * inv_s)), int(np.floor(mxy * inv_s))
                if not (c_lo <= c_hi and r_lo <= r_hi):
                    continue
                px = (np.arange(c_lo, c_hi + 1) * s).astype(f)[None, :]
                py = (np.arange(r_lo, r_hi + 1) * s).astype(f)[:, None]
                covered = np.ones((r_hi - r_lo + 1, c_hi - c_lo + 1), dtype=bool)
                near_in = covered.copy()          # not clearly outside
                clear_in = covered.copy()         # clearly inside
                M = max(max(abs(float(x)) for x in xs), max(abs(float(y)) for y in ys), float(W), float(H))
                for (ax, ay, ex, ey, sg, tie) in edges:
                    tt = sg * (ex * (py - ay) - ey * (px - ax))
                    covered &= (tt > 0) | ((tt == 0) & tie)
                    if candidates:
                        span = abs(float(ex)) + abs(float(ey))
                        margin = EDGE_ULPS * EPS32 * span * M + 2.0 * span * dv
                        near_in &= tt > -margin
                        clear_in &= tt >= margin
                rx, ry = (px - f(cam.u)) * f(cam.inv_fx), (py - f(cam.v)) * f(cam.inv_fy)
                ww = (pa[t] * rx + pb[t] * ry) + pc[t]
                z = f(1.0) / ww
                front = (ww > 0) & (z <= FLT_MAX)
                hit = covered & front
                zs, ws = zb[b, r_lo:r_hi + 1, c_lo:c_hi + 1], win[b, r_lo:r_hi + 1, c_lo:c_hi + 1]
                better = hit & ((z < zs) | ((z == zs) & ((t < ws) | (ws < 0))))
                zs[better] = z[better]
                ws[better] = t
                if candidates:
                    L = min(float(np.abs(e1[t]).sum()), float(np.abs(e2[t]).sum()), float(np.abs(e2[t] - e1[t]).sum()))
                    zrel = DEPTH_ULPS * EPS32 * (1.0 + float(np.abs(c[t]).max()) / max(L, 1e-30))
                    for rr, cc in zip(*np.nonzero(near_in & front)):
                        cand.setdefault((b, r_lo + int(rr), c_lo + int(cc)), []).append(
                            (float(z[rr, cc]), int(t), bool(clear_in[rr, cc]), zrel))
        out = _resolve(vertices, colors, triangles, P_all, zb, win, cam, s, f)
    finally:
        np.seterr(**old)
    stats[:, 0] = (win >= 0).reshape(B, -1).sum(axis=1)
    out.update(stats=stats, winner=win, z=np.where(win >= 0, zb, f(0)))
    if candidates:
        for k in cand:
            cand[k].sort()
        out['cand'] = cand
    return out


def _resolve(vertices, colors, triangles, P_all, zb, win, cam, s, f):
    B, h, w = win.shape
    labels = np.zeros((B, h, w, 4), dtype=f)
    depth = np.zeros((B, h, w), dtype=np.uint16)
    frames = np.zeros((B, h, w, 3), dtype=np.uint8)
    px = (np.arange(w) * s).astype(f)[None, :]
    py = (np.arange(h) * s).astype(f)[:, None]
    rx, ry = (px - f(cam.u)) * f(cam.inv_fx), (py - f(cam.v)) * f(cam.inv_fy)
    for b in range(B):
        P = P_all[b]
        got = win[b] >= 0
        if not got.any():
            continue
        z = np.where(got, zb[b], f(1.0))
        X, Y = rx * z, ry * z
        q = np.rint(z / f(cam.scale))
        valid = got & (q >= f(cam.raw_min)) & (q <= f(cam.raw_max))
        depth[b] = np.where(valid, q, 0).astype(np.uint16)
        for i in range(3):
            labels[b, :, :, i] = np.where(valid, ((P[4 * i] * X + P[4 * i + 1] * Y) + P[4 * i + 2] * z) + P[4 * i + 3], f(0))
        labels[b, :, :, 3] = valid.astype(f)
        cv = _to_camera(P, vertices)
        tri = triangles[np.where(got, win[b], 0)]                       # [h,w,3]
        c0, c1, c2 = cv[tri[..., 0]], cv[tri[..., 1]], cv[tri[..., 2]]
        hit = np.stack([X, Y, z], axis=-1)
        dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
        f1, f2, hp = c1 - c0, c2 - c0, hit - c0
        d11, d12, d22, h1, h2 = dot(f1, f1), dot(f1, f2), dot(f2, f2), dot(hp, f1), dot(hp, f2)
        den = d11 * d22 - d12 * d12
        b1 = (d22 * h1 - d12 * h2) / den
        b2 = (d11 * h2 - d12 * h1) / den
        b0 = (f(1.0) - b1) - b2
        for k in range(3):
            if colors is None:
                k0 = k1 = k2 = f(255.0)
            else:
                col = np.asarray(colors)[:, k].astype(f)
                k0, k1, k2 = col[tri[..., 0]], col[tri[..., 1]], col[tri[..., 2]]
            val = np.fmin(np.fmax(np.rint((b0 * k0 + b1 * k1) + b2 * k2), f(0)), f(255))
            frames[b, :, :, k] = np.where(got & np.isfinite(val), val, 0).astype(np.uint8)
    return dict(labels=labels, depth=depth, frames=frames)


def classify(ref):
    """From an fp64 run with candidates: clear [B,h,w] bool (covered samples whose every candidate is clearly inside and
    whose two nearest candidates are further apart than their depth margins), and allowed {sample: set of winners a float32
    run may report, -1 for none} for the covered or nearly covered samples that are not clear."""
    win = ref['winner']
    clear = np.zeros(win.shape, dtype=bool)
    allowed = dict()
    for key, lst in ref['cand'].items():
        ok = all(x[2] for x in lst)
        if ok and len(lst) > 1:
            ok = lst[1][0] - lst[0][0] > (lst[0][3] + lst[1][3]) * lst[1][0]
        if ok:
            clear[key] = True
            assert win[key] == lst[0][1]
        else:
            z0 = min((x[0] for x in lst if x[2]), default=np.inf)          # the nearest certain hit bounds the rest
            a = set(x[1] for x in lst if x[0] * (1.0 - x[3]) <= z0 * (1.0 + x[3]))
            if not any(x[2] for x in lst):
                a.add(-1)
            allowed[key] = a
    return clear, allowed


# ---- the cases shared by tests/test_render_host.py and tests/test_gpu_render.py ---------------------------------------------
IDENTITY = np.eye(4)[None]


def hand_camera(**kw):
    """1-pixel units: pixel (x, y) is the ray (x, y, 1); every constant a power of two, so the hand cases are exact in fp32."""
    return Camera(**dict(dict(fx=1., fy=1., u=0., v=0., scale=0.25, raw_min=1, raw_max=65534, near=0.5), **kw))


def _mesh(*tris):
    v = np.asarray([p for t in tris for p in t], dtype=np.float32)
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)


def hand_cases():
    """name -> (vertices, triangles, camera); identity pose, a 16x24 image at stride 1."""
    A = ((0, 0, 1), (8, 0, 1), (0, 8, 1))
    fan_v = np.asarray([(0, 0, 1), (8, 0, 1), (8, 8, 1), (0, 8, 1), (4, 4, 1)], dtype=np.float32)
    return {
        'one': _mesh(A) + (hand_camera(),),
        'shared_edge': _mesh(((0, 0, 1), (8, 0, 1), (8, 8, 1)), ((0, 0, 1), (8, 8, 1), (0, 8, 1))) + (hand_camera(),),
        'fan': (fan_v, np.asarray([(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4)], dtype=np.int32), hand_camera()),
        'sliver': _mesh(((1, 0, 4), (1, 40, 4), (3, 20, 4))) + (hand_camera(),),
        'twice': _mesh(A, A) + (hand_camera(),),
        'near_first': _mesh(A, ((0, 0, 2), (16, 0, 2), (0, 16, 2))) + (hand_camera(),),
        'near_last': _mesh(((0, 0, 2), (16, 0, 2), (0, 16, 2)), A) + (hand_camera(),),
        'behind': _mesh(((0, 0, -1), (8, 0, -1), (0, 8, -1))) + (hand_camera(),),
        'clip_one': _mesh(((0, 0, 1), (8, 0, 1), (0, 4, -1))) + (hand_camera(),),
        'clip_two': _mesh(((0, 0, 1), (8, 0, -1), (0, 8, -1))) + (hand_camera(),),
        'huge': _mesh(((-1000, -1000, 1), (3000, -1000, 1), (-1000, 3000, 1))) + (hand_camera(),),
        'tie': _mesh(((0, 0, 2), (16, 0, 2), (0, 16, 2)), ((24, 0, 6), (48, 0, 6), (48, 96, 6))) + (hand_camera(scale=4.0),),
        'beyond': _mesh(A, ((16, 0, 2), (32, 0, 2), (32, 16, 2))) + (hand_camera(raw_max=6),),
    }


def scene_camera(H, W):
    """7-Scenes' camera scaled to a W-wide image."""
    return Camera(fx=525. * W / 640., fy=525. * W / 640., u=W / 2., v=H / 2.)


# (H, W, stride, cells, frames, seed): the random cases; beside each, what the fp64 run alone shows (chosen on the CPU):
# covered samples and how many of them are not clear.  The condition is that at most 2 % are unclear.
RANDOM_CASES = (
    ((16, 24, 1, 4, 1, 5), (384, 1)),
    ((16, 24, 1, 4, 3, 1), (1152, 2)),
    ((64, 96, 8, 4, 2, 2), (192, 0)),
    ((64, 96, 1, 16, 1, 3), (6144, 14)),
)


def scene_case(H, W, stride, cells, frames, seed):
    from kfnet_amd import synth
    v, c, t = synth.synthetic_scene(seed, cells)
    poses = synth.synthetic_trajectory(frames + 3, seed)[3:]
    return v, c, t, poses, scene_camera(H, W)
