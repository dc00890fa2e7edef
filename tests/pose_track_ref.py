"""numpy fp64 restatement of kfn_pose_track (DESIGN.md 5c "Pose tracker"): kfn_pose_filter's recursion under the walk or the
constant-velocity model, the backward (Rauch-Tung-Striebel) pass over the frames of a call, and the carried state.  On top
of pnp_unc_ref (flags, log_so3, the trajectories) and pnp_ref (rodrigues)."""
import numpy as np

import pnp_ref as P
import pnp_unc_ref as U

UPDATED, MISSING, REJECTED, INIT, NONE = U.UPDATED, U.MISSING, U.REJECTED, U.INIT, U.NONE
DEFAULT_SIGMA = {'walk': 0.02, 'velocity': 0.005}


def _f32(x):
    return float(np.float32(x))


def transition(n):
    """F: the identity for the walk, [[I6, I6], [0, I6]] for the velocity model."""
    F = np.eye(n)
    if n == 12:
        F[:6, 6:] = np.eye(6)
    return F


def process_noise(n, qr, qt):
    """Q: diag(qr I3, qt I3) for the walk; per axis [[q/3, q/2], [q/2, q]] on (pose axis, rate axis) for the velocity model."""
    q = np.array([qr] * 3 + [qt] * 3)
    if n == 6:
        return np.diag(q)
    Q = np.zeros((12, 12))
    Q[:6, :6] = np.diag(q / 3.0)
    Q[:6, 6:] = Q[6:, :6] = np.diag(q / 2.0)
    Q[6:, 6:] = np.diag(q)
    return Q


def _mirror(M):
    return np.triu(M) + np.triu(M, 1).T


def _predict_cov(Pm, n, Q):
    """F P F^T + Q; for n = 12 block by block as the device: ((A + B) + B^T) + D mirrored, B + D, D."""
    if n == 6:
        return Pm + Q
    A, B, D = Pm[:6, :6], Pm[:6, 6:], Pm[6:, 6:]
    out = np.empty((12, 12))
    out[:6, :6] = _mirror(((A + B) + B.T) + D)
    out[:6, 6:] = B + D
    out[6:, :6] = (B + D).T
    out[6:, 6:] = D
    return out + Q


def new_state():
    """The state of one sequence: 'no estimate yet' (the device's all-zero buffer)."""
    return dict(have=False, rejects=0, R=None, p=None, xi=np.zeros(6), P=None)


def track(poses, cov, model='walk', smooth=False, rot_sigma=None, trans_sigma=None, rot_rate_sigma=0.05,
          trans_rate_sigma=0.05, gate=22.46, max_rejects=3, state=None, solve='cholesky'):
    """kfn_pose_track on one sequence: poses [T,4,4], cov [T,6,6] (as the device reads them: fp32 values) ->
    (poses [T,4,4], cov [T,6,6], flags [T], nis [T]) in fp64, with `smooth` also (smoothed poses, smoothed cov).  The
    descriptor's floats are rounded to fp32 as the descriptor holds them.  `state`: a new_state() dict that is read and
    updated (None: a fresh one).  solve = 'cholesky' factors S and P_p once as the device does, 'lu' uses
    numpy.linalg.solve for both."""
    poses = np.asarray(poses, np.float32).astype(np.float64)
    cov = np.asarray(cov, np.float32).astype(np.float64)
    T = poses.shape[0]
    n = {'walk': 6, 'velocity': 12}[model]
    rot_sigma = DEFAULT_SIGMA[model] if rot_sigma is None else rot_sigma
    trans_sigma = DEFAULT_SIGMA[model] if trans_sigma is None else trans_sigma
    qr, qt = _f32(rot_sigma) ** 2, _f32(trans_sigma) ** 2
    rr, rt = _f32(rot_rate_sigma) ** 2, _f32(trans_rate_sigma) ** 2
    gate = _f32(gate)
    F, Q = transition(n), process_noise(n, qr, qt)
    out_p = np.full((T, 4, 4), np.nan)
    out_c = np.full((T, 6, 6), np.nan)
    flags = np.zeros(T, np.int64)
    nis = np.full(T, np.nan)
    st = new_state() if state is None else state
    have, rejects, R, p, xi, Pm = st['have'], st['rejects'], st['R'], st['p'], st['xi'].copy(), st['P']
    filt, pred = [None] * T, [None] * T          # per frame (R, p, xi, P)
    for k in range(T):
        Z, Sz = poses[k], cov[k]
        valid = bool(np.isfinite(Z[:3]).all() and np.isfinite(Sz).all())
        init = False
        if not have:
            flag, init = (INIT, True) if valid else (NONE, False)
        else:
            if n == 12:
                p = p + R @ xi[3:]
                R = R @ P.rodrigues(xi[:3])
            Pm = _predict_cov(Pm, n, Q)
            pred[k] = (R.copy(), p.copy(), xi.copy(), Pm.copy())
            flag = MISSING
            if valid:
                y = np.concatenate([U.log_so3(R.T @ Z[:3, :3]), R.T @ (Z[:3, 3] - p)])
                S = Pm[:6, :6] + Sz
                try:
                    L = np.linalg.cholesky(S)
                except np.linalg.LinAlgError:
                    L = None
                if L is not None:
                    if solve == 'cholesky':
                        uu = np.linalg.solve(L, y)
                        nis[k] = float(uu @ uu)
                        K = np.linalg.solve(L.T, np.linalg.solve(L, Pm[:6, :])).T
                    else:
                        nis[k] = float(y @ np.linalg.solve(S, y))
                        K = np.linalg.solve(S, Pm[:6, :]).T
                    if nis[k] > gate:
                        rejects += 1
                        flag = REJECTED
                        if rejects >= max_rejects:
                            flag, init = INIT, True
                    else:
                        d = K @ y
                        p = p + R @ d[3:6]
                        R = R @ P.rodrigues(d[:3])
                        if n == 12:
                            xi = xi + d[6:]
                        A = np.eye(n)
                        A[:, :6] -= K
                        Pm = _mirror(A @ Pm @ A.T + K @ Sz @ K.T)
                        flag, rejects = UPDATED, 0
        if init:
            R, p, xi = Z[:3, :3].copy(), Z[:3, 3].copy(), np.zeros(6)
            Pm = np.zeros((n, n))
            Pm[:6, :6] = Sz
            if n == 12:
                Pm[6:, 6:] = np.diag([rr] * 3 + [rt] * 3)
            have, rejects = True, 0
        if have:
            out_p[k] = np.eye(4)
            out_p[k, :3, :3], out_p[k, :3, 3] = R, p
            out_c[k] = Pm[:6, :6]
            filt[k] = (R.copy(), p.copy(), xi.copy(), Pm.copy())
        flags[k] = flag
    if state is not None:
        state.update(have=have, rejects=rejects, R=R, p=p, xi=xi, P=Pm)
    if not smooth:
        return out_p, out_c, flags, nis
    sm_p = np.full((T, 4, 4), np.nan)
    sm_c = np.full((T, 6, 6), np.nan)
    nxt = None
    for k in range(T - 1, -1, -1):
        if filt[k] is None:
            nxt = None
            continue
        Rf, pf, xf, Pf = filt[k]
        cur = filt[k]
        if nxt is not None and flags[k + 1] != INIT:
            Rs, ps, xs, Ps = nxt
            Rp, pp, xp, Pp = pred[k + 1]
            try:
                L = np.linalg.cholesky(Pp)
            except np.linalg.LinAlgError:
                L = None
            if L is not None:
                e = np.concatenate([U.log_so3(Rp.T @ Rs), Rp.T @ (ps - pp), xs - xp])[:n]
                G = Pf @ F.T
                if solve == 'cholesky':
                    C = np.linalg.solve(L.T, np.linalg.solve(L, G.T)).T
                else:
                    C = np.linalg.solve(Pp, G.T).T
                d = C @ e
                xn = xf + d[6:] if n == 12 else xf
                cur = (Rf @ P.rodrigues(d[:3]), pf + Rf @ d[3:6], xn, _mirror(Pf + C @ (Ps - Pp) @ C.T))
        sm_p[k] = np.eye(4)
        sm_p[k, :3, :3], sm_p[k, :3, 3] = cur[0], cur[1]
        sm_c[k] = cur[3][:6, :6]
        nxt = cur
    return out_p, out_c, flags, nis, sm_p, sm_c
