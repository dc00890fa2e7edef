"""Times kfn_pnp_ransac at batch 20 on a 60x80 grid with 256 hypotheses (device events, after warm-up).

    python tools/mb_pnp.py [--batch 20] [--hypotheses 256] [--iters 200]

Prints one JSON line: us per batch for the whole pose stage and for the hypothesis + scoring launches alone
(kfn_pnp_hypotheses), and the scoring work's share of the fp32 vector peak from counted operations (17 VALU
instructions per point-hypothesis evaluation, pnp_score_kernel's inner loop; peak = 256 CUs x 4 SIMDs x 32 lanes x
2.4 GHz).  Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))

OPS_PER_EVAL = 17
VALU_PEAK = 256 * 4 * 32 * 2.4e9     # fp32 lane-instructions per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=20)
    ap.add_argument('--hypotheses', type=int, default=256)
    ap.add_argument('--h', type=int, default=60)
    ap.add_argument('--w', type=int, default=80)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    a = ap.parse_args()
    import torch
    import pnp_ref as P
    from kfnet_amd.KFNet.pnp import PnPSolver
    rng = np.random.default_rng(0)
    recs = []
    for _ in range(a.batch):
        R, t = P.random_pose(rng)
        rec = P.synthetic_records(rng, a.h, a.w, R, t)
        rec[..., :3] += rng.normal(scale=0.01, size=rec[..., :3].shape).astype(np.float32)
        out = rng.random((a.h, a.w)) < 0.5
        rec[..., :3][out] = rng.uniform(-5, 5, size=(int(out.sum()), 3)).astype(np.float32)
        recs.append(rec)
    dev = torch.from_numpy(np.stack(recs)).cuda()
    solver = PnPSolver(a.h, a.w, hypotheses=a.hypotheses)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    us_ransac = timed(lambda: solver.solve(dev))
    _, info = solver.solve(dev)
    # hypotheses + scoring alone, on preallocated outputs
    import ctypes as C
    from kfnet_amd import _lib
    lib = _lib.load()
    B, H = a.batch, a.hypotheses
    samples = torch.empty((B, H, 4), dtype=torch.int32, device='cuda')
    hp = torch.empty((B, H, 12), dtype=torch.float32, device='cuda')
    counts = torch.empty((B, H), dtype=torch.int32, device='cuda')
    d = solver.desc(B, 0, 4)
    stream = torch.cuda.current_stream().cuda_stream
    us_hyp_score = timed(lambda: _lib.check(lib.kfn_pnp_hypotheses(C.byref(d), dev.data_ptr(), samples.data_ptr(),
                                                                   hp.data_ptr(), counts.data_ptr(), stream)))
    evals = B * H * a.h * a.w
    print(json.dumps({
        'batch': B, 'grid': [a.h, a.w], 'hypotheses': H,
        'us_per_batch': round(us_ransac, 2),
        'us_hypotheses_and_scoring': round(us_hyp_score, 2),
        'point_hypothesis_evals': evals,
        'scoring_floor_us': round(evals * OPS_PER_EVAL / VALU_PEAK * 1e6, 2),
        'scoring_share_of_valu_peak_if_all_of_hyp_and_scoring': round(evals * OPS_PER_EVAL / VALU_PEAK / (us_hyp_score * 1e-6), 3),
        'solved': int((info[:, 0] == 0).sum().item()),
        'target_us': 50.0,
    }))


if __name__ == '__main__':
    main()
