"""OFlowNet's optical flow with the reference README's "Test OFlowNet" command line:

    python -m kfnet_amd.OFlowNet.eval --input_folder I --output_folder O --model_folder M

I holds image_list.txt.  For every consecutive image pair (i-1, i), i = 1..N-1, one `flow_<i>.npy` float32 [h,w,3] =
(u, v, 1/sigma_trans) is written to O: the flow in grid cells (cell (r, c) of frame i comes from cell (r + v, c + u) of
frame i-1) and the confidence the reference's vis/vis_optical_flow*.py threshold at 100.  flow_list.txt lists the files in
order, so `vis/vis_optical_flow_list.py O/flow_list.txt I/image_list.txt out/` pairs line k with images k and k+1.  The
flow is the same whatever the sequence length: there are no resets.  Only the flow-feature tower, the cost volume and
OFlowNet run (kfnet_amd.engine.OFlowNetEngine); the model folder's newest snapshot (a TF checkpoint model.ckpt-<step> or
a kfnet_weights*.npz) may hold just the Temporal/* scope.
`--synthetic T` / `--random_weights` replace the images / the checkpoint.

Under `python -m torch.distributed.run --nproc-per-node N -m kfnet_amd.OFlowNet.eval ...` every rank processes a
contiguous chunk [lo, hi) (its first pair recomputes the features of frame lo - 1) and writes its own files, bit-identical
to a single-process run.
"""
import argparse
import os
import sys

from .. import modes
from ..tools.io import read_lines


def eval(image_paths, weights, output_folder, image_size=(480, 640), batch=4, frames=None, chunk=256, verbose=True,
         device=None, engine=None, decode_workers=None):
    """Runs the sequence, writes flow_<i>.npy (i >= 1) and flow_list.txt; returns the records [T,h,w,3] (row 0 has no
    predecessor and means nothing)."""
    from ..engine import OFlowNetEngine
    if device is None:
        import torch
        device = 'cuda:%d' % torch.cuda.current_device()
    T = len(image_paths) if frames is None else frames.shape[0]
    eng = engine if engine is not None else OFlowNetEngine(weights, image_size=image_size, batch=batch,
                                                           max_chunk=max(1, min(chunk, T)), device=device)
    records, _ = modes.run_streamed(eng, frames if frames is not None else image_paths, image_size, output_folder, 'flow',
                                    chunk=chunk, verbose=verbose, decode_workers=decode_workers)
    if output_folder and os.path.isdir(output_folder):
        modes.write_flow_list(output_folder, T)
    return records


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--input_folder', default='')
    ap.add_argument('--output_folder', default='')
    ap.add_argument('--model_folder', default='')
    modes.add_project_flags(ap)
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    rank, world, local = modes.sharded_env()
    W = modes.load_weights(a)
    if W is None:
        return 1
    import torch
    size = (a.height, a.width)
    if a.synthetic > 0:
        T, paths = a.synthetic, None
        frames_of = modes.synthetic_frames_of(a.height, a.width)
    else:
        paths = read_lines(os.path.join(a.input_folder, 'image_list.txt'))
        T = len(paths)
        frames_of = modes.image_frames_of(paths, size)
        if rank == 0:
            modes.print_banner(T)
    if world > 1:
        from ..engine import OFlowNetEngine
        from ..dist import chunk_bounds
        modes.rank_device(local)
        lo, hi = chunk_bounds(T, world, rank)
        eng = OFlowNetEngine(W, image_size=size, batch=a.batch, max_chunk=max(hi - lo, 1),
                             device='cuda:%d' % torch.cuda.current_device())
        modes.run_shard(eng, frames_of, T, rank, world, a.output_folder, 'flow')
        torch.cuda.synchronize()
        if rank == 0 and a.output_folder and os.path.isdir(a.output_folder):
            modes.write_flow_list(a.output_folder, T)
        return 0
    torch.cuda.set_device(a.gpu)
    eval(paths, W, a.output_folder, image_size=size, batch=a.batch, frames=frames_of(0, T) if paths is None else None,
         device='cuda:%d' % a.gpu)
    return 0


if __name__ == '__main__':
    sys.exit(main())
