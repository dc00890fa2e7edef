"""Times restoring a full-size KFNet from a TF V2 checkpoint (kfnet_amd/checkpoint.py) and prints one JSON line.

    python tools/mb_checkpoint.py [--dir D] [--height 480 --width 640 --batch 4]

Writes a training-style checkpoint of synthetic_weights with the test writer (tests/tf_bundle_writer.py: every model
variable, both Adam slots, beta*_power, global_step; about 300 MB, of which about 100 MB are model variables), then splits
one load into: opening the index, reading the model tensors' bytes, their CRC-32C (kfn_crc32c), and KFNetEngine's
Graph.load_weights (packing + upload).  The file was just written, so its reads come from the page cache.  `crc_path`
names the implementation kfn_crc32c picks: the CPU's SSE4.2 crc32 instruction when /proc/cpuinfo lists sse4_2.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))


def _sse42():
    try:
        with open('/proc/cpuinfo') as f:
            return any(line.startswith('flags') and ' sse4_2' in line for line in f)
    except OSError:
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dir', default=None, help='where to write the checkpoint (default: a temporary directory)')
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--batch', type=int, default=4)
    a = ap.parse_args()
    import numpy as np
    import torch
    import tf_bundle_writer as TW
    from kfnet_amd import checkpoint as CK
    from kfnet_amd.engine import KFNetEngine
    from kfnet_amd.weights import synthetic_weights
    d = a.dir or tempfile.mkdtemp(prefix='kfn_ckpt_')
    try:
        W = synthetic_weights(1234)
        prefix = os.path.join(d, 'model.ckpt-2500')
        t0 = time.perf_counter()
        TW.training_checkpoint(prefix, W, step=2500)
        write_s = time.perf_counter() - t0
        file_bytes = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
        buf = np.random.default_rng(0).integers(0, 256, 64 << 20, dtype=np.uint8)
        CK.crc32c(buf)
        t0 = time.perf_counter()
        CK.crc32c(buf)
        crc_gbps = buf.nbytes / (time.perf_counter() - t0) / 1e9
        eng = KFNetEngine(W, image_size=(a.height, a.width), batch=a.batch, max_chunk=8, device='cuda:0')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ck = CK.Checkpoint(prefix)
        open_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        got, ck2 = CK.restore(prefix)
        restore_s = time.perf_counter() - t0
        assert all(np.array_equal(got[k], W[k]) for k in W) and len(got) == len(W)
        t0 = time.perf_counter()
        eng.graph.load_weights(got)
        torch.cuda.synchronize()
        upload_s = time.perf_counter() - t0
        tm = ck2.timings
        print(json.dumps(dict(
            tool='mb_checkpoint', file_mb=round(file_bytes / 1e6, 1), tensors=len(ck.names()), restored=len(got),
            read_mb=round(tm['bytes'] / 1e6, 1), open_index_s=round(open_s, 4), read_s=round(tm['read'], 4),
            crc_s=round(tm['crc'], 4), restore_total_s=round(restore_s, 4), engine_load_weights_s=round(upload_s, 4),
            crc_path='sse4.2' if _sse42() else 'table', crc_gb_per_s=round(crc_gbps, 2),
            write_s=round(write_s, 2), image_size=[a.height, a.width], batch=a.batch)))
    finally:
        if a.dir is None:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
