"""Builds kfnet_amd/libkfnet_hip.so (the C-ABI HIP library) in-tree for gfx950.

    python -m kfnet_amd.build [--force]

hipcc cross-compiles without a GPU.  Objects are cached under kfnet_amd/csrc/build/ and
rebuilt when a source or header is newer.  The built .so is git-ignored but travels to
the GPU box with the repo snapshot.
"""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
OBJ = os.path.join(CSRC, 'build')
LIB = os.path.join(HERE, 'libkfnet_hip.so')
HEADERS = [os.path.join(CSRC, 'kfn_common.h'), os.path.join(CSRC, 'kfn_train_shared.h'),
           os.path.join(os.path.dirname(HERE), 'include', 'kfnet_hip.h')]

ARCH = 'gfx950'
COMMON = ['--offload-arch=' + ARCH, '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function']
# per-file extra flags
EXTRA = {
    # the Kalman/warp kernel reproduces the reference's unfused elementwise arithmetic
    'kfn_kalman.hip': ['-ffp-contract=off'],
    # the metrics kernel restates TF elementwise ops whose results are thresholded and counted
    'kfn_metrics.hip': ['-ffp-contract=off'],
    # ApplyTransform / bilinear_sampler as stand-alone launches: the same unfused arithmetic as inside the scan
    'kfn_util_ops.hip': ['-ffp-contract=off'],
    # the training loss clips, thresholds and counts per-pixel terms, like the metrics kernel
    'kfn_train_loss.hip': ['-ffp-contract=off'],
    # the augmentation's index arithmetic and interpolation are a list of rounded fp32 operations
    'kfn_augment.hip': ['-ffp-contract=off'],
    # labels from depth maps: back-projection and pose as a list of rounded fp32 operations
    'kfn_labels.hip': ['-ffp-contract=off'],
    # the filter's loss and reverse scan: the loss's per-pixel terms and the forward scan's sampler weights, rounded alike
    'kfn_train_filter.hip': ['-ffp-contract=off'],
    # training OFlowNet: the loss's per-cell terms as the filter's, and gather sums that a sequential fp32 restatement repeats
    'kfn_train_flow.hip': ['-ffp-contract=off'],
    # the guarded Adam step repeats kfn_train_loss.hip's fp64 arithmetic, which a numpy restatement follows bit for bit
    'kfn_loss_scale.hip': ['-ffp-contract=off'],
    # the pose filter: a serial fp64 recursion per sequence, rounded product by product as its numpy restatement, like the scan
    'kfn_pose_filter.hip': ['-ffp-contract=off'],
    # the pose tracker: the filter's recursion under two motion models and its backward pass, rounded as their restatement
    'kfn_pose_track.hip': ['-ffp-contract=off'],
    # the reprojection loss: per-cell terms as the other loss launches' 
    'kfn_reproj.hip': ['-ffp-contract=off'],
    # the mesh renderer: transform, clipping, edge functions and depth as a list of rounded fp32 operations
    'kfn_render.hip': ['-ffp-contract=off'],
    # fusion and mesh extraction: projection, the running averages and the crossings as a list of rounded fp32 operations
    'kfn_fuse.hip': ['-ffp-contract=off'],
    # tracking against the volume: maps, ray cast and ICP rows as a list of rounded fp32 operations, the solve in unfused fp64
    'kfn_track.hip': ['-ffp-contract=off'],
    # relocalisation from fern-coded keyframes: integer tests and copies of fp64 poses, built like the tracker it sits in
    'kfn_reloc.hip': ['-ffp-contract=off'],
    # RANSAC-Kabsch: fp64 sums, Jacobi rotations and the covariance rounded product by product like the pose filter; the fp32
    # scoring fuses by explicit fmaf only (DESIGN.md 5c "Poses with depth")
    'kfn_kabsch.hip': ['-ffp-contract=off'],
}


def _hipcc():
    for c in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if c and os.path.exists(c):
            return c
    raise RuntimeError('hipcc not found (need ROCm with gfx950 support)')


def sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith('.hip'))


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    hipcc = _hipcc()
    os.makedirs(OBJ, exist_ok=True)
    jobs = []
    objs = []
    for src in sources():
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, src.replace('.hip', '.o'))
        objs.append(o)
        if force or _stale(o, [s] + HEADERS):
            jobs.append([hipcc] + COMMON + EXTRA.get(src, []) + ['-c', s, '-o', o])

    def run(cmd):
        if verbose:
            print(' '.join(cmd), flush=True)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError('hipcc failed:\n%s\n%s' % (' '.join(cmd), r.stdout))
        if verbose and r.stdout.strip():
            print(r.stdout)

    if jobs:
        with ThreadPoolExecutor(max_workers=min(4, len(jobs))) as ex:
            list(ex.map(run, jobs))
    if jobs or force or _stale(LIB, objs):
        run([hipcc, '--offload-arch=' + ARCH, '-shared', '-fPIC', '-o', LIB] + objs + ['-lz'])     # zlib: kfn_png.hip
    return LIB


if __name__ == '__main__':
    print(build(force='--force' in sys.argv))
