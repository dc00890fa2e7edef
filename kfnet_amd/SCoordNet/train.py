"""Stage 1 of the reference README's "Training": train SCoordNet on one scene.

    python -m kfnet_amd.SCoordNet.train --input_folder I --model_folder M --scene S

I holds image_list.txt, label_list.txt (one [H,W,4] float32 label per image: scene coordinates and mask) and transform.txt.
Snapshots go to M as kfnet_weights-<step>.npz (the ScoreNet/* variables: `python -m kfnet_amd.SCoordNet.eval --model_folder
M` reads it as it is) and kfnet_train_state-<step>.npz (Adam slots and counters).  A run resumes from the newest snapshot
in M -- a TF checkpoint or an .npz, with or without a state file -- and starts from an untrained graph's values otherwise.

The flags --base_lr --max_steps --display --stepvalue --snapshot --gamma --weight_decay --shuffle --reset_step --gpu are the
reference's (KFNet/train.py:14-47); stepvalue and max_steps = 5 * stepvalue follow the scene (set_stepvalue) unless given.
--loss_clip is off by default: the snapshot's clip at -2.0 (KFNet/KFNet.py:217) zeroes every gradient of an untrained
network; `--loss_clip -2` reproduces it.  `--synthetic N` trains on N seeded synthetic frames and labels.
`--augment` applies the reference's data_augmentation (KFNet/train.py:168-193) to every batch on the device, with the
parameters kfnet_amd.augment.draw(--augment_seed, step); the whole label files are then read, not only the
pixels the loss uses.
`--depth` needs no label files: I then holds image_list.txt, depth_list.txt, pose_list.txt and transform.txt (what `python -m
kfnet_amd.labels make --no_labels` writes), and every batch's labels are made on the device from its 16-bit depth maps and
poses -- at the pixels the loss reads, or at full resolution with --augment.  The camera flags are those of
`labels make`.
`--fp16` trains in mixed precision: conv1b .. conv7 on fp16 MFMA operands with fp32 accumulation, tensors and
master weights in fp32, under dynamic loss scaling that starts at --loss_scale (a power of two, default 32768).  The printed
line then ends with the scale and the number of steps skipped because of an overflow; `step` counts attempted steps.
`--reproj [W]` adds W times the reference's reprojection loss (KFNet.ReprojectionLoss, KFNet/KFNet.py:405-428; W = 50 when
the flag stands alone, as MeasureCoordLoss :246-248) to the loss.  It reads the poses that pose_list.txt of I
names (`labels make` writes it next to the label files) and the intrinsics of the camera flags; with --augment the pixel map
is augmented with the batch (KFNet/train.py:181-187).  The printed line then ends with `l_reproj`.
"""
import argparse
import sys
import time
from datetime import datetime

from .. import modes
from ..reproj import STAGE1_WEIGHT as REPROJ_WEIGHT

STEPVALUE = {'chess': 100000, 'fire': 30000, 'heads': 60000, 'office': 100000, 'pumpkin': 100000, 'redkitchen': 100000,
             'stairs': 100000}          # KFNet/train.py:330-344
FORMAT = ('[%s] epoch %d, step %d/%d, loss=%.3f, l_measure=%.3f, l_smooth=%.3f, a_measure=%.3f, #pixels=%d, lr = %.6f '
          '(%.3f sec/step)')


FORMAT_FP16 = ', loss_scale=%d, skipped=%d'
FORMAT_REPROJ = ', l_reproj=%.3f'


def format_line(now, epoch, step, max_steps, s, duration):
    """KFNet/train.py:427-432 reduced to the measurement fields; under --fp16 (s holds 'loss_scale') the scale and the
    skipped steps behind them; under --reproj (s holds 'l_reproj') the reprojection loss at the end."""
    line = FORMAT % (now, epoch, step, max_steps, s['loss'], s['l_measure'], s['l_smooth'], s['a_measure'], s['pixels'],
                     s['lr'], duration)
    if 'loss_scale' in s:
        line += FORMAT_FP16 % (s['loss_scale'], s['skipped'])
    if 'l_reproj' in s:
        line += FORMAT_REPROJ % s['l_reproj']
    return line


def schedule(scene, stepvalue=None, max_steps=None):
    """(stepvalue, max_steps): set_stepvalue's per-scene values, explicit flags winning."""
    sv = STEPVALUE[scene] if stepvalue is None else stepvalue
    return sv, (5 * sv if max_steps is None else max_steps)


def build_parser(reproj_flag=True):
    """reproj_flag = False leaves --reproj to the caller (KFNet.train's takes no number)."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--input_folder', default='')
    ap.add_argument('--model_folder', default='')
    ap.add_argument('--scene', default='')
    ap.add_argument('--base_lr', type=float, default=1e-4)
    ap.add_argument('--max_steps', type=int, default=None)
    ap.add_argument('--display', type=int, default=10)
    ap.add_argument('--stepvalue', type=int, default=None)
    ap.add_argument('--snapshot', type=int, default=5000)
    ap.add_argument('--gamma', type=float, default=0.5)
    ap.add_argument('--weight_decay', type=float, default=1e-4)
    ap.add_argument('--shuffle', action='store_true')
    ap.add_argument('--reset_step', type=int, default=-1)
    ap.add_argument('--gpu', type=int, default=0)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--loss_clip', type=float, default=None)
    ap.add_argument('--smooth_weight', type=float, default=50.0)
    ap.add_argument('--synthetic', type=int, default=0, help='train on this many seeded synthetic frames and labels')
    ap.add_argument('--augment', action='store_true', help='brightness, contrast, rotation and zoom / shrink per batch')
    ap.add_argument('--augment_seed', type=int, default=None, help='seed of the augmentation draws (default: --seed)')
    ap.add_argument('--depth', action='store_true', help='make the labels on the device from depth_list.txt and pose_list.txt')
    ap.add_argument('--fp16', action='store_true', help='mixed precision: fp16 MFMA operands under dynamic loss scaling')
    ap.add_argument('--loss_scale', type=int, default=None, help='initial loss scale of --fp16, a power of two (default 32768)')
    if reproj_flag:
        ap.add_argument('--reproj', type=float, nargs='?', const=REPROJ_WEIGHT, default=None, metavar='W',
                        help='add W (default 50) times the reprojection loss; needs pose_list.txt and the camera flags')
    from ..labels import add_camera_flags
    add_camera_flags(ap)
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.scene not in modes.SCENES:
        print('Invalid scene:', a.scene)
        return 1
    if not a.model_folder:
        print('--model_folder is required: the snapshots go there', file=sys.stderr)
        return 1
    if a.display < 1 or a.snapshot < 1 or a.batch < 1:
        print('--display, --snapshot and --batch must be >= 1', file=sys.stderr)
        return 1
    if a.loss_scale is not None and not a.fp16:
        print('--loss_scale belongs to --fp16', file=sys.stderr)
        return 1
    loss_scale = 2 ** 15 if a.loss_scale is None else a.loss_scale
    if loss_scale < 1 or loss_scale > 2 ** 24 or loss_scale & (loss_scale - 1):
        print('--loss_scale must be a power of two in 1 .. 2^24', file=sys.stderr)
        return 1
    if a.reproj is not None and not a.reproj >= 0.0:
        print('--reproj takes a weight >= 0', file=sys.stderr)
        return 1
    reproj = a.reproj or 0.0
    stepvalue, max_steps = schedule(a.scene, a.stepvalue, a.max_steps)
    from ..batches import open_source
    from ..staging import check_size
    from ..labels import camera_of
    from ..train import SCoordNetTrainer, batch_indices, restore
    try:
        check_size(a.height, a.width, '--height and --width')
        source = open_source(a, SCoordNetTrainer.needs_full_resolution(a.augment), needs_poses=reproj > 0.0)
        camera = camera_of(a) if reproj > 0.0 else None
    except (OSError, ValueError) as e:
        print(e, file=sys.stderr)
        return 1
    W, state, step = restore(a.model_folder)
    if W is None:
        from ..weights import initial_weights
        W = initial_weights(a.seed)
        print('no snapshot in %s: starting from untrained weights (seed %d)' % (a.model_folder, a.seed))
    import torch
    torch.cuda.set_device(a.gpu)
    tr = SCoordNetTrainer(W, image_size=(a.height, a.width), batch=a.batch, transform=source.transform, base_lr=a.base_lr,
                          gamma=a.gamma, stepvalue=stepvalue, weight_decay=a.weight_decay, loss_clip=a.loss_clip,
                          smooth_weight=a.smooth_weight, device='cuda:%d' % a.gpu, precision='fp16' if a.fp16 else 'fp32',
                          loss_scale=loss_scale, reproj_weight=reproj, camera=camera)
    if state is not None:
        tr.load_state(state)
    tr.global_step = step if a.reset_step < 0 else a.reset_step
    from ..augment import draw
    augment_seed = a.seed if a.augment_seed is None else a.augment_seed
    print('----------------------------------')
    print('scene: ', a.scene)
    print('training image number: ', source.count)
    print('batch size: ', a.batch)
    print('step value: ', stepvalue)
    print('max steps: ', max_steps)
    print('current step: ', tr.global_step)
    print('----------------------------------')
    while tr.global_step < max_steps:
        t0 = time.time()
        params = draw(augment_seed, tr.global_step) if a.augment else None
        indices = batch_indices(tr.global_step, a.batch, source.count, a.shuffle, a.seed)
        frames, labels = source.batch(indices, tr.needs_full_resolution(a.augment))
        if reproj > 0.0:
            tr.set_poses(source.poses[indices])
        stats = tr.step(frames, labels, augment=params)
        s = tr.global_step
        if s % a.display == 0 or s == max_steps:
            line = dict(stats)           # the read-back waits for the step
            print(format_line(datetime.now(), (s * a.batch) // source.count, s, max_steps, line, time.time() - t0), flush=True)
        if s % a.snapshot == 0 or s == max_steps:
            print('snapshot: %s, %s' % tr.save(a.model_folder, s), flush=True)
    torch.cuda.synchronize()
    return 0


if __name__ == '__main__':
    sys.exit(main())
