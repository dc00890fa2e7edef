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
from datetime import datetime

from .. import modes, train_cli
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
    train_cli.add_shared_flags(ap)
    ap.add_argument('--scene', default='')
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--smooth_weight', type=float, default=50.0)
    ap.add_argument('--augment_seed', type=int, default=None, help='seed of the augmentation draws (default: --seed)')
    ap.add_argument('--loss_scale', type=int, default=None, help='initial loss scale of --fp16, a power of two (default 32768)')
    if reproj_flag:
        ap.add_argument('--reproj', type=float, nargs='?', const=REPROJ_WEIGHT, default=None, metavar='W',
                        help='add W (default 50) times the reprojection loss; needs pose_list.txt and the camera flags')
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.scene not in modes.SCENES:
        print('Invalid scene:', a.scene)
        return 1
    message = train_cli.check_flags(a, ('display', 'snapshot', 'batch'))
    if message:
        print(message, file=sys.stderr)
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
    from ..labels import camera_of
    from ..train import SCoordNetTrainer, batch_indices, restore
    try:
        train_cli.check_size(a)
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

    def make_trainer(**kw):
        return SCoordNetTrainer(W, batch=a.batch, transform=source.transform, smooth_weight=a.smooth_weight,
                                precision='fp16' if a.fp16 else 'fp32', loss_scale=loss_scale, reproj_weight=reproj,
                                camera=camera, **kw)
    tr = train_cli.start(a, stepvalue, make_trainer, state, step if a.reset_step < 0 else a.reset_step,
                         (('scene: ', a.scene), ('training image number: ', source.count), ('batch size: ', a.batch),
                          ('step value: ', stepvalue), ('max steps: ', max_steps)))
    from ..augment import draw
    augment_seed = a.seed if a.augment_seed is None else a.augment_seed

    def batch(step):
        params = draw(augment_seed, step) if a.augment else None
        indices = batch_indices(step, a.batch, source.count, a.shuffle, a.seed)
        frames, labels = source.batch(indices, tr.needs_full_resolution(a.augment))
        return indices, frames, labels, (source.poses[indices] if reproj > 0.0 else None), dict(augment=params)

    def line(stats, s, indices, duration):
        return format_line(datetime.now(), (s * a.batch) // source.count, s, max_steps, stats, duration)
    return train_cli.loop(tr, max_steps, a.display, a.snapshot, a.model_folder, batch, line)


if __name__ == '__main__':
    sys.exit(main())
