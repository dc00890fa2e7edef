"""Stage 2 of the reference README's "Training": train OFlowNet (the Temporal scope) on pairs of consecutive frames.

    python -m kfnet_amd.OFlowNet.train --input_folder I --model_folder M [--pairs P] [--sequence_length L]

I holds image_list.txt and label_list.txt (one [H,W,4] float32 label per image: scene coordinates and mask), the lists of
several scenes concatenated if wished; transform.txt is neither needed nor read, the loss is invariant under it.  A step
trains P pairs (default 4): every [i, i + 1] followed by [i + 1, i], never across a range of --sequence_length frames (default
1000: the length of a 7-Scenes sequence; give 500 for lists of `stairs`).  Step s takes pairs s P .. s P + P - 1 of that
list, wrapping round, or a per-epoch permutation of it under --shuffle.

The loss is this project's definition (the reference's OFlowNet/train.py is absent): the likelihood of frame b's
ground-truth coordinates under frame a's, warped by the flow, with the process noise as uncertainty.  --loss_clip is off by
default.  Snapshots go to M as kfnet_weights-<step>.npz (the Temporal/* variables: `python -m kfnet_amd.OFlowNet.eval
--model_folder M` and `python -m kfnet_amd.KFNet.train --fix_flownet --oflownet M` read it as it is) and
kfnet_train_state-<step>.npz (Adam slots and counters).  A run resumes from the newest snapshot in M with its Adam slots and
starts from an untrained graph's values otherwise.

--base_lr --max_steps --display --stepvalue --snapshot --gamma --weight_decay --shuffle --reset_step --gpu --height --width
--seed are stage 1's; --stepvalue defaults to 100000 and --max_steps to 5 * stepvalue.  `--synthetic N` trains on N seeded
synthetic frames and labels; `--depth` makes the labels on the device from depth_list.txt and pose_list.txt (that
source does read transform.txt).  --augment is refused: a pair would need one draw for both frames, which is not built.
"""
import argparse
import sys
from datetime import datetime

from .. import train_cli

STEPVALUE = 100000
SEQUENCE_LENGTH = 1000
FORMAT = '[%s] epoch %d, step %d/%d, %5d~%5d, loss=%.3f, accuracy=%.3f, #pixels=%d, #lost=%d, lr = %.6f (%.3f sec/step)'


def format_line(now, epoch, step, max_steps, pair, s, duration):
    return FORMAT % (now, epoch, step, max_steps, pair[0], pair[1], s['loss'], s['accuracy'], s['pixels'], s['lost'], s['lr'], duration)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    train_cli.add_shared_flags(ap, STEPVALUE, augment='refused: not built for pairs',
                               fp16='refused: mixed precision is built for SCoordNet.train only')
    ap.add_argument('--pairs', type=int, default=4, help='pairs of frames per step')
    ap.add_argument('--sequence_length', type=int, default=SEQUENCE_LENGTH,
                    help='no pair reaches across a range of this many frames of the list (default 1000)')
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.augment:
        print('--augment is not built for OFlowNet.train: both frames of a pair would need one draw', file=sys.stderr)
        return 1
    if a.fp16:
        print('--fp16 is refused: mixed precision is built for stage 1 (SCoordNet.train) only', file=sys.stderr)
        return 1
    message = train_cli.check_flags(a, ('display', 'snapshot', 'pairs', 'stepvalue'))
    if message:
        print(message, file=sys.stderr)
        return 1
    stepvalue, max_steps = a.stepvalue, (5 * a.stepvalue if a.max_steps is None else a.max_steps)
    from ..batches import open_source
    from ..train_kfnet import group_indices, group_list
    a.batch = 2 * a.pairs                            # what a DepthSource sizes its labeler by
    try:
        train_cli.check_size(a)
        if a.sequence_length < 2:
            raise ValueError('--sequence_length must be at least 2')
        source = open_source(a, False, needs_transform=False)
        pairs = group_list(source.count, a.sequence_length, group=2)
        if not pairs:
            raise ValueError('%d frames hold no pair of consecutive frames' % source.count)
    except (OSError, ValueError) as e:
        print(e, file=sys.stderr)
        return 1
    from ..train import restore
    from ..train_flow import SCOPE, OFlowNetTrainer
    try:
        W, state, step = restore(a.model_folder, scope=SCOPE)
    except (OSError, ValueError) as e:
        print(e, file=sys.stderr)
        return 1
    if not W:
        from ..weights import initial_weights
        W, state = initial_weights(a.seed, scopes=(SCOPE,)), None
        print('no %s/* snapshot in %s: starting from untrained weights (seed %d)' % (SCOPE, a.model_folder, a.seed))
    tr = train_cli.start(a, stepvalue, lambda **kw: OFlowNetTrainer(W, pairs=a.pairs, **kw), state,
                         step if a.reset_step < 0 else a.reset_step,
                         (('training image number: ', source.count), ('pairs per step: ', a.pairs), ('step value: ', stepvalue),
                          ('max steps: ', max_steps)))

    def batch(step):
        indices = group_indices(step, a.pairs, pairs, a.shuffle, a.seed)
        frames, labels = source.batch(indices, False)
        return indices, frames, labels, None, {}

    def line(stats, s, indices, duration):
        return format_line(datetime.now(), (s * a.pairs) // len(pairs), s, max_steps, indices[:2], stats, duration)
    return train_cli.loop(tr, max_steps, a.display, a.snapshot, a.model_folder, batch, line)


if __name__ == '__main__':
    sys.exit(main())
