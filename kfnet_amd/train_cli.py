"""The run path of the three training programs (SCoordNet.train, OFlowNet.train, KFNet.train; DESIGN.md 6b "Shared host
pieces"): the flags they share, declared once; the checks they share; the start of a run -- device, trainer, state, first
step, banner -- and the loop.  What is a program's own stays in its module: its further flags and refusals, its batches,
its epoch formula and its printed line."""
import time

HELP = dict(synthetic='train on this many seeded synthetic frames and labels',
            augment='brightness, contrast, rotation and zoom / shrink per batch',
            fp16='mixed precision: fp16 MFMA operands under dynamic loss scaling',
            depth='make the labels on the device from depth_list.txt and pose_list.txt')


def add_shared_flags(ap, stepvalue=None, **texts):
    """The reference's flags (KFNet/train.py:14-47), this project's --height .. --depth and the camera flags of `labels make`.
    stepvalue: the program's default of --stepvalue (None: it follows the scene); texts: help texts that replace those of HELP."""
    help = dict(HELP, **texts)
    ap.add_argument('--input_folder', default='')
    ap.add_argument('--model_folder', default='')
    ap.add_argument('--base_lr', type=float, default=1e-4)
    ap.add_argument('--max_steps', type=int, default=None)
    ap.add_argument('--display', type=int, default=10)
    ap.add_argument('--stepvalue', type=int, default=stepvalue)
    ap.add_argument('--snapshot', type=int, default=5000)
    ap.add_argument('--gamma', type=float, default=0.5)
    ap.add_argument('--weight_decay', type=float, default=1e-4)
    ap.add_argument('--shuffle', action='store_true')
    ap.add_argument('--reset_step', type=int, default=-1)
    ap.add_argument('--gpu', type=int, default=0)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--loss_clip', type=float, default=None)
    ap.add_argument('--synthetic', type=int, default=0, help=help['synthetic'])
    ap.add_argument('--augment', action='store_true', help=help['augment'])
    ap.add_argument('--fp16', action='store_true', help=help['fp16'])
    ap.add_argument('--depth', action='store_true', help=help['depth'])
    from .labels import add_camera_flags
    add_camera_flags(ap)


def check_flags(a, counts):
    """The message of the first shared check that fails, or None: --model_folder is given, and every flag of `counts` (the
    program's list, '--display' and '--snapshot' first) is at least 1."""
    if not a.model_folder:
        return '--model_folder is required: the snapshots go there'
    if any(getattr(a, name) < 1 for name in counts):
        flags = ['--' + name for name in counts]
        return '%s and %s must be >= 1' % (', '.join(flags[:-1]), flags[-1])
    return None


def check_size(a):
    """ValueError unless --height and --width are positive multiples of 8; the programs call it where they open their source."""
    from .staging import check_size
    check_size(a.height, a.width, '--height and --width')


def start(a, stepvalue, make_trainer, state, step, banner):
    """The first use of the device, behind the program's last refusal: picks --gpu, builds the trainer -- make_trainer(**kw)
    with the arguments every trainer takes -- loads the Adam state if there is one, sets the first step and prints the
    banner: the program's (label, value) lines and the current step between two rules.  Returns the trainer."""
    import torch
    torch.cuda.set_device(a.gpu)
    tr = make_trainer(image_size=(a.height, a.width), base_lr=a.base_lr, gamma=a.gamma, stepvalue=stepvalue,
                      weight_decay=a.weight_decay, loss_clip=a.loss_clip, device='cuda:%d' % a.gpu)
    if state is not None:
        tr.load_state(state)
    tr.global_step = step
    print('----------------------------------')
    for label, value in banner:
        print(label, value)
    print('current step: ', tr.global_step)
    print('----------------------------------')
    return tr


def loop(tr, max_steps, display, snapshot, model_folder, batch, line):
    """Steps until tr.global_step reaches max_steps.  batch(step) gives update number step's (indices, frames, labels, poses
    or None, keyword arguments of tr.step); line(stats, step, indices, duration) gives the text of a display step, every
    `display` steps and at the end -- only there are the stats read back.  A snapshot every `snapshot` steps and at the end."""
    import torch
    while tr.global_step < max_steps:
        t0 = time.time()
        indices, frames, labels, poses, kw = batch(tr.global_step)
        if poses is not None:
            tr.set_poses(poses)
        stats = tr.step(frames, labels, **kw)
        s = tr.global_step
        if s % display == 0 or s == max_steps:
            print(line(dict(stats), s, indices, time.time() - t0), flush=True)           # the read-back waits for the step
        if s % snapshot == 0 or s == max_steps:
            print('snapshot: %s, %s' % tr.save(model_folder, s), flush=True)
    torch.cuda.synchronize()
    return 0
