"""Microbenchmark of the training step (DESIGN.md "Training"): ms per step of kfnet_amd.train.SCoordNetTrainer on synthetic
frames and labels, the split of a step over its phases, and per layer the weight-gradient launch beside the forward direct
launch as fractions of the fp32 MFMA peak.

    python tools/mb_train.py [--height 480 --width 640 --batch 4 --steps 10 --warmup 3] [--layers] [--augment] [--depth]
    python tools/mb_train.py --fp16 [--layers] [--rounds 5]
    python tools/mb_train.py --kfnet [--groups 1]
    python tools/mb_train.py --oflownet [--pairs 4]
    python tools/mb_train.py --joint [--groups 1]
    python tools/mb_train.py --reproj [--kfnet | --joint] [--rounds 5]

--augment times the step with the augmentation of DESIGN.md 6c on: full-resolution labels, the parameters of
kfnet_amd.augment.draw(0, step) in turn (its kernels are channel_sums_kernel and augment_kernel in a kernel trace).
--depth makes every step's labels on the device from synthetic depth maps and poses that stay there (stride 8,
or stride 1 with --augment; depth_labels_grid_kernel / depth_labels_full_kernel in a kernel trace).
--fp16 times the mixed-precision step beside the fp32 step in ONE process: two trainers on the same batch, timed
in alternating rounds (median and minimum of --rounds windows of --steps steps each), the phases of both, and with --layers
every layer's weight gradient, forward and input-gradient launch of both, as ms and TFLOP/s of the layer's nominal FLOPs.
--kfnet times kfnet_amd.train_kfnet.KFNetTrainer instead: ms per step on --groups groups of four frames, and
the launches it adds to stage 1's step -- the OFlowNet forward, the measurement map and the scan, the three-term loss, the
reverse scan -- each alone and as a share of the step.
--oflownet times kfnet_amd.train_flow.OFlowNetTrainer (stage 2): ms per step on --pairs pairs of frames, its
forward, loss + backward, Adam and packs, and the launches stage 2 adds, each alone: the cost volume's transpose with the bytes
that have to cross HBM (d_vol once, two feature maps) over its time as a share of 8 TB/s, the flow head's and the L2
normalisation's backward, and the loss.
--joint times the joint step of KFNetTrainer (train_flownet): ms per step with OFlowNet's backward pass on the
flow stream beside SCoordNet's and on one stream, the share of the launches the joint step adds to the fixed one (the reverse
scan's joint form beside the fixed form, the copies between the pair and the scan layout), and the OFlowNet backward alone.
--reproj times the step with the reprojection term beside the plain step in ONE process: two trainers on the
same batch in alternating rounds (median, minimum and maximum of --rounds windows), for stage 1, or with --kfnet / --joint
for stage 3 fixed / joint; then kfn_reproj_loss_grad (one and three outputs) and kfn_augment_pixel_map alone.

Under `rocprofv3 --kernel-trace --stats -- python tools/mb_train.py --steps 5` the kernel table gives the same split per
kernel name (wgrad_mfma_kernel, conv_mfma_kernel, ...)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FP32_MFMA = 157.3e12      # MI355X, v_mfma_f32_32x32x2_f32


def timed(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kfnet(a):
    import torch
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    from kfnet_amd.train import synthetic_labels
    from kfnet_amd.train_kfnet import GROUP, KFNetTrainer
    from kfnet_amd.weights import initial_weights, synthetic_weights
    W = initial_weights(0)
    W.update({k: v for k, v in synthetic_weights(1234).items() if k.startswith('Temporal/')})
    B = a.groups * GROUP
    tr = KFNetTrainer(W, image_size=(a.height, a.width), groups=a.groups, transform=synthetic_transform())
    frames = torch.from_numpy(synthetic_sequence(B, a.height, a.width)).cuda()
    labels = torch.from_numpy(synthetic_labels(B, tr.sc.grid)).cuda()
    for _ in range(a.warmup):
        tr.step(frames, labels)
    ms = timed(torch, lambda: tr.step(frames, labels), a.steps)
    print('%dx%d, %d group(s) of %d: %.2f ms per step (%.1f frames/s)' % (a.height, a.width, a.groups, GROUP, ms, 1e3 * B / ms))
    main = torch.cuda.current_stream()
    stride = tr.sc.stage(frames, labels, None, main.cuda_stream)

    def flow():
        tr.flow(main)
        main.wait_event(tr.ev_flow)
    tr.flow(main)
    parts = [('OFlowNet forward', flow), ('SCoordNet forward + measurement map + scan', tr.forward),
             ('SCoordNet forward', tr.sc.forward), ('three-term loss', lambda: tr.loss(stride)),
             ('reverse scan', tr.filter_backward), ('SCoordNet backward', tr.sc.backward)]
    t = {}
    for name, fn in parts:
        t[name] = timed(torch, fn, a.steps)
    scan = t['SCoordNet forward + measurement map + scan'] - t['SCoordNet forward']
    new = t['OFlowNet forward'] + scan + t['three-term loss'] + t['reverse scan']
    for name, v in (('OFlowNet forward (alone; in a step it overlaps SCoordNet\'s forward)', t['OFlowNet forward']),
                    ('measurement map + scan', scan), ('three-term loss', t['three-term loss']), ('reverse scan', t['reverse scan'])):
        print('%-72s %7.3f ms  %5.1f%% of the step' % (name, v, 100 * v / ms))
    print('the new launches together %.3f ms = %.1f%% of the step; SCoordNet forward %.2f ms, backward %.2f ms' %
          (new, 100 * new / ms, t['SCoordNet forward'], t['SCoordNet backward']))
    return 0


def joint(a):
    import torch
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    from kfnet_amd.train import synthetic_labels
    from kfnet_amd.train_kfnet import GROUP, KFNetTrainer
    from kfnet_amd.weights import initial_weights, synthetic_weights
    W = initial_weights(0)
    W.update({k: v for k, v in synthetic_weights(1234).items() if k.startswith('Temporal/')})
    B = a.groups * GROUP
    frames = torch.from_numpy(synthetic_sequence(B, a.height, a.width)).cuda()
    ms = {}
    for overlap in (True, False):
        tr = KFNetTrainer(W, image_size=(a.height, a.width), groups=a.groups, transform=synthetic_transform(), train_flownet=True,
                          overlap=overlap)
        labels = torch.from_numpy(synthetic_labels(B, tr.sc.grid)).cuda()
        for _ in range(a.warmup):
            tr.step(frames, labels)
        ms[overlap] = timed(torch, lambda: tr.step(frames, labels), a.steps)
        print('%dx%d, %d group(s) of %d, joint, OFlowNet backward %s: %.2f ms per step (%.1f frames/s)' % (
            a.height, a.width, a.groups, GROUP, 'on the flow stream' if overlap else 'on the main stream', ms[overlap],
            1e3 * B / ms[overlap]))
    step = ms[False]
    main = torch.cuda.current_stream()
    stride = tr.sc.stage(frames, labels, None, main.cuda_stream)
    tr.flow(main)
    tr.forward()
    tr.loss(stride)
    fixed = tr.lib.kfn_filter_backward
    c_flow = tr.c_flow.data_ptr()

    def fixed_scan():
        fixed(tr.back_desc, c_flow, tr.meas.data_ptr(), tr.temp.data_ptr(), tr.kf.data_ptr(), tr.d_temp.data_ptr(),
              tr.d_kf.data_ptr(), tr.sc.dact[-1].data_ptr(), tr.stats.data_ptr(), tr.back_scratch.data_ptr(), main.cuda_stream)

    def copies():
        S, T, ft = tr.S, tr.T, tr.ft
        tr.c_flow.view(S, T, -1, 2)[:, 1:].copy_(ft.flow.view(S, T - 1, -1, 2))
        tr.c_sigma.view(S, T, -1)[:, 1:].copy_(ft.sigma.view(S, T - 1, -1))
        ft.d_flow.view(S, T - 1, -1, 2).copy_(tr.d_flow.view(S, T, -1, 2)[:, 1:])
        ft.d_sigma.view(S, T - 1, -1).copy_(tr.d_sigma.view(S, T, -1)[:, 1:])
    parts = [('reverse scan, joint form', tr.filter_backward), ('reverse scan, fixed form', fixed_scan),
             ('copies between the pair and the scan layout', copies), ('OFlowNet forward, activations kept', tr.ft.forward),
             ('OFlowNet backward', lambda: tr.ft.backward()), ('OFlowNet Adam + packs', lambda: (tr.ft.apply_gradients(),
                                                                                                 tr.ft._repack(main.cuda_stream))),
             ('SCoordNet backward', tr.sc.backward)]
    t = {name: timed(torch, fn, a.steps) for name, fn in parts}
    for name, _ in parts:
        print('%-48s %7.3f ms  %5.1f%% of the one-stream step' % (name, t[name], 100 * t[name] / step))
    new = t['reverse scan, joint form'] - t['reverse scan, fixed form'] + t['copies between the pair and the scan layout']
    print('the new launches (the scan\'s extra work and the copies) %.3f ms = %.2f%% of the step; the flow stream hides %.2f ms' %
          (new, 100 * new / step, ms[False] - ms[True]))
    return 0


def oflownet(a):
    import ctypes as C
    import torch
    from kfnet_amd import _lib
    lib = _lib.load()
    P, h, w, Cc = a.pairs, a.height // 8, a.width // 8, 32
    N = P * h * w
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device='cuda').manual_seed(0)

    def rand(*shape):
        return torch.randn(*shape, device='cuda', generator=g)
    d_vol, d_f2, d_f1 = rand(N, 8, 8, Cc), torch.empty(N, Cc, device='cuda'), torch.empty(N, Cc, device='cuda')
    d_flow, prob = rand(N, 2), torch.softmax(rand(N, 64), -1)
    d_sigma, sigma = rand(N), 1e-2 * torch.exp(rand(N))
    d_logits, d_pre = torch.empty(N * 64, 16, device='cuda'), torch.empty(N, 16, device='cuda')
    x, gy, dx = rand(2 * N, Cc), rand(2 * N, Cc), torch.empty(2 * N, Cc, device='cuda')
    labels = rand(2 * P, h, w, 4)
    labels[..., 3] = (labels[..., 3] > -1.3).float()
    flow, stats = 2.0 * torch.rand(N, 2, device='cuda', generator=g) - 1.0, torch.zeros(16, device='cuda')
    desc = _lib.FlowLossDesc(P=P, h=h, w=w, label_stride=1, dist_threshold=0.05, min_uncertainty=1e-5)
    launches = [
        ('kfn_cost_volume_backward', lambda: lib.kfn_cost_volume_backward(d_vol.data_ptr(), d_f2.data_ptr(), d_f1.data_ptr(), P, h, w,
                                                                          Cc, stream)),
        ('kfn_flow_head_backward', lambda: lib.kfn_flow_head_backward(d_flow.data_ptr(), prob.data_ptr(), d_sigma.data_ptr(),
                                                                      sigma.data_ptr(), d_logits.data_ptr(), 16, d_pre.data_ptr(), 16,
                                                                      N, stream)),
        ('kfn_l2norm_backward', lambda: lib.kfn_l2norm_backward(x.data_ptr(), Cc, gy.data_ptr(), Cc, dx.data_ptr(), Cc, 2 * N, Cc,
                                                                stream)),
        ('kfn_flow_loss_grad', lambda: lib.kfn_flow_loss_grad(C.byref(desc), flow.data_ptr(), sigma.data_ptr(), labels.data_ptr(),
                                                              d_flow.data_ptr(), d_sigma.data_ptr(), stats.data_ptr(), stream)),
    ]
    print('%dx%d, %d pair(s): grid %dx%d, %d windows' % (a.height, a.width, P, h, w, N))
    from kfnet_amd.synth import synthetic_sequence
    from kfnet_amd.train import synthetic_labels
    from kfnet_amd.train_flow import OFlowNetTrainer
    from kfnet_amd.weights import synthetic_weights
    tr = OFlowNetTrainer(synthetic_weights(1234), image_size=(a.height, a.width), pairs=P)
    frames = torch.from_numpy(synthetic_sequence(2 * P, a.height, a.width)).cuda()
    labs = torch.from_numpy(synthetic_labels(2 * P, tr.grid)).cuda()
    for _ in range(a.warmup):
        tr.step(frames, labs)
    ms = timed(torch, lambda: tr.step(frames, labs), a.steps)
    tr.stage(frames, labs)
    parts = [('forward', tr.forward), ('loss + backward', lambda: (tr.loss(), tr.backward())),
             ('adam', lambda: tr.apply_gradients()), ('packs', lambda: tr._repack(stream))]
    print('%.2f ms per step (%.1f pairs/s), %.2f M parameters; %s' % (
        ms, 1e3 * P / ms, tr.num_floats / 1e6, ', '.join('%s %.2f ms' % (n, timed(torch, f, a.steps)) for n, f in parts)))
    for name, fn in launches:
        _lib.check(fn(), name)
        ms = timed(torch, fn, max(a.steps, 20))
        line = '%-26s %8.3f ms' % (name, ms)
        if name == 'kfn_cost_volume_backward':
            need = 4.0 * (d_vol.numel() + 2 * N * Cc)
            line += '   %.1f MB have to cross HBM: %.2f TB/s = %.1f%% of 8 TB/s (the launch reads d_vol twice)' % (
                need / 1e6, need / (ms * 1e-3) / 1e12, 100 * need / (ms * 1e-3) / 8e12)
        print(line)
    return 0


def fp16(a):
    """The fp32 and the fp16 step side by side, in alternating rounds."""
    import torch
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    from kfnet_amd.train import LAYERS, SCoordNetTrainer, synthetic_labels
    from kfnet_amd.weights import initial_weights
    size = (a.height, a.width)
    trs = {p: SCoordNetTrainer(initial_weights(0), image_size=size, batch=a.batch, transform=synthetic_transform(), precision=p)
           for p in ('fp32', 'fp16')}
    frames = torch.from_numpy(synthetic_sequence(a.batch, a.height, a.width)).cuda()
    labels = torch.from_numpy(synthetic_labels(a.batch, trs['fp32'].grid)).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def rounds(fns):
        """{name: (median, minimum)} of --rounds windows per function, the functions taking turns."""
        t = {n: [] for n in fns}
        for _ in range(a.rounds):
            for n, fn in fns.items():
                t[n].append(timed(torch, fn, a.steps))
        return {n: (float(np.median(v)), min(v)) for n, v in t.items()}
    for tr in trs.values():
        for _ in range(a.warmup):
            tr.step(frames, labels)
    ms = rounds({p: (lambda tr=tr: tr.step(frames, labels)) for p, tr in trs.items()})
    for p in trs:
        print('%dx%d batch %d, %s: %.2f ms per step (median of %d windows of %d steps; fastest %.2f), %.1f frames/s' %
              (a.height, a.width, a.batch, p, ms[p][0], a.rounds, a.steps, ms[p][1], 1e3 * a.batch / ms[p][0]))
    print('fp16 step / fp32 step = %.3f; loss scale state after the timed steps: %s' %
          (ms['fp16'][0] / ms['fp32'][0], trs['fp16'].loss_scale_state()))
    stride = {p: tr.stage(frames, labels) for p, tr in trs.items()}
    parts = {}
    for p, tr in trs.items():
        parts['forward ' + p] = tr.forward
        parts['loss + backward ' + p] = lambda tr=tr, p=p: tr.loss_and_gradients(stride[p])
        parts['packs ' + p] = lambda tr=tr: tr._repack(stream)
    t = rounds(parts)
    for p in trs:
        print('%s: forward %.2f ms, loss + backward %.2f ms, packs %.2f ms' %
              (p, t['forward ' + p][0], t['loss + backward ' + p][0], t['packs ' + p][0]))
    if not a.layers:
        return 0
    print('ms (median) and TFLOP/s of the nominal 2 P k k Cin Cout, fp32 | fp16; * = the layer stays on fp32 operands')
    print('%-11s %23s %7s | %23s %7s | %23s %7s' % ('layer', 'wgrad ms / TFLOP/s', 'x', 'forward ms / TFLOP/s', 'x',
                                                   'input grad ms / TFLOP/s', 'x'))
    tot = {}
    for li in range(1, len(LAYERS)):
        name, k, ci, co, s, relu = LAYERS[li]
        hin, win, ho, wo = trs['fp32'].shapes[li]
        nominal = 2.0 * a.batch * ho * wo * k * k * ci * co
        fns = {}
        for p, tr in trs.items():
            fns['w' + p] = lambda tr=tr: tr.weight_gradient(li, stream)
            fns['f' + p] = lambda tr=tr: tr.forward_layer(li, stream)
            fns['i' + p] = lambda tr=tr: tr.input_gradient(li, stream)       # with the ReLU gradient of the layer below
        t = rounds(fns)
        cols = []
        for kind in 'wfi':
            t32, t16 = t[kind + 'fp32'][0], t[kind + 'fp16'][0]
            tot[kind + 'fp32'] = tot.get(kind + 'fp32', 0.0) + t32
            tot[kind + 'fp16'] = tot.get(kind + 'fp16', 0.0) + t16
            cols.append('%6.3f/%6.1f %6.3f/%6.1f %6.2fx' % (t32, nominal / t32 / 1e9, t16, nominal / t16 / 1e9, t32 / t16))
        print('%-11s %s' % (name + ('' if trs['fp16'].f16[li] else '*'), ' | '.join(cols)))
    print('sums: weight gradients %.2f -> %.2f ms, forward %.2f -> %.2f ms, input gradients %.2f -> %.2f ms (conv1a apart)' %
          (tot['wfp32'], tot['wfp16'], tot['ffp32'], tot['ffp16'], tot['ifp32'], tot['ifp16']))
    return 0


def reproj(a):
    """The step with and without the reprojection term, in alternating rounds; then the two new launches alone."""
    import torch
    from kfnet_amd.augment import AugmentParams, Augmenter, ENLARGE
    from kfnet_amd.labels import DepthCamera
    from kfnet_amd.reproj import STAGE1_WEIGHT, STAGE3_WEIGHTS, ReprojTerm
    from kfnet_amd.synth import synthetic_poses, synthetic_sequence, synthetic_transform
    from kfnet_amd.train import SCoordNetTrainer, synthetic_labels
    from kfnet_amd.train_kfnet import GROUP, KFNetTrainer
    from kfnet_amd.weights import initial_weights, synthetic_weights
    size = (a.height, a.width)
    stage3 = a.kfnet or a.joint
    B = a.groups * GROUP if stage3 else a.batch
    W = initial_weights(0)
    if stage3:
        W.update({k: v for k, v in synthetic_weights(1234).items() if k.startswith('Temporal/')})
        trs = {on: KFNetTrainer(W, image_size=size, groups=a.groups, transform=synthetic_transform(), train_flownet=a.joint,
                                reproj_weights=STAGE3_WEIGHTS if on else None) for on in (False, True)}
        grid = trs[True].sc.grid
    else:
        trs = {on: SCoordNetTrainer(W, image_size=size, batch=B, transform=synthetic_transform(),
                                    reproj_weight=STAGE1_WEIGHT if on else 0.0) for on in (False, True)}
        grid = trs[True].grid
    frames = torch.from_numpy(synthetic_sequence(B, a.height, a.width)).cuda()
    labels = torch.from_numpy(synthetic_labels(B, grid)).cuda()
    poses = synthetic_poses(B)
    fns = {on: (lambda tr=tr: (tr.set_poses(poses), tr.step(frames, labels))) for on, tr in trs.items()}
    for fn in fns.values():
        for _ in range(a.warmup):
            fn()
    t = {on: [] for on in fns}
    for _ in range(a.rounds):
        for on, fn in fns.items():
            t[on].append(timed(torch, fn, a.steps))
    kind = 'stage 3 joint' if a.joint else 'stage 3 fixed' if a.kfnet else 'stage 1'
    for on in (False, True):
        print('%dx%d batch %d, %s, %s: %.2f ms per step (median of %d windows of %d steps; %.2f .. %.2f)' %
              (a.height, a.width, B, kind, 'with the term' if on else 'plain', float(np.median(t[on])), a.rounds, a.steps,
               min(t[on]), max(t[on])))
    print('the term costs %.3f ms per step (difference of the medians)' % (float(np.median(t[True])) - float(np.median(t[False]))))
    # the two launches alone
    h, w = grid
    stream = torch.cuda.current_stream().cuda_stream
    term = ReprojTerm(B, h, w, DepthCamera(), synthetic_transform())
    term.set_poses(poses)
    g = torch.Generator(device='cuda').manual_seed(0)
    xs = [torch.randn(B, h, w, 4, device='cuda', generator=g) for _ in range(3)]
    dxs = [torch.zeros(B, h, w, 16 if o == 0 else 4, device='cuda') for o in range(3)]
    nll = torch.zeros(16, device='cuda')
    nll[3] = float(labels[..., 3].sum().item()) + 1.0
    for n in (1, 3):
        outs = [(xs[o], dxs[o], 1.0) for o in range(n)]
        ms = timed(torch, lambda: term.launch(outs, labels, 1, None, nll, 3, stream), max(a.steps, 50))
        print('kfn_reproj_loss_grad, %d output(s), %d cells: %.4f ms' % (n, B * h * w, ms))
    aug = Augmenter(B, a.height, a.width)
    pm = torch.zeros(h, w, 2, device='cuda')
    params = AugmentParams(ENLARGE, angle=17.0, x1=0.05, y1=0.1, ratio=0.85)
    ms = timed(torch, lambda: aug.pixel_map(params, DepthCamera(), pm, stream), max(a.steps, 50))
    print('kfn_augment_pixel_map, %dx%d: %.4f ms' % (h, w, ms))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--layers', action='store_true', help='also time every layer\'s weight-gradient and forward launch')
    ap.add_argument('--augment', action='store_true', help='time the step with augmentation on')
    ap.add_argument('--depth', action='store_true', help='make the labels of every step from depth maps and poses')
    ap.add_argument('--kfnet', action='store_true', help='time the step of KFNetTrainer (SCoordNet through the filter)')
    ap.add_argument('--groups', type=int, default=1, help='--kfnet, --joint: groups of four frames per step')
    ap.add_argument('--joint', action='store_true', help='time the joint step of KFNetTrainer (both networks trained)')
    ap.add_argument('--oflownet', action='store_true', help='time the step of OFlowNetTrainer (stage 2) and the launches it adds')
    ap.add_argument('--pairs', type=int, default=4, help='--oflownet: pairs of frames per step')
    ap.add_argument('--fp16', action='store_true', help='time the mixed-precision step beside the fp32 step')
    ap.add_argument('--rounds', type=int, default=5, help='--fp16, --reproj: timing windows per variant, taken in turns')
    ap.add_argument('--reproj', action='store_true', help='time the step with the reprojection term beside the plain step')
    a = ap.parse_args(argv)
    if a.reproj:
        return reproj(a)
    if a.fp16:
        return fp16(a)
    if a.joint:
        return joint(a)
    if a.kfnet:
        return kfnet(a)
    if a.oflownet:
        return oflownet(a)
    import torch
    from kfnet_amd import _lib
    from kfnet_amd.synth import synthetic_sequence, synthetic_transform
    from kfnet_amd.train import LAYERS, SCoordNetTrainer, synthetic_labels
    from kfnet_amd.weights import initial_weights
    size = (a.height, a.width)
    tr = SCoordNetTrainer(initial_weights(0), image_size=size, batch=a.batch, transform=synthetic_transform())
    frames = torch.from_numpy(synthetic_sequence(a.batch, a.height, a.width)).cuda()
    labels = torch.from_numpy(synthetic_labels(a.batch, tr.label_shape(a.augment)[1:3])).cuda()
    if a.depth:
        from kfnet_amd.labels import DepthLabeler, pose_rows
        rng = np.random.default_rng(0)
        depth = torch.from_numpy(rng.integers(500, 4000, size=(a.batch,) + size).astype(np.uint16).view(np.int16)).cuda()
        poses = torch.from_numpy(pose_rows(np.tile(np.eye(4), (a.batch, 1, 1)))).cuda()
        labeler = DepthLabeler(a.batch, a.height, a.width, 1 if tr.needs_full_resolution(a.augment) else 8)

        def labels_of_step():
            return labeler.labels(depth, poses)
    else:
        def labels_of_step():
            return labels
    from kfnet_amd.augment import draw
    count = [0]

    def step():
        count[0] += 1
        tr.step(frames, labels_of_step(), augment=draw(0, count[0]) if a.augment else None)
    for _ in range(a.warmup):
        step()
    ms = timed(torch, step, a.steps)
    print('%dx%d batch %d%s: %.2f ms per step (%.1f frames/s), %.1f M parameters' %
          (a.height, a.width, a.batch, (', augmented' if a.augment else '') + (', labels from depth' if a.depth else ''), ms,
           1e3 * a.batch / ms, tr.num_floats / 1e6))
    stride = tr.stage(frames, labels)
    fwd = timed(torch, tr.forward, a.steps)
    bwd = timed(torch, lambda: tr.loss_and_gradients(stride), a.steps)
    lib = tr.lib
    stream = torch.cuda.current_stream().cuda_stream
    adam = timed(torch, lambda: _lib.check(lib.kfn_adam_step(tr.params.data_ptr(), tr.m.data_ptr(), tr.v.data_ptr(),
                                                             tr.grads.data_ptr(), tr.num_floats, 0.0, 0.9, 0.999, 1e-8, 0.0,
                                                             stream), 'adam'), a.steps)
    pack = timed(torch, lambda: tr._repack(stream), a.steps)
    print('forward %.2f ms, loss + backward %.2f ms, adam %.2f ms, packs %.2f ms' % (fwd, bwd, adam, pack))
    if not a.layers:
        return 0
    print('%-11s %10s %9s %7s | %10s %9s %7s' % ('layer', 'wgrad ms', 'TFLOP/s', 'peak', 'forward ms', 'TFLOP/s', 'peak'))
    tot_w = tot_f = 0.0
    for li in range(1, len(LAYERS)):
        name, k, ci, co, s, relu = LAYERS[li]
        hin, win, ho, wo = tr.shapes[li]
        P = a.batch * ho * wo
        # FLOPs the weight-gradient MFMAs execute: whole 128 x (64 | 128) tiles, the bias row included
        bn = 64 if co <= 64 else 128
        executed = 2.0 * P * (-(-(k * k * ci + 1) // 128) * 128) * (-(-co // bn) * bn)
        nominal = 2.0 * P * k * k * ci * co
        tw = timed(torch, lambda: tr.weight_gradient(li, stream), a.steps)
        tf = timed(torch, lambda: tr.forward_layer(li, stream), a.steps)
        tot_w += tw
        tot_f += tf
        print('%-11s %10.3f %9.1f %6.1f%% | %10.3f %9.1f %6.1f%%' %
              (name, tw, executed / tw / 1e9, 100 * executed / (tw * 1e-3) / PEAK_FP32_MFMA,
               tf, nominal / tf / 1e9, 100 * nominal / (tf * 1e-3) / PEAK_FP32_MFMA))
    print('weight gradients %.2f ms, forward convolutions %.2f ms (conv1a apart)' % (tot_w, tot_f))
    return 0


if __name__ == '__main__':
    sys.exit(main())
