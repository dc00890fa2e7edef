"""Host side of mixed-precision training, no device: the loss-scale state machine's numpy restatement against
hand-written expectations, the layers' eligibility table, the command lines' flags and refusals, the printed line, and the
new exports."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import train_f16_ref as HR
import train_ref as R
from kfnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kfn_pack_conv_weights_f16', 'kfn_loss_scale_apply', 'kfn_loss_scale_unscale_check', 'kfn_adam_step_guarded')


# -- the state machine ---------------------------------------------------------------------------------------------------------
def _drive(ls, pattern):
    """Feeds the overflow flags of `pattern` ('x' = overflow, '.' = clean); returns the scale after every step."""
    out = []
    for c in pattern:
        ls.update(c == 'x')
        out.append(float(ls.scale))
    return out


def test_scale_halves_on_overflow_and_stops_at_one():
    ls = HR.LossScale(8.0, growth_interval=2000)
    assert _drive(ls, 'xxxxx') == [4.0, 2.0, 1.0, 1.0, 1.0]
    assert (ls.skipped, ls.adam_t, ls.good_steps) == (5, 0, 0)
    assert ls.beta1_power == 1.0 and ls.beta2_power == 1.0           # nothing was applied


def test_scale_doubles_after_the_interval_and_an_overflow_restarts_the_count():
    ls = HR.LossScale(1024.0, growth_interval=3)
    #                 1 2 3(x2) 4 5 x(/2) 7 8 9(x2) 10
    assert _drive(ls, '...' '..' 'x' '...' '.') == [1024, 1024, 2048, 2048, 2048, 1024, 1024, 1024, 2048, 2048]
    assert (ls.skipped, ls.adam_t, ls.good_steps) == (1, 9, 1)


def test_scale_is_capped_at_two_to_the_24():
    ls = HR.LossScale(2.0 ** 23, growth_interval=1)
    assert _drive(ls, '...') == [2.0 ** 24, 2.0 ** 24, 2.0 ** 24]
    assert (ls.skipped, ls.adam_t, ls.good_steps) == (0, 3, 0)


def test_bias_correction_follows_the_applied_steps_only():
    ls = HR.LossScale(2.0 ** 15, growth_interval=2000)
    _drive(ls, '.x.x.')
    assert ls.adam_t == 3 and ls.skipped == 2
    # products accumulated once per applied step, as TensorFlow's beta1_power / beta2_power variables
    assert ls.beta1_power == R.BETA1 * R.BETA1 * R.BETA1 and ls.beta2_power == (R.BETA2 * R.BETA2) * R.BETA2
    # the NEXT update is number 4
    assert abs(ls.lr_t(1e-4) / R.adam_lr_t(1e-4, 4) - 1.0) < 1e-14


def test_a_guarded_step_leaves_everything_alone_on_inf_and_nan():
    rng = np.random.default_rng(0)
    w = rng.normal(size=50).astype(np.float32)
    m, v = np.zeros(50, np.float32), np.zeros(50, np.float32)
    for poison in (np.inf, -np.inf, np.nan):
        ls = HR.LossScale(64.0)
        g = rng.normal(size=50).astype(np.float32) * np.float32(64.0)
        g[7] = poison
        w1, m1, v1 = ls.step(w, m, v, g, 1e-4, 1e-4)
        assert w1 is w and m1 is m and v1 is v
        assert (float(ls.scale), ls.skipped, ls.adam_t) == (32.0, 1, 0)
    ls = HR.LossScale(64.0)
    g = rng.normal(size=50).astype(np.float32)
    w1, m1, v1 = ls.step(w, m, v, g * np.float32(64.0), 1e-4, 1e-4)
    w2, m2, v2 = R.adam_step(w, m, v, g, 1e-4, 1, 1e-4)                  # the scale is a power of two: unscaling is exact
    assert float(R.ulp_distance(w1, w2).max()) <= 1.0 and np.array_equal(m1, m2) and float(R.ulp_distance(v1, v2).max()) <= 1.0
    assert (float(ls.scale), ls.skipped, ls.adam_t, ls.good_steps) == (64.0, 0, 1, 1)


def test_the_emulated_convolution_rounds_what_the_kernels_round():
    import torch
    x = torch.tensor([[[[1.0 + 2.0 ** -12]]]], dtype=torch.float64, requires_grad=True)       # rounds to 1 in fp16
    w = torch.tensor([[[[3.0 + 2.0 ** -11]]]], dtype=torch.float64, requires_grad=True)        # rounds to 3
    b = torch.tensor([0.5], dtype=torch.float64, requires_grad=True)
    y = HR.HalfConv.apply(x, w, b, 1, 4.0)
    assert y.item() == 3.5
    gx, gw, gb = torch.autograd.grad(y, [x, w, b], torch.tensor([[[[2.0 ** -26]]]], dtype=torch.float64))
    # 4 * 2^-26 = 2^-24 is the smallest fp16 subnormal: it survives; the products use the rounded operands
    assert gb.item() == 2.0 ** -26 and gx.item() == 3.0 * 2.0 ** -26 and gw.item() == 2.0 ** -26
    gx, gw, gb = torch.autograd.grad(HR.HalfConv.apply(x, w, b, 1, 1.0), [x, w, b], torch.tensor([[[[2.0 ** -26]]]], dtype=torch.float64))
    assert gb.item() == 0.0 and gx.item() == 0.0 and gw.item() == 0.0                          # without the scale it underflows


# -- the trainer's table ---------------------------------------------------------------------------------------------------------
def test_eligibility_table_of_the_layers():
    from kfnet_amd.train import LAYERS, f16_layer
    table = {name: f16_layer(k, ci, co) for name, k, ci, co, _, _ in LAYERS}
    assert [n for n, on in table.items() if not on] == ['conv1a', 'prediction']
    assert sum(table.values()) == 10
    assert tuple(n for n in table if not table[n]) == HR.FP32_LAYERS            # the emulation's own list
    assert not f16_layer(3, 48, 64) and not f16_layer(3, 64, 16) and f16_layer(1, 32, 32)


def test_trainer_refuses_bad_precision_arguments_before_any_device():
    from kfnet_amd.train import SCoordNetTrainer
    for kw in (dict(precision='bf16'), dict(precision='fp16', loss_scale=3), dict(precision='fp16', loss_scale=2 ** 25),
               dict(precision='fp16', loss_scale=0.5), dict(precision='fp16', growth_interval=0)):
        with pytest.raises(ValueError):
            SCoordNetTrainer({}, image_size=(64, 96), **kw)


def test_beta_powers_are_accumulated_products():
    from kfnet_amd.train import beta_powers
    assert beta_powers(0) == (1.0, 1.0)
    ls = HR.LossScale()
    _drive(ls, '.' * 7)
    assert beta_powers(7) == (float(ls.beta1_power), float(ls.beta2_power))


# -- command lines ----------------------------------------------------------------------------------------------------------------
def _cli(module, *args):
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    env['HIP_VISIBLE_DEVICES'] = env['CUDA_VISIBLE_DEVICES'] = ''        # a refusal must come before any device is needed
    return subprocess.run([sys.executable, '-m', module] + list(args), cwd=ROOT, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=120)


def test_parser_flags_and_the_printed_line():
    from kfnet_amd.SCoordNet.train import build_parser, format_line
    a = build_parser().parse_args([])
    assert a.fp16 is False and a.loss_scale is None
    a = build_parser().parse_args(['--fp16', '--loss_scale', '1024'])
    assert a.fp16 is True and a.loss_scale == 1024
    s = dict(loss=1.5, l_measure=1.25, l_smooth=0.005, a_measure=0.5, pixels=95.0, lr=1e-4)
    plain = ('[now] epoch 1, step 20/100, loss=1.500, l_measure=1.250, l_smooth=0.005, a_measure=0.500, #pixels=95, '
             'lr = 0.000100 (0.250 sec/step)')
    assert format_line('now', 1, 20, 100, s, 0.25) == plain
    assert format_line('now', 1, 20, 100, dict(s, loss_scale=32768.0, skipped=3), 0.25) == plain + ', loss_scale=32768, skipped=3'
    r = _cli('kfnet_amd.SCoordNet.train', '--help')
    assert r.returncode == 0 and '--fp16' in r.stdout and '--loss_scale' in r.stdout


def test_refusals_of_the_three_training_programs(tmp_path):
    m = str(tmp_path)
    cases = [
        ('kfnet_amd.SCoordNet.train', ['--scene', 'fire', '--model_folder', m, '--synthetic', '4', '--fp16', '--loss_scale', '1000'],
         'power of two'),
        ('kfnet_amd.SCoordNet.train', ['--scene', 'fire', '--model_folder', m, '--synthetic', '4', '--loss_scale', '1024'], '--fp16'),
        ('kfnet_amd.KFNet.train', ['--scene', 'fire', '--model_folder', m, '--synthetic', '8', '--fix_flownet', '--fp16'], '--fp16 is refused'),
        ('kfnet_amd.KFNet.train', ['--scene', 'fire', '--model_folder', m, '--synthetic', '8', '--joint', '--fp16'], '--fp16 is refused'),
        ('kfnet_amd.OFlowNet.train', ['--model_folder', m, '--synthetic', '8', '--fp16'], '--fp16 is refused'),
    ]
    for module, args, text in cases:
        r = _cli(module, *args)
        assert r.returncode == 1, (module, args, r.stderr[-500:])
        lines = [l for l in r.stderr.splitlines() if l.strip()]
        assert len(lines) == 1 and text in lines[0], (module, args, r.stderr[-500:])        # one line, no traceback
        assert r.stdout == '' and os.listdir(m) == []                                      # nothing started, nothing written


# -- exports --------------------------------------------------------------------------------------------------------------------
def test_new_exports_are_present_and_check_their_arguments_without_a_device():
    lib = _lib.load()
    assert lib.kfn_abi_version() == 13                                   # added exports: the number stays
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    header = open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()
    for name in NEW + ('kfn_loss_scale_state',):
        assert name in header
    assert C.sizeof(_lib.LossScaleState) == 40
    ARG = -1
    buf = np.zeros(64, np.float32).ctypes.data
    nb = C.c_size_t()

    def desc(**kw):
        d = dict(N=1, H=9, W=13, Cin=64, ldx=64, Cout=64, cout_pad=64, ldy=64, kh=3, kw=3, stride=1, operand_dtype=_lib.OPERAND_F16)
        d.update(kw)
        return _lib.ConvDesc(**d)
    d = desc()
    assert lib.kfn_conv2d_grad_weights_workspace_bytes(C.byref(d), C.byref(nb)) == 0 and nb.value == (9 * 64 + 1) * 64 * 4
    # 1040 pixels in two runs: of 544 (a multiple of 32) under fp16 operands, of 528 (of 16) under fp32 -- two planes each
    big = dict(N=1, H=26, W=40, Cin=512, ldx=512, Cout=512, cout_pad=512, ldy=512)
    d16, d32 = desc(**big), desc(operand_dtype=0, **big)
    n16, n32 = C.c_size_t(), C.c_size_t()
    assert lib.kfn_conv2d_grad_weights_workspace_bytes(C.byref(d16), C.byref(n16)) == 0
    assert lib.kfn_conv2d_grad_weights_workspace_bytes(C.byref(d32), C.byref(n32)) == 0
    assert n16.value == n32.value == 2 * (9 * 512 + 1) * 512 * 4
    for bad in (dict(Cin=48, ldx=48), dict(Cout=4, ldy=16), dict(Cout=48, ldy=48), dict(ldy=66), dict(operand_dtype=2),
                dict(x_dtype=1), dict(transposed=1, stride=2)):
        d = desc(**bad)
        assert lib.kfn_conv2d_grad_weights_workspace_bytes(C.byref(d), C.byref(nb)) == ARG, bad
        assert lib.kfn_conv2d_grad_weights(C.byref(d), buf, buf, buf, buf, buf, None) == ARG, bad
        assert b'kfn_conv2d_grad_weights' in lib.kfn_last_error()
    assert lib.kfn_pack_conv_weights_f16(buf, 3, 3, 0, 4, 0, buf, None) == ARG
    assert lib.kfn_pack_conv_weights_f16(buf, 3, 3, 64, 64, 7, buf, None) == ARG
    assert lib.kfn_pack_conv_weights_f16(None, 3, 3, 64, 64, 0, buf, None) == ARG
    assert lib.kfn_loss_scale_apply(buf, 0, buf, None) == ARG and lib.kfn_loss_scale_apply(buf, 8, None, None) == ARG
    assert lib.kfn_loss_scale_unscale_check(None, 8, buf, None) == ARG
    assert lib.kfn_adam_step_guarded(buf, buf, buf, buf, 8, 1e-4, 0.9, 0.999, 1e-8, 0.0, 0, buf, None) == ARG      # growth_interval
    assert lib.kfn_adam_step_guarded(buf, buf, buf, buf, 8, 1e-4, 1.0, 0.999, 1e-8, 0.0, 2000, buf, None) == ARG
    assert lib.kfn_adam_step_guarded(buf, buf, buf, buf, 8, 1e-4, 0.9, 0.999, 1e-8, 0.0, 2000, None, None) == ARG
