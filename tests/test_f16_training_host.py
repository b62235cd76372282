"""Why float16 training needs its own gradient checks, and the inputs those checks use (host only, float64 oracle).

The whole-net float16 tests (tests/test_gpu_f16.py: f16_net_step) compare parameter gradients that already hold the
regulariser's 2 * lambda * w at 1e-2 of each parameter's largest element.  With the analytic weights that term IS the
gradient of most parameters of the U-nets (test_l2_term_dominates_most_parameter_gradients pins the table), so a data
gradient wrong by a factor of 300 would pass.  tests/test_gpu_f16_training.py therefore judges the data gradient alone
(Net.data_grads) against a bound taken from Net.stored16, the oracle with every activation and activation gradient
stored once in binary16; this file pins the two oracle helpers to Net.loss_and_grads and checks that the inputs of the
GPU file stay judgeable: along the oracle's own SGD trajectory no parameter's binary16-storage deviation passes 1.25e-2.

This module also holds what the GPU file shares with it: the page cases, the judging constants and the deviation."""
import functools

import numpy as np

from oracle import nn_oracle as O

PAGE_NETS = ('Monochrome', 'Paragraph', 'Line')
TAGS = {'Monochrome': ('image', 'monochrome'), 'Paragraph': ('monochrome', 'paragraph'), 'Line': ('monochrome', 'line')}
PAGE = (2, 64, 128, 16)            # batch, height, width, char_width: the smallest page whose data gradients are not ~1e-9 of L2
TRAJECTORY_SEEDS = (1, 9)          # re-measure before changing: seeds 31, 5, 2, 8, 12, 41 reach 0.1 .. 0.8 on Line down_1/conv_1/b
LR = 0.05

# the judging rule for a float16 data gradient: err_p <= max(GRAD_FLOOR, STORE_FACTOR * dev_p)
GRAD_FLOOR = 1e-2                  # the project's whole-net gradient tolerance
STORE_FACTOR = 4                   # what stored16 leaves out: binary16 weight operands of the MFMA kernels, other rounding points
DEV_CAP = 1.25e-2                  # beyond it the bound would pass 5e-2: the parameter is unjudgeable at that step


def f32(a):
    """float64 -> float32 -> float64: what a float32 master weight holds"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def page_batch(seed):
    from univer_ocr_amd.my_model.synthetic import make_page_batch
    return make_page_batch(*PAGE, seed=seed)


def page_case(name, seed):
    """(X, y) of net `name` on the page batch of `seed`, as the host holds them (X not yet rounded to binary16)"""
    data = page_batch(seed)
    return data[TAGS[name][0]], data[TAGS[name][1]]


def analytic_net(name):
    """the oracle net with the analytic weights rounded to float32 (what Model.set_weights uploads)"""
    net = O.make_net(name)
    net.params = {pn: f32(v) for pn, v in net.params.items()}
    return net


def grad_scale_log2():
    from univer_ocr_amd.nn import ops
    return ops.f16_grad_scale_log2('seg', PAGE[1] * PAGE[2])


def l2_grads(net):
    """{param: (loss term, 2 * lambda * w)} of the regularised parameters"""
    return {pn: O.l2_reg(net.params[pn], lam) for pn, lam in net.regularised()}


def linf(a):
    return float(np.max(np.abs(a)))


def stored16_deviation(net, X16, y, grads, k):
    """{param: max|g16 - g| / max|g|}: how far honest binary16 storage moves each data gradient at these weights"""
    _, _, g16 = net.stored16(X16, y, k)
    return {pn: linf(g16[pn] - grads[pn]) / linf(grads[pn]) for pn in grads}


@functools.lru_cache(maxsize=None)
def _golden_case(name):
    from conftest import load_golden
    g = load_golden(f'my_model_{name.lower()}')
    return np.asarray(g['sgd/X'], np.float64), np.asarray(g['sgd/y'], np.float64)


ALL_NETS = PAGE_NETS + ('Char',)


def test_data_grads_plus_l2_is_loss_and_grads():
    """One copy of forward / loss / backward: data_grads + l2_reg of every regularised parameter == loss_and_grads,
    bit for bit, for the four nets (the Char net's dense layers are not regularised)."""
    for name in ALL_NETS:
        X, y = _golden_case(name)
        net = O.make_net(name)
        losses, pred, dx = net.loss_and_grads(X, y)
        total = net.grads
        pred2, loss2, data = net.data_grads(X, y)
        reg = l2_grads(net)
        assert sorted(data) == sorted(total) == sorted(net.params)
        assert np.array_equal(pred, pred2) and losses['output_losses'] == [loss2]
        assert np.array_equal(dx, net.input_grad)
        assert losses['regularization_loss'] == sum(reg[pn][0] for pn, _ in net.regularised())
        for pn in data:
            assert np.array_equal(total[pn], data[pn] + reg[pn][1] if pn in reg else data[pn]), pn
        assert len(reg) == (6 if name == 'Char' else len(net.params))


def test_stored16_with_identity_rounding_is_data_grads():
    for name in ALL_NETS:
        X, y = _golden_case(name)
        net = O.make_net(name)
        pred, loss, data = net.data_grads(X, y)
        pred2, loss2, same = net.stored16(X, y, 9, rnd=lambda a: a)
        assert np.array_equal(pred, pred2) and loss == loss2
        for pn in data:
            assert np.array_equal(data[pn], same[pn]), pn


def test_stored16_rounds_what_it_says():
    """binary16 on: the prediction is a binary16 tensor, the last layer's dw (a float64 sum over the rounded loss
    gradient and the rounded stored input) differs from the exact one by about 2^-11, not by 0 and not by much."""
    X, y = page_case('Paragraph', 1)
    net = analytic_net('Paragraph')
    X16 = O.round16(X)
    _, _, data = net.data_grads(X16, y)
    pred16, _, g16 = net.stored16(X16, y, 9)
    assert np.array_equal(pred16, O.round16(pred16))
    dev = linf(g16['Paragraph/end/conv_1/w'] - data['Paragraph/end/conv_1/w']) / linf(data['Paragraph/end/conv_1/w'])
    assert 0 < dev <= 4 * 2.0 ** -11


def test_l2_term_dominates_most_parameter_gradients():
    """The reason for tests/test_gpu_f16_training.py, at the inputs of test_page_net_step_f16_vs_oracle (seed 31,
    analytic weights): only 6 of the 24 parameters of the page nets have a data gradient as large as their L2 term, and
    the table pins seven of the others (max|data gradient| / max|data gradient + L2 gradient|, to 5 %): six lie below
    1e-2 of the total -- the old tolerance -- down to 3.2e-5 for Paragraph up_2/conv_block/conv_1/w."""
    ratio, data_led = {}, {}
    for name in PAGE_NETS:
        X, y = page_case(name, 31)
        net = analytic_net(name)
        _, _, data = net.data_grads(O.round16(X), y)
        reg = l2_grads(net)
        for pn in data:
            ratio[pn] = linf(data[pn]) / linf(data[pn] + reg[pn][1])
            data_led[pn] = linf(data[pn]) >= linf(reg[pn][1])
    assert len(ratio) == 24
    assert sum(data_led.values()) == 6 < len(ratio) / 2
    assert sorted(pn for pn, led in data_led.items() if led) == [
        'Line/end/conv_1/b', 'Line/end/conv_1/w', 'Monochrome/conv_2/w', 'Paragraph/down_1/conv_1/b',
        'Paragraph/end/conv_1/b', 'Paragraph/end/conv_1/w']
    table = {'Paragraph/up_2/conv_block/conv_1/w': 3.2e-5, 'Line/down_1/conv_1/b': 1.1e-4, 'Line/down_1/conv_1/w': 4.7e-4,
             'Paragraph/down_2/conv_1/w': 7.8e-4, 'Paragraph/down_1/conv_1/w': 1.1e-3, 'Line/down_2/conv_1/b': 3.9e-3,
             'Monochrome/conv_1/b': 6.0e-2}
    for pn, value in table.items():
        assert abs(ratio[pn] - value) <= 0.05 * value, (pn, ratio[pn])


def test_weight_operands_explain_the_line_net():
    """What stored16 leaves out, restated once on the CPU: the binary16-MFMA conv kernels (conv_h16*.hip) round the float32
    master weights to binary16 as matrix operands -- forward and backward-data of the 5x5 convs with 4 input channels,
    backward-data of the stride-2 1 -> 4 conv (tests/test_gpu_f16.py::test_conv_kernels_f16 lists them); dw / db use no
    weights.  Per-position storage roundings average out in a parameter gradient, a rounded weight shifts it coherently:
    Line up_2/conv_block/conv_1/b moves by 2.8e-3 where storage alone gives 1.3e-4 (MI355X: 3.1e-3 unfused), more than
    STORE_FACTOR times dev_p.  It is the GRAD_FLOOR that admits it; the bound of the rule admits every parameter."""
    name, k = 'Line', grad_scale_log2()
    X, y = page_case(name, 1)
    X16 = O.round16(X)
    net = analytic_net(name)
    _, _, data = net.data_grads(X16, y)
    dev = stored16_deviation(net, X16, y, data, k)

    def fwd(X, w, b, stride, padding, pad_value, bias):
        return O.conv2d_fwd(X, O.round16(w) if w.shape[2] == 4 else w, b, stride, padding, pad_value, bias)

    def bwd(X, w, g, stride, padding, pad_value, bias):
        rounded = w.shape[2] == 4 or (O._pair(stride) == (2, 2) and w.shape[3] == 4)
        dx, _, _ = O.conv2d_bwd(X, O.round16(w) if rounded else w, g, stride, padding, pad_value, bias)
        _, dw, db = O.conv2d_bwd(X, w, g, stride, padding, pad_value, bias)
        return dx, dw, db
    net._conv_fwd, net._conv_bwd = fwd, bwd
    moved = stored16_deviation(net, X16, y, data, k)
    for pn in data:
        assert moved[pn] <= max(GRAD_FLOOR, STORE_FACTOR * dev[pn]), (pn, moved[pn], dev[pn])
    pn = 'Line/up_2/conv_block/conv_1/b'
    assert STORE_FACTOR * dev[pn] < 2e-3 < moved[pn] < 4e-3, (moved[pn], dev[pn])


def test_trajectory_inputs_stay_judgeable():
    """The inputs of the GPU file, along the oracle's own trajectory: SGD (lr 0.05, momentum 0), six steps alternating
    the page batches of seeds 1 and 9, analytic weights re-rounded to float32 after every step, gradient scale 2^9.  The
    binary16-storage deviation of every parameter of every page net stays at or below DEV_CAP = 1.25e-2 (measured over
    eight steps: Monochrome 5.8e-3, Paragraph 4.2e-3, Line 7.2e-3), and at every step each net has a parameter whose
    data gradient is at least its L2 term, so a weight update checks the data path.  The deviation comes from the static
    gradient scale being sized for the loss gradient: by the first encoder layer the gradient is ~1e-9 per position, a
    binary16 subnormal even times 2^9 (other seeds reach 0.1 .. 0.8 on Line down_1/conv_1/b within a few steps)."""
    k = grad_scale_log2()
    assert k == 9
    for name in PAGE_NETS:
        net = analytic_net(name)
        worst = 0.0
        for step in range(6):
            X, y = page_case(name, TRAJECTORY_SEEDS[step % 2])
            X16 = O.round16(X)
            _, _, data = net.data_grads(X16, y)
            devs = stored16_deviation(net, X16, y, data, k)
            reg = l2_grads(net)
            worst = max(worst, max(devs.values()))
            assert max(devs.values()) <= DEV_CAP, (name, step, max(devs, key=devs.get), max(devs.values()))
            assert any(linf(data[pn]) >= linf(reg[pn][1]) for pn in data), (name, step)
            net.params = {pn: f32(w - LR * (data[pn] + reg[pn][1])) for pn, w in net.params.items()}
        print(f'{name}: worst stored16 deviation over six steps {worst:.2e}')
