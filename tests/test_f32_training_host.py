"""Why the float32 trainer step is judged through the optimizer's velocity buffer, and the inputs of that check (host
only, float64 oracle).

The float32 oracle tests judge parameters AFTER a step (5e-5 of max|w|, or an update inequality with the float32 rounding
of w += v in it).  With the analytic weights that reading cannot see the data gradient of many parameters: the L2 term
2 * lambda * w is most of the update, and the rounding of the addition at |w| ~ 1 alone hides a gradient of 1e-6
(test_update_reading_is_blind pins the table).  The fused optimizer tail (opt_fused_one, csrc/elementwise.hip) computes
v = mu * v - lr * g_total in float32; with Momentum(momentum=0) and lr a power of two that is exactly -lr * g_total, so
after any step -- eager or replayed from a HIP graph, where the gradient buffer itself is already zero again --
g_read = -v / lr is the float32 total gradient the step used, at the gradient's own magnitude.  Subtracting the oracle's
2 * lambda * w leaves the data gradient; what the reading adds is the float32 rounding of the L2 product and of the sum,
    read_p = 3 * 2^-24 * (1 + max|l2_p| / max|g_data_p|)
relative to max|g_data_p|.  tests/test_gpu_f32_training.py judges every parameter of every net by
    max|g_read - (g_ref + l2_ref)| / max|g_ref| <= GRAD_TOL + read_p
and this file checks that its inputs keep read_p <= READ_CAP = 1e-2 along the oracle's own trajectory
(test_velocity_reading_sees_every_parameter), so every parameter is judged to better than 1 %.

This module also holds what the GPU file shares with it: the page cases, the judging constants and oracle_step."""
import functools
import hashlib

import numpy as np

from oracle import nn_oracle as O
from test_f16_training_host import analytic_net, f32, l2_grads, linf

PAGE = (2, 64, 128, 64)            # batch, height, width, char_width: at 64 the Char net takes its production route
SEEDS = (1, 9)                     # (windows + dense kernel, MFMA convs); the page part is that of the float16 file
LR = 2.0 ** -5                     # a power of two: -lr * g is exact in float32, -v / lr gives g back
ALL_NETS = ('Monochrome', 'Paragraph', 'Line', 'Char')
TAGS = {'Monochrome': ('image', 'monochrome'), 'Paragraph': ('monochrome', 'paragraph'), 'Line': ('monochrome', 'line'),
        'Char': ('char_lines', 'char_labels')}
GRAD_TOL = 2e-5                    # the project's float32 per-pass gradient tolerance (test_data_gradients_f32_f64)
READ_CAP = 1e-2                    # a condition on the inputs, not a tolerance: the oracle alone stays within it
STEPS = 6

ADAM_LR = 2.0 ** -16               # Adam legs of the GPU file (beta1 = 0): see test_adam_inputs_stay_near_the_analytic_weights
BETA2, EPS = float(np.float32(0.999)), float(np.float32(1e-8))      # as the fused tail holds them (float32)

UPDATE_TOL = 2e-5                 # the update-based reading of the existing tests, restated (test_update_reading_is_blind)
F32_TAIL = 4 * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def page_batch(seed):
    from univer_ocr_amd.my_model.synthetic import make_page_batch
    return make_page_batch(*PAGE, seed=seed)


def page_case(name, seed):
    """(X, y) of net `name` on the page batch of `seed`, rounded to float32 as the device holds them"""
    data = page_batch(seed)
    return f32(data[TAGS[name][0]]), f32(data[TAGS[name][1]])


def read_noise(g, l2):
    """read_p: what reading the data gradient of one parameter out of v = -lr * (g + l2) adds, relative to max|g|: the
    float32 roundings of 2 * w, of lambda * (2 w) and of the sum are each at most 2^-24 of max|g| + max|l2|"""
    return 3 * 2.0 ** -24 * (1 + linf(l2) / linf(g))


_ORACLE = {}


def oracle_step(name, seed, weights):
    """What the oracle says about one step of net `name` on the page batch of `seed` from float32 `weights`: prediction,
    loss, data gradients, L2 terms (zeros for a parameter without a regulariser), L2 loss and read_p.  Computed once
    per (net, batch, weights) and shared: the trainer legs reach the same weights whenever the GPU is deterministic."""
    key = (name, seed, hashlib.sha1(b''.join(np.ascontiguousarray(weights[pn]).tobytes() for pn in sorted(weights))).digest())
    if key not in _ORACLE:
        X, y = page_case(name, seed)
        net = O.make_net(name, {pn: np.array(w, dtype=np.float64) for pn, w in weights.items()})
        pred, loss, grads = net.data_grads(X, y)
        reg = l2_grads(net)
        l2 = {pn: reg[pn][1] if pn in reg else np.zeros_like(g) for pn, g in grads.items()}
        _ORACLE[key] = dict(pred=pred, loss=loss, grads=grads, l2=l2, l2_loss=sum(v[0] for v in reg.values()),
                            read={pn: read_noise(g, l2[pn]) for pn, g in grads.items()})
    return _ORACLE[key]


def sgd_trajectory(name):
    """[(step, seed, weights, oracle_step)] along the oracle's own SGD trajectory: STEPS steps from the analytic weights,
    batches of SEEDS alternating, weights rounded to float32 after every step (as the device holds them)"""
    weights = analytic_net(name).params
    out = []
    for step in range(STEPS):
        seed = SEEDS[step % 2]
        ref = oracle_step(name, seed, weights)
        out.append((step, seed, weights, ref))
        weights = {pn: f32(w - LR * (ref['grads'][pn] + ref['l2'][pn])) for pn, w in weights.items()}
    return out


def adam_trajectory(name, lr, steps=STEPS):
    """[(step, weights, oracle_step)] along the oracle's Adam trajectory as the GPU file runs it: beta1 = 0 (v = g_total),
    no bias correction, eps outside the root, state and weights rounded to float32 after every step"""
    weights = analytic_net(name).params
    acc = {pn: np.zeros_like(w) for pn, w in weights.items()}
    out = []
    for step in range(steps):
        ref = oracle_step(name, SEEDS[step % 2], weights)
        out.append((step, weights, ref))
        v = {pn: f32(ref['grads'][pn] + ref['l2'][pn]) for pn in weights}
        acc = {pn: f32(BETA2 * acc[pn] + (1 - BETA2) * v[pn] ** 2) for pn in weights}
        weights = {pn: f32(w - lr * v[pn] / (np.sqrt(acc[pn]) + EPS)) for pn, w in weights.items()}
    return out


def update_blindness(ref, weights):
    """{param: the smallest relative data-gradient error an update-based check can detect}: the allowance of
    |dw + lr (g + l2)| <= lr * 2e-5 * (max|g| + max|l2|) + 4 * 2^-24 * max|w| over lr * max|g_data|"""
    out = {}
    for pn, g in ref['grads'].items():
        allowance = LR * UPDATE_TOL * (linf(g) + linf(ref['l2'][pn])) + F32_TAIL * linf(weights[pn])
        out[pn] = allowance / (LR * linf(g))
    return out


def test_update_reading_is_blind():
    """Analytic float32 weights, both batches, all four nets: 66 parameter cases.  For at least 10 of them (13 measured) an
    update-based check cannot tell a data gradient of zero or of twice its value from the right one (detectable relative
    error >= 0.5); Char/conv_block/conv_1/b needs a factor above 5 (17 measured)."""
    figures = {}
    for name in ALL_NETS:
        weights = analytic_net(name).params
        for seed in SEEDS:
            for pn, value in update_blindness(oracle_step(name, seed, weights), weights).items():
                figures[pn, seed] = value
    assert len(figures) == 66
    print('smallest relative data-gradient error an update-based check detects (seed: value)')
    for pn in sorted({pn for pn, _ in figures}, key=lambda pn: -max(figures[pn, s] for s in SEEDS)):
        print(f'  {pn:42s} ' + '  '.join(f'{seed}: {figures[pn, seed]:9.2e}' for seed in SEEDS))
    blind = sum(value >= 0.5 for value in figures.values())
    print(f'{blind} of {len(figures)} at or above 0.5')
    assert blind >= 10
    assert max(figures['Char/conv_block/conv_1/b', seed] for seed in SEEDS) >= 5


def test_velocity_reading_sees_every_parameter():
    """Along the oracle's own six-step SGD trajectory read_p <= READ_CAP for every parameter of every net at every step
    (measured: Char conv_1/b 6.9e-3 at step 0, Line down_1/conv_1/b 2.2e-3, Paragraph up_2/conv_block/conv_1/w 9.5e-4,
    Monochrome conv_1/b 3.2e-6).  If a change of inputs breaks this, change the inputs, not the cap."""
    print('worst read_p per net along the trajectory')
    for name in ALL_NETS:
        worst = (0.0, None, None)
        for step, seed, weights, ref in sgd_trajectory(name):
            for pn, value in ref['read'].items():
                assert value <= READ_CAP, (pn, step, value)
                worst = max(worst, (value, pn, step))
        print(f'  {name:11s} {worst[1]:42s} step {worst[2]}  read_p {worst[0]:.2e}')


def test_some_data_gradient_is_tiny():
    """The inputs are of the kind the post-step readings cannot see: at every step of the trajectory some parameter of
    the four nets has max|g_data| < 1e-5 * max|w|."""
    tiny = {step: [] for step in range(STEPS)}
    for name in ALL_NETS:
        for step, seed, weights, ref in sgd_trajectory(name):
            tiny[step] += [pn for pn, g in ref['grads'].items() if linf(g) < 1e-5 * linf(weights[pn])]
    for step, found in tiny.items():
        assert found, step


def test_adam_inputs_stay_near_the_analytic_weights():
    """Adam without bias correction and with beta1 = 0 moves EVERY element by lr / sqrt(1 - beta2) = 31.6 lr in its first
    step, whatever its gradient.  At lr = 2^-10 that is 0.03 per element: the Char net's logits (0.085 at the analytic
    weights) reach 30 after one step and 1.4e4 after two, where the float64 softmax cross-entropy of the oracle itself
    is 0 * log 0.  At ADAM_LR = 2^-16 every net stays near the analytic weights for the six steps: the loss within 2 % of
    its first value for the same batch, the Char logits below 1, and read_p <= READ_CAP throughout."""
    with np.errstate(divide='ignore', invalid='ignore'):
        blown = adam_trajectory('Char', 2.0 ** -10, steps=3)
    assert linf(blown[0][2]['pred']) < 0.1 and linf(blown[2][2]['pred']) > 1e3
    for name in ALL_NETS:
        first = {}
        for step, weights, ref in adam_trajectory(name, ADAM_LR):
            start = first.setdefault(step % 2, ref['loss'])
            assert abs(ref['loss'] - start) <= 0.02 * start, (name, step, ref['loss'])
            assert max(ref['read'].values()) <= READ_CAP, (name, step)
            assert name != 'Char' or linf(ref['pred']) < 1
