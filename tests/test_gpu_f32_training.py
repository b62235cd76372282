"""The float32 PageTrainer step -- what bench.py times by default -- against the float64 oracle, read through the
optimizer's velocity buffer.

The trainer tests compare the trainer with itself (graph against eager, pipelined against joined, grouped against separate)
and the whole-net oracle tests judge parameters after a step, where the L2 term and the float32 rounding of w += v hide the
data gradient of 13 of the 66 parameter cases used here (tests/test_f32_training_host.py pins the table).  This file reads
the gradient the step used out of the optimizer state instead.  The fused tail (opt_fused_one, csrc/elementwise.hip)
computes v = mu * v - lr * g_total in float32; with Momentum(momentum=0) and lr = 2^-5 that is -lr * g_total exactly, so
after any step, eager or replayed from a HIP graph, g_read = -v / lr is the float32 total gradient of that step.  The rule,
for every parameter of every net at every step:
    err_p = max|g_read - (g_ref + l2_ref)| / max|g_ref| <= GRAD_TOL + read_p
g_ref = Net.data_grads of the oracle at the GPU's own pre-step weights and the float32 inputs, l2_ref = 2 * lambda * w in
float64, GRAD_TOL = 2e-5 the project's float32 per-pass gradient tolerance, read_p = 3 * 2^-24 * (1 + max|l2| / max|g_ref|)
the float32 roundings of the L2 product and sum (at most 6.9e-3 along the oracle's trajectory, asserted <= 1e-2 here too).
Before every step the oracle is set to the GPU's weights, so every bound is a single-step bound.  Had a parameter missed
the bound by float32 summation order alone, its bound would have become max(GRAD_TOL, 4 x the deviation of a float32-
accumulated NumPy evaluation of that layer's dw) + read_p -- the factor 4 of the float16 rule; none did.

With Adam and beta1 = 0 the tail stores v = g_total exactly, so the same rule applies with g_read = v; the rest of the tail
is judged elementwise in float64 from the GPU's own v and a, with the hyper-parameters as the kernel holds them (float32 of
0.999 and of 1e-8: 1 - float32(0.999) differs from 0.001 by 1.3e-5):
    |a_after - (b2 a_before + (1 - b2) v^2)| <= 4 * 2^-24 * that + 2^-126       (square, two products, sum)
    |(w_before - w_after) - lr v / (sqrt(a_after) + eps)| <= 8 * 2^-24 * |that| + 2^-24 * |w_before|
                                                                 (square root, sum, divide, multiply; the subtraction)
Both factors are choices that cover the float32 operations named; 2^-126 is the smallest normal float32.

The Adam legs use lr = 2^-16, not the 2^-10 first planned: without bias correction and with beta1 = 0 the first Adam step
moves every element by 31.6 lr whatever its gradient, and at 2^-10 the Char net's logits reach 1.4e4 after two steps, where
the oracle's own float64 cross-entropy is 0 * log 0 (tests/test_f32_training_host.py pins both); every bound is relative to
the step, so a smaller lr checks no less.

All cases use 2 x 64 x 128 pages and 2 x 32 x 64 strips (char_width 64: the Char net's windows + dense kernel and MFMA
convs) of seeds 1 and 9, analytic weights.

Measured on MI355X (pytest -s; the whole file runs in 4.3 s: 1.7 s of set-up, its longest case 0.6 s, the first, which fills
the oracle cache; the other SGD legs reach bit-identical weights and take 0.12 s each):
    largest err_p (largest err_p / (GRAD_TOL + read_p)), the same in all six SGD legs:
        Monochrome 1.50e-6 (0.06),  Paragraph 2.83e-4 (0.44),  Line 8.01e-4 (0.44),  Char 3.64e-3 (0.56);
    the two Adam legs, equal to each other: Monochrome 1.47e-6 (0.06), Paragraph 4.57e-4 (0.36), Line 9.09e-4 (0.49),
        Char 3.64e-3 (0.56); a error / allowance 0.43 / 0.36 / 0.43 / 0.50, weight-step error / allowance 0.98 / 0.95 / 0.96 /
        1.00 (the float32 rounding of w - step alone reaches 2^-24 |w| just above a power of two);
    no parameter needed the summation-order bound.
    test_checker_sees_a_doubled_weight_gradient: old criterion / velocity rule err_p
        Char conv_1/w 1.11e-7 / 1.000, conv_1/b 3.44e-8 / 1.000;  Paragraph up_2 conv_1/w 1.17e-7 / 1.000, /b 4.42e-5 / 1.000.
    Before uocr_finish_defer ordered two finishes for one dw (csrc/finish_group.hip) this test read err_p 1.000 / 0.004 for
    the Char pair and 0.000 for Paragraph up_2 conv_1/w: both finishes of the deferred group ran in one launch, unordered,
    and one sum was lost.  A net's backward pass writes every dw once, so no step of the trainer was affected.
"""
import numpy as np
import pytest

from conftest import rel_linf
from test_f16_training_host import analytic_net, linf
from test_f32_training_host import (ADAM_LR, ALL_NETS, BETA2, EPS, GRAD_TOL, LR, PAGE, READ_CAP, SEEDS, STEPS, oracle_step,
                                     page_batch)

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-5            # loss and published prediction of a whole net in float32
TOL_L2 = 2e-5             # the regularisation loss
TOL_OLD = 5e-5            # the old criterion: post-step parameters, relative to max|w|
ULP = 2.0 ** -24


@pytest.fixture
def f32_lazy():
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    lazy = CP.lazy_losses
    CP.set_dtype('float32')
    yield CP
    CP.set_dtype('float32')
    CP.lazy_losses = lazy


def nest(flat):
    out = {}
    for key, value in flat.items():
        layer, pname = key.rsplit('/', 1)
        out.setdefault(layer, {})[pname] = value.tolist()
    return out


def page_trainer(optimizer, graphs, pipelined, lr=LR, **extra):
    from univer_ocr_amd.my_model.trainer import PageTrainer
    from univer_ocr_amd.nn import CP
    CP.lazy_losses = True
    trainer = PageTrainer(*PAGE, optimizer=optimizer, lr=lr, seed=3, graphs=graphs, pipelined=pipelined, **extra)
    assert tuple(trainer.models) == ALL_NETS and trainer.lanes is not None
    assert trainer.graphs == graphs and trainer.pipelined == pipelined
    for name, model in trainer.models.items():
        model.set_weights(nest(analytic_net(name).params))
    return trainer


def _per_param(trainer, read):
    return {name: {pn: read(p) for pn, p in model.params().items()} for name, model in trainer.models.items()}


def weights(trainer):
    """{net: {param: float64 array}} of the float32 weights; read only after trainer.join()"""
    return _per_param(trainer, lambda p: p.value.numpy().astype(np.float64))


def _state(trainer, which):
    def read(p):
        state = trainer.optimizer.groups[id(p)][1]
        if state is None:                              # before the first step: the initial value
            return np.zeros(p.value.shape, np.float64)
        array = getattr(state, which).numpy()
        assert array.dtype == np.float32 and array.shape == p.value.shape
        return array.astype(np.float64)
    return _per_param(trainer, read)


def velocities(trainer):
    """{net: {param: float64 array}} of the optimizer's float32 velocity (views into the flat state buffer of the net's
    pack); read only after trainer.join()"""
    return _state(trainer, 'velocity')


def accumulated(trainer):
    return _state(trainer, 'accumulated')


def f32_sum(a, b):
    """one float32 addition of float32 values held in float64 arrays"""
    return a.astype(np.float32) + b.astype(np.float32)


def gradient_errors(ref, g_read):
    """{param: (err_p, bound_p)} of the rule of the module docstring"""
    out = {}
    for pn, g in ref['grads'].items():
        err = linf(g_read[pn] - (g + ref['l2'][pn])) / linf(g)
        out[pn] = (err, GRAD_TOL + ref['read'][pn])
    return out


def check_outputs(CP, trainer, context, losses, name, ref, what):
    """loss, published prediction, regularisation loss and the fusions of the production route"""
    model = trainer.models[name]
    assert len(model._wins_used) == (name == 'Char') and len(model._ups_used) == 2 * (name in ('Paragraph', 'Line')), what
    loss = float(losses[name]['output_losses'][0])
    assert abs(loss - ref['loss']) <= TOL_OUT * abs(ref['loss']), (what, loss, ref['loss'])
    pred = CP.asnumpy(context[f'{name.lower()}_pred'])
    assert pred.dtype == np.float32 and rel_linf(pred, ref['pred']) <= TOL_OUT, what
    reg = float(losses[name]['regularization_loss'])
    assert abs(reg - ref['l2_loss']) <= TOL_L2 * ref['l2_loss'], (what, reg, ref['l2_loss'])


def check_gradients(ref, g_read, what, worst):
    failed = []
    for pn, (err, bound) in sorted(gradient_errors(ref, g_read).items()):
        print(f'  {what} {pn}: err_p {err:.2e} read_p {ref["read"][pn]:.2e}')
        assert ref['read'][pn] <= READ_CAP, (what, pn, ref['read'][pn])
        worst['err'], worst['ratio'] = max(worst['err'], err), max(worst['ratio'], err / bound)
        if not err <= bound:
            failed.append(f'{what} {pn}: err_p {err:.3e} > {bound:.3e} (read_p {ref["read"][pn]:.2e})')
    return failed


def gradient_buffer_is_zero(model):
    return not np.any(model.pack._grad.numpy())


LEGS = [pytest.param(False, False, {}, id='eager-joined'),
        pytest.param(False, True, {}, id='eager-pipelined'),
        pytest.param(True, False, {}, id='graphs-joined'),
        pytest.param(True, True, {}, id='graphs-pipelined'),
        pytest.param(False, False, {'group_wgrad': ()}, id='eager-ungrouped'),
        pytest.param(False, False, {'group_wgrad': (), 'side_wgrad': ('Char',)}, id='eager-ungrouped-side')]


@pytest.mark.parametrize('graphs, pipelined, extra', LEGS)
def test_trainer_steps_f32_vs_oracle(graphs, pipelined, extra, f32_lazy):
    """The step bench.py times by default (PageTrainer in float32, SGD, four nets on lanes, weight gradients from the
    deferred groups, fused optimizer tail), six steps alternating two batches: steps 0 and 1 eager, step 2 captures,
    3 to 5 replay.  Per net and step: loss, published prediction and regularisation loss; every parameter's gradient
    by the velocity rule; w_after == float32(w_before + v) bit for bit (one float32 addition of stored values); the
    gradient buffer zero after the step.  Legs 5 and 6 take the weight gradients from separate launches, and the Char
    net's from the side stream."""
    CP = f32_lazy
    trainer = page_trainer('sgd', graphs, pipelined, **extra)
    for name, model in trainer.models.items():
        assert model.group_wgrad == ('group_wgrad' not in extra)
        assert model.side_wgrad == (name in extra.get('side_wgrad', ()))
    worst = {name: dict(err=0.0, ratio=0.0) for name in ALL_NETS}
    failed = []
    for step in range(STEPS):
        seed = SEEDS[step % 2]
        trainer.join()
        before = weights(trainer)
        context = trainer.make_context(page_batch(seed))
        losses = trainer.step(context)
        trainer.join()
        after, v = weights(trainer), velocities(trainer)
        assert (trainer._captured is not None) == (graphs and step >= 2)
        for name in ALL_NETS:
            what = f'{name} step {step}'
            ref = oracle_step(name, seed, before[name])
            check_outputs(CP, trainer, context, losses, name, ref, what)
            failed += check_gradients(ref, {pn: -a / LR for pn, a in v[name].items()}, what, worst[name])
            for pn, w in before[name].items():
                assert np.array_equal(after[name][pn].astype(np.float32), f32_sum(w, v[name][pn])), (what, pn)
            assert gradient_buffer_is_zero(trainer.models[name]), what
    assert (trainer._captured is not None) == graphs
    print(f'graphs={graphs} pipelined={pipelined} {extra}: largest err_p, largest err_p / bound_p: '
          + ', '.join(f'{name} {w["err"]:.2e} {w["ratio"]:.2f}' for name, w in worst.items()))
    assert not failed, failed


@pytest.mark.parametrize('graphs, pipelined', [pytest.param(False, False, id='eager'),
                                               pytest.param(True, True, id='graphs-pipelined')])
def test_trainer_steps_adam_f32_vs_oracle(graphs, pipelined, f32_lazy):
    """The same six steps with Adam (lr 2^-16: the module docstring) and beta1 = 0, set before the first step: v = g_total
    exactly, judged by the velocity rule; a and the weight step elementwise from the GPU's own v and a by the two
    inequalities of the module docstring."""
    CP = f32_lazy
    trainer = page_trainer('adam', graphs, pipelined, lr=ADAM_LR)
    trainer.optimizer.beta1 = 0.0
    assert float(np.float32(trainer.optimizer.beta2)) == BETA2 and trainer.optimizer.lr == ADAM_LR
    worst = {name: dict(err=0.0, ratio=0.0, a=0.0, w=0.0, read=0.0) for name in ALL_NETS}
    failed = []
    for step in range(STEPS):
        seed = SEEDS[step % 2]
        trainer.join()
        before, a_before = weights(trainer), accumulated(trainer)
        context = trainer.make_context(page_batch(seed))
        losses = trainer.step(context)
        trainer.join()
        after, v, a_after = weights(trainer), velocities(trainer), accumulated(trainer)
        for name in ALL_NETS:
            what = f'{name} step {step}'
            ref = oracle_step(name, seed, before[name])
            check_outputs(CP, trainer, context, losses, name, ref, what)
            for pn, (err, bound) in sorted(gradient_errors(ref, v[name]).items()):
                print(f'  {what} {pn}: err_p {err:.2e} read_p {ref["read"][pn]:.2e}')
                w = worst[name]
                w['err'], w['ratio'], w['read'] = max(w['err'], err), max(w['ratio'], err / bound), max(w['read'], ref['read'][pn])
                if not err <= bound:
                    failed.append(f'{what} {pn}: err_p {err:.3e} > {bound:.3e} (read_p {ref["read"][pn]:.2e})')
            for pn in before[name]:
                vp, a0, a1 = (x[name][pn] for x in (v, a_before, a_after))
                w0, w1 = (x[name][pn] for x in (before, after))
                a_ref = BETA2 * a0 + (1 - BETA2) * vp * vp
                a_err = np.abs(a1 - a_ref) / (4 * ULP * a_ref + 2.0 ** -126)
                step_ref = ADAM_LR * vp / (np.sqrt(a1) + EPS)
                w_err = np.abs((w0 - w1) - step_ref) / (8 * ULP * np.abs(step_ref) + ULP * np.abs(w0) + 2.0 ** -126)
                worst[name]['a'], worst[name]['w'] = max(worst[name]['a'], a_err.max()), max(worst[name]['w'], w_err.max())
                assert a_err.max() <= 1, (what, pn, a_err.max())
                assert w_err.max() <= 1, (what, pn, w_err.max())
            assert gradient_buffer_is_zero(trainer.models[name]), what
    assert (trainer._captured is not None) == graphs
    print(f'adam graphs={graphs} pipelined={pipelined}: largest err_p, err_p / bound_p, read_p, a error / allowance, '
          'weight-step error / allowance: '
          + ', '.join(f'{name} {w["err"]:.2e} {w["ratio"]:.2f} {w["read"]:.1e} {w["a"]:.2f} {w["w"]:.2f}' for name, w in worst.items()))
    assert not failed, failed


@pytest.mark.parametrize('net_name, layer_name, op_name', [
    ('Char', 'Char/conv_block/conv_1', 'conv2d_bwd_weight'),
    ('Paragraph', 'Paragraph/up_2/conv_block/conv_1', 'upconv2x_bwd_weight')])
def test_checker_sees_a_doubled_weight_gradient(net_name, layer_name, op_name, f32_lazy, monkeypatch):
    """The velocity rule bites where the post-step reading does not.  In one eager SGD step from the analytic weights the
    weight-gradient call of one layer is issued twice (accumulate=True both times: two legal launches into a zeroed
    buffer), which doubles that layer's dw and db -- inside the net's deferred weight-gradient group, which has to order
    the two finishes it records for one dw.  The old criterion -- post-step parameters within 5e-5 of max|w| of
    the oracle's -- still accepts both parameters; the velocity rule rejects both with err_p ~ 1 and accepts every other
    parameter of every net."""
    from univer_ocr_amd.nn import ops
    trainer = page_trainer('sgd', False, False)
    layer, seen = trainer.models[net_name].layers[layer_name], []
    original = getattr(ops, op_name)

    def twice(x, dy, dw, *args, **kwargs):
        if dw.ptr == layer.w._grad.ptr:
            assert kwargs['accumulate'] is True
            seen.append(op_name)
            original(x, dy, dw, *args, **kwargs)
        return original(x, dy, dw, *args, **kwargs)
    trainer.join()
    before = weights(trainer)
    context = trainer.make_context(page_batch(SEEDS[0]))
    with monkeypatch.context() as patch:
        patch.setattr(ops, op_name, twice)
        trainer.step(context)
        trainer.join()
    assert seen == [op_name]
    after, v = weights(trainer), velocities(trainer)
    doubled = {layer_name + '/w', layer_name + '/b'}
    for name in ALL_NETS:
        ref = oracle_step(name, SEEDS[0], before[name])
        errors = gradient_errors(ref, {pn: -a / LR for pn, a in v[name].items()})
        for pn, (err, bound) in errors.items():
            if pn not in doubled:
                assert err <= bound, (pn, err, bound)
                continue
            w_ref = before[name][pn] - LR * (ref['grads'][pn] + ref['l2'][pn])
            old_err = rel_linf(after[name][pn], w_ref)
            print(f'{pn} doubled: old criterion {old_err:.2e} (accepts at {TOL_OLD:.0e}), velocity rule err_p {err:.3f} > {bound:.2e}')
            assert old_err <= TOL_OLD, 'the old criterion was expected to accept the doubled data gradient'
            assert 0.9 <= err <= 1.1 and err > bound
        assert doubled <= set(errors) or name != net_name
