"""float16 training judged on its DATA gradients, and the float16 step the benchmark times against the oracle.

tests/test_gpu_f16.py compares whole-net parameter gradients that already hold the regulariser's 2 * lambda * w, which for
most parameters of the U-nets is the gradient (tests/test_f16_training_host.py pins the table).  Here Model.train_begin is
read before train_finish adds the L2 term, so every parameter gradient is the data gradient alone.

The judging rule, used by every float16 case:
    err_p = max|g_gpu - g_ref| / max|g_ref| <= max(1e-2, 4 * dev_p)
g_ref = Net.data_grads of the float64 oracle on the binary16-rounded inputs with the GPU's float32 weights; dev_p = the same
measure for Net.stored16 (every activation and activation gradient stored once in binary16) at those weights and inputs,
computed here on the CPU, never from the GPU's output.  1e-2 is the project's whole-net gradient tolerance; the factor 4
covers what stored16 leaves out (binary16 weight operands of the MFMA kernels, rounding points that differ in the fused
kernels) and is a choice, not a measurement.  A parameter with dev_p > 1.25e-2 (a bound past 5e-2) is unjudgeable at that
step: checked for being finite only, printed, at most one per net and step and none at step 0.

A weight update is judged by the same bound: |dw_gpu - dw_ref| <= lr * (bound_p * max|g_ref| + 2e-5 * max|2 lambda w|)
+ 4 * 2^-24 * max|w| -- the data part as judged, the L2 part in float32 arithmetic, the float32 roundings of the fused tail.
The trainer cases re-synchronise the oracle to the GPU's weights before every step, so every bound is a single-step bound.

All cases use 2 x 64 x 128 pages (char_width 16) of seeds 1 and 9: at 2 x 32 x 64 the data gradients are ~1e-9 of the L2
term, and other seeds make Line down_1/conv_1/b unjudgeable within a few steps (test_f16_training_host.py).

Measured on MI355X (pytest -s; the whole file runs in 4 s, its longest case in 0.7 s):
    largest err_p / dev_p, fused / unfused:  Monochrome 3.30 / 1.00,  Paragraph 3.72 / 1.17,  Line 13.74 / 23.85.
    Line is above the factor 4 at up_2/conv_block/conv_1/b (err 1.8e-3 / 3.1e-3, dev 1.3e-4) and .../w (4.2 / 6.0), both held
    by the 1e-2 floor.  Cause: the binary16 weight OPERANDS of the 4-channel MFMA convs shift a gradient coherently, where
    the per-position storage roundings of stored16 average out in a sum over 4 096 positions; the oracle with those operand
    roundings added gives 2.8e-3 (test_f16_training_host.py::test_weight_operands_explain_the_line_net).  Not a kernel bug.
    unjudgeable parameter-steps in test_trainer_steps_f16_vs_oracle: 2 of 144 in each of the four runs, Line
    down_1/conv_1/b at steps 2 and 4 (dev 9.2e-2, 8.5e-2; the oracle's own trajectory has none); worst weight-update error
    / allowance: Monochrome 0.67, Paragraph 0.23, Line 0.39.
    test_checker_sees_a_wrong_scale: old criterion 3.2e-5 (accepts at 1e-2), this rule err_p 1.01 / 0.99 > bound 3.2e-2.
"""
import hashlib

import numpy as np
import pytest

from conftest import load_golden, rel_linf
from oracle import nn_oracle as O
from test_f16_training_host import (ALL_NETS, DEV_CAP, GRAD_FLOOR, LR, PAGE, PAGE_NETS, STORE_FACTOR, TRAJECTORY_SEEDS,
                                    analytic_net, f32, grad_scale_log2, l2_grads, linf, page_batch, page_case,
                                    stored16_deviation)

pytestmark = pytest.mark.gpu

TOL_NET = 3e-3            # prediction and loss of a whole net in float16 (tests/test_gpu_f16.py)
TOL_EXACT = 2e-5          # float32 / float64 outputs of exact inputs
F32_TAIL = 4 * 2.0 ** -24


@pytest.fixture
def f16():
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    lazy = CP.lazy_losses
    CP.set_dtype('float16')
    yield CP
    CP.set_dtype('float32')
    CP.f16_grad_scale_log2 = None
    CP.lazy_losses = lazy


def nest(flat):
    out = {}
    for key, value in flat.items():
        layer, pname = key.rsplit('/', 1)
        out.setdefault(layer, {})[pname] = value.tolist()
    return out


def bare_model(name, shape, params, fuse, lr=LR):
    from univer_ocr_amd.my_model.model import NET_MAKERS
    from univer_ocr_amd.nn.optimizers import Momentum
    model = NET_MAKERS[name](shape, Momentum(lr=lr, momentum=0))
    model.set_weights(nest(params))
    model.enable_fusion(fuse)
    return model


_ORACLE = {}


def oracle_step(name, seed, weights):
    """What the oracle says about one step of net `name` on the page batch of `seed` from float32 `weights`: prediction,
    loss, data gradients, L2 terms, the stored16 deviation and the bound of every parameter.  Computed once per
    (net, batch, weights) and shared: the trainer cases reach the same weights whenever the GPU is deterministic."""
    key = (name, seed, hashlib.sha1(b''.join(np.ascontiguousarray(weights[pn]).tobytes() for pn in sorted(weights))).digest())
    if key not in _ORACLE:
        X, y = page_case(name, seed)
        X16 = O.round16(X)
        net = O.make_net(name, {pn: np.array(w, dtype=np.float64) for pn, w in weights.items()})
        pred, loss, grads = net.data_grads(X16, y)
        dev = stored16_deviation(net, X16, y, grads, grad_scale_log2())
        reg = l2_grads(net)
        _ORACLE[key] = dict(pred=pred, loss=loss, grads=grads, dev=dev,
                            l2_loss=sum(v[0] for v in reg.values()), l2={pn: v[1] for pn, v in reg.items()},
                            bound={pn: max(GRAD_FLOOR, STORE_FACTOR * d) for pn, d in dev.items()},
                            unjudgeable=sorted(pn for pn, d in dev.items() if not d <= DEV_CAP))
    return _ORACLE[key]


def check_unjudgeable(ref, what, step):
    if ref['unjudgeable']:
        print(f'{what}: unjudgeable at step {step}: ' + ', '.join(f'{pn} (dev {ref["dev"][pn]:.2e})' for pn in ref['unjudgeable']))
    assert len(ref['unjudgeable']) <= (0 if step == 0 else 1), (what, step, ref['unjudgeable'])
    return len(ref['unjudgeable'])


def check_update(ref, before, after, lr, what):
    """the weight update of one SGD step by the inequality of the module docstring; returns the worst error / allowance"""
    worst = 0.0
    for pn, w in before.items():
        assert np.all(np.isfinite(after[pn])), (what, pn)
        if pn in ref['unjudgeable']:
            continue
        g, l2 = ref['grads'][pn], ref['l2'][pn]
        allowed = lr * (ref['bound'][pn] * linf(g) + TOL_EXACT * linf(l2)) + F32_TAIL * linf(w)
        err = linf((after[pn] - w) + lr * (g + l2))
        assert err <= allowed, f'{what} {pn}: update off by {err:.3e} > {allowed:.3e} (bound {ref["bound"][pn]:.2e})'
        worst = max(worst, err / allowed)
    return worst


@pytest.mark.parametrize('name', PAGE_NETS)
@pytest.mark.parametrize('fuse', [True, False])
def test_data_gradients_f16(name, fuse, f16):
    """One bare net, analytic weights, the page batch of seed 1: prediction, loss, every data gradient by the rule, then
    train_finish (L2 + SGD in the fused tail): regularisation loss and the weight update.  Prints err_p, dev_p and
    the largest err_p / dev_p (-s); the figures measured on MI355X are in the module docstring."""
    CP = f16
    X, y = page_case(name, 1)
    net = analytic_net(name)
    ref = oracle_step(name, 1, net.params)
    assert check_unjudgeable(ref, name, 0) == 0
    model = bare_model(name, X.shape, net.params, fuse)
    model.train_begin(CP.copy(X), CP.copy(y))
    if fuse:
        assert len(model._pairs_used) == (name == 'Monochrome') and len(model._ups_used) == 2 * (name != 'Monochrome')
    pred = CP.asnumpy(model.layers_outputs[0]).astype(np.float64)
    loss = float(model._pending_losses[0])
    grads = {pn: CP.asnumpy(p.grad).astype(np.float64) for pn, p in model.params().items()}
    assert sorted(grads) == sorted(ref['grads'])
    assert rel_linf(pred, ref['pred']) <= TOL_NET
    assert abs(loss - ref['loss']) <= TOL_NET * abs(ref['loss'])
    worst, failed = 0.0, []
    for pn in sorted(grads):
        err, dev, bound = rel_linf(grads[pn], ref['grads'][pn]), ref['dev'][pn], ref['bound'][pn]
        print(f'{pn} fuse={fuse}: err {err:.2e} dev {dev:.2e} bound {bound:.2e} err/dev {err / dev:.2f}')
        worst = max(worst, err / dev)
        if not err <= bound:
            failed.append(f'{pn}: err {err:.2e} > bound {bound:.2e} (dev {dev:.2e})')
    print(f'{name} fuse={fuse}: largest err_p / dev_p {worst:.2f}')
    assert not failed, failed
    losses = model.train_finish()
    assert abs(float(losses['regularization_loss']) - ref['l2_loss']) <= TOL_EXACT * ref['l2_loss']
    after = {pn: CP.asnumpy(p.value).astype(np.float64) for pn, p in model.params().items()}
    check_update(ref, net.params, after, LR, f'{name} fuse={fuse}')


def test_checker_sees_a_wrong_scale(f16, monkeypatch):
    """The rule bites where the old criterion does not.  One weight-gradient launch of the Paragraph net (up_2, fused:
    uocr_upconv2x_bwd_weight, unfused: uocr_conv2d_bwd_weight) receives dy with gscale lowered by one -- a legal launch
    with another scalar -- which doubles that layer's dw and db.  At the inputs of test_page_net_step_f16_vs_oracle
    (seed 31) the old criterion, 1e-2 of max|data + L2|, still accepts up_2/conv_block/conv_1/w; the rule of this file
    rejects it with err_p ~ 1 and accepts every parameter of the other layers."""
    from univer_ocr_amd.nn import ops
    from univer_ocr_amd.nn.gpu import DeviceArray
    CP = f16
    name, layer_name = 'Paragraph', 'Paragraph/up_2/conv_block/conv_1'
    X, y = page_case(name, 31)
    net = analytic_net(name)
    ref = oracle_step(name, 31, net.params)
    assert not ref['unjudgeable']
    for fuse in (True, False):
        model = bare_model(name, X.shape, net.params, fuse)
        layer, seen = model.layers[layer_name], []

        def lowered(original, layer=layer, seen=seen):
            def wrapped(x, dy, dw, *args, **kwargs):
                if dw.ptr == layer.w._grad.ptr:
                    seen.append((original.__name__, dy.gscale))
                    dy = DeviceArray(dy.t, dy.gscale - 1)
                return original(x, dy, dw, *args, **kwargs)
            return wrapped
        Xd, yd = CP.copy(X), CP.copy(y)
        with monkeypatch.context() as patch:
            patch.setattr(ops, 'upconv2x_bwd_weight', lowered(ops.upconv2x_bwd_weight))
            patch.setattr(ops, 'conv2d_bwd_weight', lowered(ops.conv2d_bwd_weight))
            model.compute_loss_and_gradients(Xd, yd)                     # what the old test reads: data + L2
            total = {pn: CP.asnumpy(p.grad).astype(np.float64) for pn, p in model.params().items()}
            model.train_begin(Xd, yd)                                    # what this file reads: data alone
            data = {pn: CP.asnumpy(p.grad).astype(np.float64) for pn, p in model.params().items()}
        assert seen == [('upconv2x_bwd_weight' if fuse else 'conv2d_bwd_weight', grad_scale_log2())] * 2
        w = layer_name + '/w'
        old_err = rel_linf(total[w], ref['grads'][w] + ref['l2'][w])
        new_err = rel_linf(data[w], ref['grads'][w])
        print(f'fuse={fuse}: {w} doubled: old criterion {old_err:.2e} (passes at 1e-2), new rule {new_err:.2f} > {ref["bound"][w]:.2e}')
        assert old_err <= GRAD_FLOOR, 'the old criterion was expected to accept the doubled data gradient'
        assert 0.9 <= new_err <= 1.1 and new_err > ref['bound'][w]
        for pn in data:
            if not pn.startswith(layer_name + '/'):
                assert rel_linf(data[pn], ref['grads'][pn]) <= ref['bound'][pn], pn


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('net_name', ALL_NETS)
def test_data_gradients_f32_f64(net_name, fused, dtype):
    """The same train_begin reading in float32 and float64 for the four nets at the golden inputs: the float32 legs of
    test_gpu_models.py::test_my_model_net judge 2e-5 of a total that is mostly L2.  Tolerances: the per-pass gradient
    tolerances, 2e-5 / 1e-11 of max|g_data|; the oracle runs on the values the device holds."""
    from univer_ocr_amd.nn import CP
    g = load_golden(f'my_model_{net_name.lower()}')
    held = f32 if dtype == 'float32' else (lambda a: np.asarray(a, dtype=np.float64))
    X, y = held(g['sgd/X']), held(g['sgd/y'])
    net = O.make_net(net_name)
    net.params = {pn: held(v) for pn, v in net.params.items()}
    _, loss, data = net.data_grads(X, y)
    tol = {'float32': 2e-5, 'float64': 1e-11}[dtype]
    CP.use_gpu(0)
    CP.set_dtype(dtype)
    try:
        model = bare_model(net_name, tuple(int(v) for v in g['in_shape']), net.params, fused, lr=0.01)
        model.train_begin(CP.copy(X), CP.copy(y))
        assert abs(float(model._pending_losses[0]) - loss) <= tol * abs(loss)
        assert sorted(model.params()) == sorted(data)
        for pn, p in model.params().items():
            err = rel_linf(CP.asnumpy(p.grad), data[pn])
            assert err <= tol, f'{pn}: data gradient {err:.2e} > {tol:.0e}'
    finally:
        CP.set_dtype('float32')


def page_trainer(optimizer, lr, graphs, pipelined):
    from univer_ocr_amd.my_model.trainer import PageTrainer
    trainer = PageTrainer(*PAGE, optimizer=optimizer, lr=lr, seed=3, nets=PAGE_NETS, graphs=graphs, pipelined=pipelined)
    for name, model in trainer.models.items():
        model.set_weights(nest(analytic_net(name).params))
    return trainer


def trainer_weights(trainer):
    return {name: {pn: p.value.numpy().astype(np.float64) for pn, p in model.params().items()}
            for name, model in trainer.models.items()}


@pytest.mark.parametrize('graphs', [False, True], ids=['eager', 'graphs'])
@pytest.mark.parametrize('pipelined', [False, True], ids=['joined', 'pipelined'])
def test_trainer_steps_f16_vs_oracle(graphs, pipelined, f16):
    """The step bench.py --config highres-fp16 times (PageTrainer in float16, lanes, fused optimizer tail; with graphs:
    gscale baked into captured launches, binary16 static inputs refilled in place), six SGD steps alternating two batches:
    steps 0 and 1 eager, step 2 captures, 3 to 5 replay.  No free-running trajectory: before every step the oracle is set
    to the GPU's weights, so loss, prediction, regularisation loss and the weight update are single-step comparisons."""
    CP = f16
    CP.lazy_losses = True
    trainer = page_trainer('sgd', LR, graphs, pipelined)
    assert trainer.lanes is not None and trainer.graphs == graphs and trainer.pipelined == pipelined
    unjudgeable, worst = 0, {name: 0.0 for name in PAGE_NETS}
    for step in range(6):
        seed = TRAJECTORY_SEEDS[step % 2]
        trainer.join()
        before = trainer_weights(trainer)
        context = trainer.make_context(page_batch(seed))
        losses = trainer.step(context)
        trainer.join()
        after = trainer_weights(trainer)
        for name in PAGE_NETS:
            what = f'{name} step {step}'
            ref = oracle_step(name, seed, before[name])
            unjudgeable += check_unjudgeable(ref, what, step)
            loss = float(losses[name]['output_losses'][0])
            assert abs(loss - ref['loss']) <= TOL_NET * abs(ref['loss']), what
            pred = CP.asnumpy(context[f'{name.lower()}_pred'])
            assert pred.dtype == np.float16 and rel_linf(pred.astype(np.float64), ref['pred']) <= TOL_NET, what
            assert abs(float(losses[name]['regularization_loss']) - ref['l2_loss']) <= TOL_EXACT * ref['l2_loss'], what
            # not vacuous: some parameter of the net moves mostly by its data gradient
            assert any(linf(ref['grads'][pn]) >= linf(ref['l2'][pn]) for pn in ref['grads']), what
            worst[name] = max(worst[name], check_update(ref, before[name], after[name], LR, what))
    assert (trainer._captured is not None) == graphs
    print(f'graphs={graphs} pipelined={pipelined}: unjudgeable parameter-steps {unjudgeable}; worst update error / allowance '
          + ', '.join(f'{name} {v:.2f}' for name, v in worst.items()))


def test_graphs_and_pipelining_change_nothing_f16(f16):
    """The float16 twin of test_graph_replay_matches_eager_steps and test_pipelined_lanes_match_joined_steps: graphs on or
    off times pipelined on or off, Adam, eight steps over three batches, losses read only after the last step (through the
    snapshot ring where there are graphs).  Loss history, published predictions and final weights are bit-identical."""
    CP = f16
    CP.lazy_losses = True
    results = {}
    for graphs in (False, True):
        for pipelined in (False, True):
            trainer = page_trainer('adam', 0.001, graphs, pipelined)
            kept = []
            for i in range(8):
                context = trainer.make_context(page_batch((1, 9, 13)[i % 3]))
                kept.append(trainer.step(context))
            trainer.join()
            preds = {label: CP.asnumpy(context[label]) for label in ('line_pred', 'monochrome_pred')}
            history = [{n: [float(v) for v in l['output_losses']] + [float(l['regularization_loss'])]
                        for n, l in losses.items()} for losses in kept]
            assert (trainer._captured is not None) == graphs
            results[graphs, pipelined] = (history, preds, trainer_weights(trainer))
    history, preds, weights = results[False, False]
    assert len({tuple(step['Line']) for step in history}) == 8
    assert all(np.isfinite(v) for step in history for row in step.values() for v in row)
    for key, (h, p, w) in results.items():
        assert h == history, key
        for label in preds:
            assert np.array_equal(p[label], preds[label]), (key, label)
        for name in weights:
            for pn in weights[name]:
                assert np.array_equal(w[name][pn], weights[name][pn]), (key, pn)


def test_f16_dense_is_refused(f16):
    """float16 mode leaves the Char net out by a clean error, not by wrong numbers: uocr_gemm has no binary16 form (the
    MFMA GEMM is float32 only, the generic kernel float32 / float64), so a dense layer on binary16 activations raises."""
    from univer_ocr_amd.hip.lib import HipError
    from univer_ocr_amd.nn import ops
    CP = f16
    rng = np.random.default_rng(0)
    x = CP.copy(rng.standard_normal((8, 32)))
    w = CP.copy(rng.standard_normal((33, 16)), np.float32)
    assert x.dtype == np.float16
    with pytest.raises(HipError):
        ops.dense_fwd(x, w)
