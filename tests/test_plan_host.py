"""The step lists that nn/plan.py compiles, checked on the host: the graphs of tests/test_gpu_fused_graphs.py and a few
hundred seeded random chains, built under the recording backend of tests/test_launch_trace.py (no GPU).

What a step list must satisfy whatever the graph:
  * the derivative of every activation is applied EXACTLY ONCE in a backward pass -- counted here by the executor's
    rules (Model._backward_pass): a PLAIN activation applies its own; the producer of an ALIAS activation applies it
    unless its step says `act_folded` or the loss kernel took it over (`loss_folded`; a PAIR step knows the second
    reason only); every step with the activation as `in_act` applies it in its dx epilogue; a pair's inner LeakyReLU
    is applied inside the pair kernel;
  * one step per node of the model's topological order, in that order; every ABSORBED node lies inside exactly one
    step; no step reads an ABSORBED node; an ALIAS names a step that produces a tensor; the gradient a step returns is
    the one its sources' steps look up;
  * the multi-layer kernels are used only in float32 and only with their enable_fusion flag on.
"""
import numpy as np
import pytest

from test_gpu_fused_graphs import (FLATTEN, FUSIONS, GRAPHS, SIGMOID, UP2, UP3, WINDOWS8, build_model, chain, conv, dense,
                                   leaky, routes_expected, routes_used)
from test_launch_trace import recording

ALPHAS = (-0.1, 0.0, 0.01, 1.0, 1.5)
POOL = ('maxpool', dict(ks=2))


def random_chain(seed):
    """A chain over {conv (varied kernel, channels, padding, padding_value, bias), LeakyReLU (ALPHAS), Sigmoid,
    Upsample2D(2 / 3), MaxPool, windows + flatten + dense}; pair-, upsample+conv- and windows-shaped runs are drawn as
    wholes about as often as single layers, with random neighbours and random departures from the exact pattern."""
    rng = np.random.default_rng(seed)
    pick = lambda options: options[rng.integers(len(options))]           # noqa: E731
    c, h, w = int(pick((1, 2, 4))), int(pick((6, 8, 9))), int(pick((8, 12, 16)))
    in_shape, specs, flat = (2, h, w, c), [], None                       # flat: the width of a 2-D tensor

    def activation():
        return SIGMOID if rng.random() < 0.4 else leaky(float(pick(ALPHAS)))

    def add_conv(ks, cout, pad, pv=0.0, bias=True):
        nonlocal c, h, w
        if h + 2 * pad < ks or w + 2 * pad < ks:
            return
        specs.append(conv(ks, c, cout, pad, pv, bias))
        c, h, w = cout, h + 2 * pad - ks + 1, w + 2 * pad - ks + 1

    for _ in range(int(rng.integers(2, 7))):
        kind = pick(('conv', 'conv', 'act', 'pair', 'pair', 'up', 'up', 'windows', 'windows', 'pool', 'up3'))
        if flat is not None:
            specs.extend([dense(flat, int(pick((5, 32)))), activation()] if kind != 'act' else [activation()])
            flat = specs[-2][1]['n_out'] if kind != 'act' else flat
        elif kind == 'conv':
            add_conv(int(pick((1, 3, 5))), int(pick((1, 2, 4, 16))), int(pick((0, 1, 2))), float(pick((0.0, 0.5))),
                     bool(rng.random() < 0.8))
        elif kind == 'act':
            specs.append(activation())
        elif kind == 'pair':
            if c != 1 or rng.random() < 0.3:
                add_conv(3, 1, 1)
                if rng.random() < 0.7:
                    specs.append(activation())
            add_conv(3, 16, 1, float(pick((0.0, 0.0, 0.5))), bool(rng.random() < 0.8))
            specs.append(leaky(float(pick(ALPHAS + (0.01, 0.01)))))
            add_conv(3, 1, 1, float(pick((0.0, 0.0, 0.0, 0.5))), bool(rng.random() < 0.8))
            if rng.random() < 0.6:
                specs.append(activation())
        elif kind in ('up', 'up3') and h * w <= 600:
            if c not in (1, 4) and rng.random() < 0.7:
                add_conv(3, int(pick((1, 4))), 1)
            if rng.random() < 0.7:
                specs.append(activation())
            scale = 3 if kind == 'up3' else 2
            specs.append(UP3 if scale == 3 else UP2)
            h, w = h * scale, w * scale
            add_conv(5, c, 2, float(pick((0.0, 0.0, 0.0, 0.5))))
            if rng.random() < 0.7:
                specs.append(activation())
        elif kind == 'windows' and w >= 8:
            if rng.random() < 0.7:
                add_conv(3, int(pick((8, 32, 32))), 1)
                specs.append(activation())
            specs.extend([WINDOWS8, FLATTEN, dense(h * 8 * c, int(pick((5, 32, 32))))])
            flat = specs[-1][1]['n_out']
        elif kind == 'pool' and h >= 2 and w >= 2:
            specs.append(POOL)
            h, w = h // 2, w // 2
    if not specs or specs[0][0] not in ('conv', 'dense'):                  # (a model needs a parameter)
        specs.insert(0, conv(1, in_shape[3], in_shape[3]))
    return chain(specs, in_shape, 'softmax_ce' if flat is not None else 'dice')


def all_cases():
    cases = dict(GRAPHS)
    cases.update({f'random_{seed}': random_chain(seed) for seed in range(300)})
    return cases


def derivative_counts(model, loss_folded=()):
    """{activation node: how many times a backward pass over the step list applies its derivative}."""
    from univer_ocr_amd.nn import plan
    from univer_ocr_amd.nn.layers import LeakyRelu, Sigmoid
    steps = model._compiled().steps
    counts = {}
    for step in steps:
        if not isinstance(model.layers[step.node], (LeakyRelu, Sigmoid)):
            continue
        node, layer = step.node, model.layers[step.node]
        count = sum(1 for other in steps if other.in_act is layer)
        if step.kind == plan.PLAIN:
            count += 1
        elif step.kind == plan.ALIAS:
            producer, = [other for other in steps if other.act_node == node]
            assert producer.node == step.alias_of and producer.act is layer
            folded = node in loss_folded or (producer.act_folded and producer.kind != plan.PAIR)
            count += 0 if folded else 1
        else:                                              # the inner LeakyReLU of a pair: applied by the pair kernel
            assert step.kind == plan.ABSORBED
            count += sum(1 for other in steps if other.kind == plan.PAIR and other.first_act is layer)
        counts[node] = count
    return counts


def check_structure(model):
    from univer_ocr_amd.nn import plan
    compiled = model._compiled()
    steps = compiled.steps
    assert [step.node for step in steps] == list(model._plan)
    by_node = {step.node: step for step in steps}
    tensors = (plan.PLAIN, plan.FUSED, plan.PAIR, plan.UP, plan.WINDOWS)
    for step in steps:
        if step.kind == plan.ABSORBED:
            assert sum(step.node in other.inside for other in steps) == 1, step.node
            continue
        assert not any(by_node[n].kind != plan.ABSORBED for n in step.inside), step.node
        assert all(isinstance(s, int) or by_node[s].kind != plan.ABSORBED for s in step.sources), step.node
        if step.kind == plan.ALIAS:
            assert by_node[step.alias_of].kind in tensors and model.relations[step.node] == [step.alias_of]
        else:
            # what its backward returns is stored under grad_node: the sources' steps look it up under that name
            assert model.relations[step.grad_node] == step.sources, step.node
    return compiled


CASES = all_cases()


def test_random_chains_reach_every_step_kind():
    """The generator is not blind: over its chains every step kind occurs, each many times, and so do the positions
    the nets never build (an activation folded into a pair's neighbour is what the counts below are about)."""
    from univer_ocr_amd.nn import plan
    seen = {}
    with recording('float32'):
        for name, case in CASES.items():
            if name.startswith('random_'):
                for step in build_model(case, {})._compiled().steps:
                    seen[step.kind] = seen.get(step.kind, 0) + 1
                    if step.in_act is not None:
                        seen[step.kind, 'in_act'] = seen.get((step.kind, 'in_act'), 0) + 1
    for kind in (plan.PLAIN, plan.FUSED, plan.ALIAS, plan.ABSORBED):
        assert seen.get(kind, 0) >= 100, (kind, seen)
    for kind in (plan.PAIR, plan.UP, plan.WINDOWS, (plan.FUSED, 'in_act'), (plan.UP, 'in_act'), (plan.WINDOWS, 'in_act')):
        assert seen.get(kind, 0) >= 20, (kind, seen)


@pytest.mark.parametrize('fusion', list(FUSIONS))
@pytest.mark.parametrize('skip', [False, True], ids=['full', 'skip'])
def test_every_derivative_is_applied_exactly_once(fusion, skip):
    wrong = {}
    with recording('float32'):
        for name, case in CASES.items():
            model = build_model(case, FUSIONS[fusion], skip)
            compiled = check_structure(model)
            counts = derivative_counts(model)
            if any(count != 1 for count in counts.values()):
                wrong[name] = {node: count for node, count in counts.items() if count != 1}
            folded = set(compiled.output_sigmoid) - {None}
            counts = derivative_counts(model, folded)
            if any(count != (0 if node in folded else 1) for node, count in counts.items()):
                wrong[name, 'loss_folded'] = counts
    assert not wrong, wrong


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_multi_layer_kernels_only_in_float32_and_with_their_flag(dtype):
    with recording(dtype):
        for name, case in CASES.items():
            for fusion in FUSIONS.values():
                model = build_model(case, fusion)
                used = routes_used(model)
                if dtype == 'float64' or fusion is None:
                    assert not used, name
                if fusion is not None and fusion.get('pairs') is False:
                    assert not used & {'pairs', 'ups'}, name
                if fusion is not None and fusion.get('windows') is False:
                    assert 'wins' not in used, name
                if name in GRAPHS:
                    assert used == routes_expected(case, fusion, dtype), name
                if dtype == 'float64':
                    check_structure(model)
                    assert set(derivative_counts(model).values()) <= {1}, name


def test_the_graphs_take_the_steps_they_were_written_for():
    """With every fusion on, in float32: the position each graph of test_gpu_fused_graphs.py is about."""
    from univer_ocr_amd.nn import plan
    from univer_ocr_amd.nn.layers import Sigmoid

    def steps_of(name):
        model = build_model(GRAPHS[name], {})
        return model, {step.node: step for step in model._compiled().steps}
    with recording('float32'):
        model, steps = steps_of('c1_sigmoid_into_dx')
        assert steps['04_conv'].kind == plan.FUSED and isinstance(steps['04_conv'].in_act, Sigmoid)
        assert steps['02_conv'].act_folded and steps['00_conv'].act_folded
        for name in ('c2_leaky_pair', 'c2_sigmoid_pair'):                   # the activation in front keeps its derivative
            model, steps = steps_of(name)
            assert steps['04_conv'].kind == plan.PAIR and steps['04_conv'].sources == ['01_' + name.split('_')[1]]
            assert steps['00_conv'].kind == plan.FUSED and not steps['00_conv'].act_folded
        model, steps = steps_of('c3_pair_sigmoid_conv')                    # the pair's Sigmoid folds into no consumer
        assert steps['02_conv'].kind == plan.PAIR and steps['04_conv'].in_act is None
        model, steps = steps_of('c3_pair_leaky_conv')
        assert not model._pairs_used and steps['02_conv'].kind == plan.FUSED and steps['04_conv'].in_act is not None
        model, steps = steps_of('c4_pair_sigmoid')
        assert model._compiled().output_sigmoid == ['03_sigmoid']
        for name in ('c5_ups_c4', 'c5_ups_c1'):
            model, steps = steps_of(name)
            assert isinstance(steps['03_conv'].in_act, Sigmoid) and steps['06_conv'].in_act is model.layers['04_leaky']
            assert steps['03_conv'].kind == steps['06_conv'].kind == plan.UP
        for name, kind in (('c6_windows_leaky', 'leaky'), ('c6_windows_sigmoid', 'sigmoid')):
            model, steps = steps_of(name)
            assert steps['04_dense'].kind == plan.WINDOWS and steps['04_dense'].in_act is model.layers[f'01_{kind}']
        model, steps = steps_of('c6_windows_narrow')
        assert [steps[n].kind for n in ('02_fixed_width', '03_flatten')] == [plan.PLAIN] * 2
        assert steps['04_dense'].kind == plan.FUSED
        for tag, kind in (('1', plan.ABSORBED), ('1p5', plan.ALIAS), ('0', plan.PLAIN), ('neg', plan.PLAIN)):
            model, steps = steps_of(f'c7_pair_alpha_{tag}')
            assert steps['03_leaky'].kind == kind and bool(model._pairs_used) == (tag == '1')
            model, steps = steps_of(f'c7_chain1_alpha_{tag}')
            assert steps['01_leaky'].kind == (plan.ALIAS if tag in ('1', '1p5') else plan.PLAIN)
        model, steps = steps_of('d1_act_two_convs')
        assert steps['act'].kind == plan.ALIAS and not steps['conv'].act_folded
        assert steps['left'].in_act is None and steps['right'].in_act is None
        model, steps = steps_of('d2_act_output_and_conv')
        assert steps['act'].kind == plan.ALIAS and not steps['conv'].act_folded and steps['next'].in_act is None
        assert model._compiled().output_sigmoid == [None, None]
        model, steps = steps_of('d3_conv_two_consumers')
        assert steps['conv'].kind == steps['act'].kind == plan.PLAIN
        model, steps = steps_of('d4_up_two_convs')
        assert steps['up'].kind == plan.PLAIN and not model._ups_used
        model, steps = steps_of('d5_two_output_sigmoids')
        assert model._compiled().output_sigmoid == ['left_sigmoid', 'right_sigmoid']
        model, steps = steps_of('d6_sigmoid_two_outputs')
        assert steps['sigmoid'].kind == plan.ALIAS and model._compiled().output_sigmoid == [None, None]
