"""Fused step lists (nn/plan.py) on hand-built graphs against the float64 oracle.

The four nets reach every fusion kind in one position each.  The graphs here put each kind where the nets never do:
a Sigmoid folded into the dx epilogue of a conv, an upsample+conv and a windows+dense step; a conv pair fed by a fused
activation, and one whose Sigmoid feeds a conv (both got an activation derivative never / twice before the step
compiler stopped folding across the edge of a pair); fused LeakyReLUs with alpha 1, 1.5, 0 and -0.1; the near misses
of every pattern; and DAGs in which a fused activation has two consumers, is a model output, or must not fuse.

Every graph runs unfused, fused, fused without pairs and fused without windows, with and without skip_input_grads,
in float32 and float64, from analytic weights on a seeded input: prediction, loss row, input gradients and every
parameter gradient of compute_loss_and_gradients, then the loss rows and all weights of two train steps with
Momentum(0.01, 0.9) (state that a fused step keeps between steps), against oracle.Graph.  Graphs that end in ONE
fused Sigmoid also run forward + backward(grads) with an explicit gradient: the path on which no loss kernel takes
the Sigmoid's derivative over.

Tolerances (normalised max error, as tests/test_gpu_models.py): single passes 1e-5 / 1e-11, gradients 2e-5 / 2e-11,
after the steps 5e-5 / 1e-10 (float32 / float64).  In float32 every graph asserts which of the pair / upsample+conv /
windows kernels its step list uses, so that no case can quietly stop reaching the kernel it was written for.

test_inputs_are_well_conditioned (no GPU) asserts with the oracle alone, for every graph at every pass compared, that
each LeakyReLU sees both signs, that no pre-activation of a LeakyReLU lies within 4e-5 max|z| of zero (four times the
float32 forward tolerance: the derivative taken from the output cannot then legitimately differ from the one taken
from the input) and that every Sigmoid output lies in [0.02, 0.98].  No element is left out of any comparison.

Worst errors measured on MI355X (printed per case with -s): float32 2.5e-7 (passes), 3.5e-6 (gradients), 4.1e-7
(after the steps); float64 8.8e-16, 1.3e-14, 2.9e-15.  With the step compiler as it was before nothing folded across
a pair's edge, the c2_* graphs and c7_pair_alpha_1 were off by 0.9 - 3.2 (gradients of the conv in front of the pair,
input gradient) and c3_pair_sigmoid_conv by 0.75 (every gradient of the pair) in float32; float64 forms no pair.
Per graph, over the four fusion settings and both skip_input_grads settings (route: what the float32 step list uses
with every fusion on):

                             route        float32: pass, gradients, steps | float64
  c1_sigmoid_into_dx         fused only   1.2e-07 4.2e-07 1.2e-07 | 1.5e-16 1.1e-15 1.8e-16
  c2_leaky_pair              pairs        1.4e-07 3.2e-07 2.8e-07 | 3.1e-16 2.6e-15 2.0e-15
  c2_leaky_pair_sigmoid      pairs        1.0e-07 3.0e-06 1.4e-07 | 3.3e-16 1.3e-14 2.9e-15
  c2_sigmoid_pair            pairs        1.5e-07 2.6e-07 4.1e-07 | 3.2e-16 3.4e-15 6.6e-16
  c2_sigmoid_pair_sigmoid    pairs        1.0e-07 8.7e-07 1.9e-07 | 1.7e-16 9.3e-15 6.6e-16
  c3_pair_sigmoid_conv       pairs        5.3e-08 2.3e-07 1.0e-07 | 1.3e-16 2.1e-15 6.5e-16
  c3_pair_conv               pairs        1.2e-07 3.5e-07 1.3e-07 | 3.3e-16 1.3e-15 4.2e-16
  c3_pair_leaky_conv         fused only   5.3e-08 1.9e-07 9.1e-08 | 2.1e-16 1.9e-15 3.3e-16
  c4_pair_sigmoid            pairs        1.1e-07 3.4e-07 9.6e-08 | 3.0e-16 1.6e-15 1.6e-16
  c5_ups_c4                  ups          2.1e-07 3.5e-06 1.1e-07 | 2.3e-16 1.0e-14 1.9e-16
  c5_ups_c1                  ups          1.1e-07 1.9e-06 9.6e-08 | 2.2e-16 6.5e-15 1.7e-16
  c6_windows_leaky           wins         2.3e-07 8.0e-07 1.1e-07 | 8.8e-16 1.8e-15 2.2e-16
  c6_windows_sigmoid         wins         1.6e-07 2.5e-06 9.9e-08 | 5.9e-16 2.5e-15 1.1e-16
  c6_windows_narrow          fused only   2.5e-07 5.6e-07 8.3e-08 | 1.4e-16 1.4e-15 1.4e-16
  c8_pair_pv_first           pairs        9.8e-08 1.3e-06 1.1e-07 | 4.6e-16 1.3e-15 2.1e-16
  c8_pair_pv_second          fused only   7.8e-08 2.4e-07 1.2e-07 | 3.0e-16 1.6e-15 1.6e-16
  c8_pair_nobias_first       pairs        1.1e-07 2.1e-07 1.1e-07 | 3.5e-16 2.1e-15 2.2e-16
  c8_pair_nobias_second      pairs        1.2e-07 4.3e-07 8.1e-08 | 2.9e-16 1.6e-15 1.6e-16
  c8_up_pv                   fused only   9.3e-08 1.8e-06 8.9e-08 | 3.0e-16 2.7e-15 2.7e-16
  c8_up_2to2                 fused only   9.3e-08 5.7e-07 6.4e-08 | 2.9e-16 1.0e-15 2.7e-16
  c8_up_scale3               fused only   1.1e-07 1.3e-06 9.9e-08 | 3.0e-16 2.4e-15 3.9e-16
  c7_chain1_alpha_1          fused only   1.1e-07 6.9e-07 1.1e-07 | 1.5e-16 1.1e-15 3.0e-16
  c7_pair_alpha_1            pairs        1.9e-07 3.0e-07 9.5e-08 | 4.1e-16 6.7e-15 8.2e-16
  c7_chain1_alpha_1p5        fused only   1.1e-07 4.9e-07 1.4e-07 | 1.4e-16 1.0e-15 9.4e-17
  c7_pair_alpha_1p5          fused only   8.9e-08 3.1e-07 2.7e-07 | 4.2e-16 9.6e-16 1.0e-15
  c7_chain1_alpha_0          fused only   8.9e-08 2.9e-07 1.0e-07 | 1.4e-16 1.5e-15 1.5e-16
  c7_pair_alpha_0            fused only   7.6e-08 3.4e-07 2.2e-07 | 2.3e-16 2.0e-15 2.8e-16
  c7_chain1_alpha_neg        fused only   1.0e-07 3.1e-07 1.2e-07 | 1.4e-16 1.4e-15 8.8e-17
  c7_pair_alpha_neg          fused only   9.0e-08 3.0e-07 2.0e-07 | 3.2e-16 2.4e-15 2.7e-15
  d1_act_two_convs           fused only   8.3e-08 2.0e-07 9.7e-08 | 1.7e-16 1.1e-15 2.0e-16
  d2_act_output_and_conv     fused only   2.1e-07 2.1e-07 1.0e-07 | 3.4e-16 5.6e-16 2.2e-16
  d3_conv_two_consumers      fused only   8.5e-08 1.5e-07 7.9e-08 | 1.5e-16 6.1e-16 1.5e-16
  d4_up_two_convs            fused only   9.9e-08 2.2e-06 1.1e-07 | 2.1e-16 4.7e-15 4.1e-16
  d5_two_output_sigmoids     fused only   9.5e-08 1.8e-07 9.9e-08 | 1.9e-16 7.8e-16 1.7e-16
  d6_sigmoid_two_outputs     fused only   8.9e-08 1.9e-07 8.3e-08 | 2.4e-16 3.7e-16 2.4e-16
"""
import functools

import numpy as np
import pytest

from conftest import rel_linf
from oracle import nn_oracle as O

PASS_TOL = {'float32': 1e-5, 'float64': 1e-11}
GRAD_TOL = {'float32': 2e-5, 'float64': 2e-11}
STEP_TOL = {'float32': 5e-5, 'float64': 1e-10}
FUSIONS = {'unfused': None, 'fused': {}, 'fused_nopairs': {'pairs': False}, 'fused_nowindows': {'windows': False}}
STEPS = 2


# -- layer specs: (kind, cfg) as oracle.Graph takes them ---------------------------------------------------------------
def conv(ks, cin, cout, pad=0, pv=0.0, bias=True):
    return 'conv', dict(ks=(ks, ks), cin=cin, cout=cout, stride=1, padding=pad, padding_value=pv, bias=bias)


def leaky(alpha=0.01):
    return 'leaky', dict(alpha=alpha)


def dense(n_in, n_out):
    return 'dense', dict(n_in=n_in, n_out=n_out)


SIGMOID, FLATTEN, CONCAT = ('sigmoid', {}), ('flatten', {}), ('concat', {})
UP2, UP3, WINDOWS8 = ('upsample', dict(scale=2)), ('upsample', dict(scale=3)), ('fixed_width', dict(width=8))
PAIR = [conv(3, 1, 16, 1), leaky(), conv(3, 16, 1, 1)]


class Case:
    """One graph: layers / relations, input shapes, one loss per output, the seed of its inputs, labels and explicit
    gradient, the salt of its analytic weights; `route`: the multi-layer kernels its float32 step list uses with every
    fusion on ('pairs' / 'ups' / 'wins', None: fused activations only); `explicit`: it ends in one fused Sigmoid, so backward(grads) is run too."""

    def __init__(self, layers, relations, in_shapes, losses, seed, route=None, explicit=False, salt=0):
        self.layers, self.relations, self.in_shapes, self.losses = layers, relations, in_shapes, losses
        self.seed, self.route, self.explicit, self.salt = seed, route, explicit, salt


def chain(specs, in_shape, loss='dice', seed=0, **more):
    names = [f'{i:02d}_{kind}' for i, (kind, _) in enumerate(specs)]
    relations = dict(zip(names, [0] + names[:-1]))
    relations[0] = names[-1]
    return Case(dict(zip(names, specs)), relations, [in_shape], [loss], seed, **more)


def dag(layers, relations, in_shape, losses, seed=0):
    return Case(layers, relations, [in_shape], losses, seed)


def windows_chain(channels, act, **more):
    return chain([conv(3, 1, channels, 1), act, WINDOWS8, FLATTEN, dense(4 * 8 * channels, 32), leaky(), dense(32, 5)],
                 (2, 4, 16, 1), 'softmax_ce', **more)


def up_chain(c, up=UP2, pv=0.0, **more):
    return chain([conv(3, 2, c, 1), leaky(), up, conv(5, c, c, 2, pv), SIGMOID], (2, 6, 10, 2), explicit=True, **more)


def pair_of(alpha=0.01, pv1=0.0, pv2=0.0, bias1=True, bias2=True):
    return [conv(3, 1, 16, 1, pv1, bias1), leaky(alpha), conv(3, 16, 1, 1, pv2, bias2)]


LOW, PAGE1, PAGE2 = (2, 6, 10, 2), (2, 12, 20, 1), (2, 12, 20, 2)
GRAPHS = {
    # 1: a Sigmoid folded into the dx epilogue of a FUSED conv
    'c1_sigmoid_into_dx': chain([conv(3, 3, 5), leaky(), conv(3, 5, 4), SIGMOID, conv(3, 4, 2)], (2, 9, 14, 3), seed=0),
    # 2: a pair fed by a fused activation (it got no derivative)
    'c2_leaky_pair': chain([conv(3, 2, 1, 1), leaky()] + PAIR, PAGE2, seed=0, route='pairs'),
    'c2_leaky_pair_sigmoid': chain([conv(3, 2, 1, 1), leaky()] + PAIR + [SIGMOID], PAGE2, seed=0, route='pairs',
                                   explicit=True),
    'c2_sigmoid_pair': chain([conv(3, 2, 1, 1), SIGMOID] + PAIR, PAGE2, seed=0, route='pairs'),
    'c2_sigmoid_pair_sigmoid': chain([conv(3, 2, 1, 1), SIGMOID] + PAIR + [SIGMOID], PAGE2, seed=0, route='pairs',
                                     explicit=True),
    # 3: a pair whose Sigmoid feeds a conv (it got the derivative twice); its neighbours
    'c3_pair_sigmoid_conv': chain(PAIR + [SIGMOID, conv(3, 1, 3)], PAGE1, seed=0, route='pairs'),
    'c3_pair_conv': chain(PAIR + [conv(3, 1, 3)], PAGE1, seed=0, route='pairs'),
    'c3_pair_leaky_conv': chain(PAIR + [leaky(), conv(3, 1, 3)], PAGE1, seed=0),
    # 4: the pair and its Sigmoid as the model output: Dice folds the Sigmoid, the explicit gradient does not
    'c4_pair_sigmoid': chain(PAIR + [SIGMOID], PAGE1, seed=0, route='pairs', explicit=True),
    # 5: Sigmoid and LeakyReLU folded into the dx of upsample+conv steps, 4 and 1 channels
    'c5_ups_c4': chain([conv(3, 2, 4, 1), SIGMOID, UP2, conv(5, 4, 4, 2), leaky(), UP2, conv(5, 4, 4, 2), SIGMOID], LOW,
                       seed=0, route='ups', explicit=True),
    'c5_ups_c1': chain([conv(3, 2, 1, 1), SIGMOID, UP2, conv(5, 1, 1, 2), leaky(), UP2, conv(5, 1, 1, 2), SIGMOID], LOW,
                       seed=0, route='ups', explicit=True),
    # 6: LeakyReLU / Sigmoid folded into the dx of a windows step; 8 channels: the three layers stay separate
    'c6_windows_leaky': windows_chain(32, leaky(), seed=0, route='wins'),
    'c6_windows_sigmoid': windows_chain(32, SIGMOID, seed=0, route='wins'),
    'c6_windows_narrow': windows_chain(8, leaky(), seed=0),
    # 8: near misses of the pair and of upsample+conv
    'c8_pair_pv_first': chain(pair_of(pv1=0.5) + [SIGMOID], PAGE1, seed=0, route='pairs', explicit=True),
    'c8_pair_pv_second': chain(pair_of(pv2=0.5) + [SIGMOID], PAGE1, seed=0, explicit=True),
    'c8_pair_nobias_first': chain(pair_of(bias1=False) + [SIGMOID], PAGE1, seed=0, route='pairs', explicit=True),
    'c8_pair_nobias_second': chain(pair_of(bias2=False) + [SIGMOID], PAGE1, seed=0, route='pairs', explicit=True),
    'c8_up_pv': up_chain(4, pv=0.5, seed=0),
    'c8_up_2to2': up_chain(2, seed=0),
    'c8_up_scale3': up_chain(4, up=UP3, seed=0),
}
# 7: chain 1 and the pair of chain 2 with the inner LeakyReLU at other slopes: the pair forms at 1.0 alone (1.5 is no
# max(z, alpha z); 0 and -0.1 do not fuse at all, the derivative cannot be taken from the output)
for _alpha, _tag in ((1.0, '1'), (1.5, '1p5'), (0.0, '0'), (-0.1, 'neg')):
    GRAPHS[f'c7_chain1_alpha_{_tag}'] = chain([conv(3, 3, 5), leaky(_alpha), conv(3, 5, 4), SIGMOID, conv(3, 4, 2)],
                                              (2, 9, 14, 3), seed=0)
    GRAPHS[f'c7_pair_alpha_{_tag}'] = chain([conv(3, 2, 1, 1), leaky()] + pair_of(_alpha), PAGE2, seed=0,
                                            route='pairs' if _alpha == 1.0 else None)

C23, C32, C44 = conv(3, 2, 3, 1), conv(3, 3, 2, 1), conv(5, 4, 4, 2)
GRAPHS.update({
    # D1: a fused activation consumed by two convs: their gradients are summed, nothing is folded
    'd1_act_two_convs': dag({'conv': C23, 'act': leaky(), 'left': C32, 'right': C32, 'concat': CONCAT},
                            {'conv': 0, 'act': 'conv', 'left': 'act', 'right': 'act', 'concat': ['left', 'right'],
                             0: 'concat'}, (2, 7, 9, 2), ['dice']),
    # D2: a fused activation that is a model output and the input of a conv
    'd2_act_output_and_conv': dag({'conv': C23, 'act': SIGMOID, 'next': C32},
                                  {'conv': 0, 'act': 'conv', 'next': 'act', 0: 'act', 1: 'next'}, (2, 7, 9, 2),
                                  ['dice', 'dice']),
    # D3: a conv consumed by an activation and by a Concat: it must not fuse
    'd3_conv_two_consumers': dag({'conv': C23, 'act': leaky(), 'next': conv(3, 3, 3, 1), 'concat': CONCAT},
                                 {'conv': 0, 'act': 'conv', 'next': 'act', 'concat': ['conv', 'next'], 0: 'concat'},
                                 (2, 7, 9, 2), ['dice']),
    # D4: an Upsample2D(2) consumed by two 5x5 4->4 convs: no upsample+conv step
    'd4_up_two_convs': dag({'conv': conv(3, 2, 4, 1), 'up': UP2, 'left': C44, 'right': C44, 'concat': CONCAT},
                           {'conv': 0, 'up': 'conv', 'left': 'up', 'right': 'up', 'concat': ['left', 'right'],
                            0: 'concat'}, LOW, ['dice']),
    # D5: two fused output Sigmoids: Dice folds its one, the cross-entropy (no `folds_sigmoid`) does not
    'd5_two_output_sigmoids': dag({'conv': C23, 'act': leaky(), 'left': C32, 'left_sigmoid': SIGMOID, 'right': C32,
                                   'right_sigmoid': SIGMOID},
                                  {'conv': 0, 'act': 'conv', 'left': 'act', 'left_sigmoid': 'left', 'right': 'act',
                                   'right_sigmoid': 'right', 0: 'left_sigmoid', 1: 'right_sigmoid'}, (2, 7, 9, 2),
                                  ['dice', 'sigmoid_ce']),
    # D6: one fused Sigmoid wired to two model outputs: not the only consumer, so no loss folds it
    'd6_sigmoid_two_outputs': dag({'conv': C23, 'sigmoid': SIGMOID}, {'conv': 0, 'sigmoid': 'conv', 0: 'sigmoid',
                                                                     1: 'sigmoid'}, (2, 7, 9, 2), ['dice', 'jaccard']),
})
# the seeds (0 where none is given) and weight salts with which test_inputs_are_well_conditioned holds
for _name, _seed in {'c1_sigmoid_into_dx': 2, 'c6_windows_sigmoid': 1, 'c8_pair_pv_first': 4, 'c8_pair_nobias_first': 1,
                     'c7_pair_alpha_1': 4, 'c7_chain1_alpha_0': 2, 'c7_chain1_alpha_neg': 2}.items():
    GRAPHS[_name].seed = _seed
GRAPHS['c5_ups_c4'].salt, GRAPHS['c5_ups_c1'].salt = 1, 5



# -- the oracle's side -----------------------------------------------------------------------------------------------
def make_oracle(case):
    """oracle.Graph with oracle.analytic_weights: salt = case.salt + the layer's place among the sorted names, + 0.5
    per parameter in sorted order (as analytic_net_weights, which starts at salt 0)."""
    spec = [(name, kind, cfg) for name, (kind, cfg) in case.layers.items()]
    shapes, weights = O.param_shapes(spec), {}
    for place, layer in enumerate(sorted(case.layers)):
        for j, pn in enumerate(sorted(p for p in shapes if p.rsplit('/', 1)[0] == layer)):
            weights[pn] = O.analytic_weights(shapes[pn], case.salt + place + 0.5 * j)
    return O.make_graph(case.layers, case.relations, case.losses, weights)


def make_data(case):
    """Seeded inputs in (-1, 1), labels for each loss, and one explicit gradient per output."""
    rng = np.random.default_rng(case.seed)
    Xs = [rng.uniform(-1.0, 1.0, shape) for shape in case.in_shapes]
    shapes = [p.shape for p in make_oracle(case).forward(Xs)]
    ys = []
    for loss, shape in zip(case.losses, shapes):
        if loss == 'softmax_ce':
            ys.append(np.eye(shape[1])[rng.integers(0, shape[1], shape[0])])
        else:
            ys.append(rng.integers(0, 2, shape).astype(np.float64))
    return Xs, ys, [rng.standard_normal(shape) for shape in shapes]


def badly_conditioned(graph, values):
    """What the values of one forward pass break of the conditions in the module docstring."""
    found = []
    for node, (kind, _) in graph.layers.items():
        if kind == 'leaky':
            z = values[graph.relations[node][0]]
            if not (z.min() < 0 < z.max()):
                found.append(f'{node}: one sign only')
            if np.abs(z).min() <= 4e-5 * np.abs(z).max():
                found.append(f'{node}: |z| = {np.abs(z).min():.2e} with max|z| = {np.abs(z).max():.2e}')
        elif kind == 'sigmoid' and not (0.02 <= values[node].min() and values[node].max() <= 0.98):
            found.append(f'{node}: output in [{values[node].min():.3f}, {values[node].max():.3f}]')
    return found


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything the GPU cases of one graph compare with, computed once in float64; nobody changes it."""
    case = GRAPHS[name]
    Xs, ys, Gs = make_data(case)
    graph = make_oracle(case)
    ref = {'Xs': Xs, 'ys': ys, 'Gs': Gs, 'weights': dict(graph.params), 'conditioning': []}
    preds, values, stash = graph.forward(Xs, keep=True)
    ref['conditioning'] += badly_conditioned(graph, values)
    ref['explicit_dxs'], ref['explicit_grads'] = graph.backward(Gs, stash)
    losses, ref['preds'], ref['dxs'] = graph.loss_and_grads(Xs, ys)
    ref['loss'] = np.array([*losses['output_losses'], losses['regularization_loss']])
    ref['grads'] = dict(graph.grads)
    optimizer, rows = O.MomentumState(0.01, 0.9), []
    for _ in range(STEPS):
        ref['conditioning'] += badly_conditioned(graph, graph.forward(Xs, keep=True)[1])
        losses, _ = graph.train_step(Xs, ys, optimizer)
        rows.append([*losses['output_losses'], losses['regularization_loss']])
    ref['step_losses'], ref['stepped'] = np.array(rows), dict(graph.params)
    return ref


# -- the project's side ------------------------------------------------------------------------------------------------
def build_model(case, fusion=None, skip=False):
    """The Model of a case under the current backend and dtype, every parameter on one Momentum(0.01, 0.9)."""
    from univer_ocr_amd.nn import layers as L
    from univer_ocr_amd.nn import losses
    from univer_ocr_amd.nn.models import Model
    from univer_ocr_amd.nn.optimizers import Momentum
    opt = Momentum(lr=0.01, momentum=0.9)
    make = {'conv': lambda c: L.Convolutional2D(c['ks'], c['cin'], c['cout'], padding=c['padding'],
                                                padding_value=c['padding_value'], bias=c['bias'], optimizer=opt),
            'dense': lambda c: L.FullyConnected(c['n_in'], c['n_out'], optimizer=opt),
            'leaky': lambda c: L.LeakyRelu(c['alpha']), 'sigmoid': lambda c: L.Sigmoid(),
            'upsample': lambda c: L.Upsample2D(c['scale']), 'maxpool': lambda c: L.MaxPool2D(c['ks']),
            'flatten': lambda c: L.Flatten(),
            'fixed_width': lambda c: L.Conv2DToBatchedFixedWidthed(c['width']), 'concat': lambda c: L.Concat()}
    loss_of = {'dice': losses.SegmentationDice2D, 'jaccard': losses.SegmentationJaccard2D,
               'sigmoid_ce': losses.SigmoidCrossEntropy, 'softmax_ce': losses.SoftmaxCrossEntropy}
    model = Model({name: make[kind](cfg) for name, (kind, cfg) in case.layers.items()}, dict(case.relations),
                  loss=[loss_of[name]() for name in case.losses])
    model.initialize(list(case.in_shapes))
    if fusion is not None:
        model.enable_fusion(True, **fusion)
    if skip:
        model.skip_input_grads()
    return model


def routes_expected(case, fusion, dtype):
    """Which of _pairs_used / _ups_used / _wins_used the step list of this setting fills."""
    if fusion is None or dtype != 'float32' or case.route is None:
        return set()
    off = {'pairs', 'ups'} if fusion.get('pairs') is False else {'wins'} if fusion.get('windows') is False else set()
    return {case.route} - off


def routes_used(model):
    return {tag for tag, used in (('pairs', model._pairs_used), ('ups', model._ups_used), ('wins', model._wins_used))
            if used}


def test_inputs_are_well_conditioned():
    for name in GRAPHS:
        assert reference(name)['conditioning'] == [], name


@pytest.fixture(params=['float32', 'float64'])
def dt(request):
    from univer_ocr_amd.nn import CP
    CP.set_dtype(request.param)
    yield request.param
    CP.set_dtype('float32')


class Worst:
    """The largest error of each kind of quantity in one case; every figure is printed before it is asserted."""

    def __init__(self, dtype):
        self.dtype, self.seen, self.failed = dtype, {}, []

    def close(self, got, want, tols, kind, what):
        from univer_ocr_amd.nn import CP
        err = rel_linf(CP.asnumpy(got), want)
        self.seen[kind] = max(self.seen.get(kind, 0.0), err)
        if not err <= tols[self.dtype]:
            self.failed.append(f'{what}: rel_linf={err:.3e} > {tols[self.dtype]:.1e}')


def losses_row(losses):
    return np.array([float(v) for v in losses['output_losses']] + [float(losses['regularization_loss'])])


@pytest.mark.gpu
@pytest.mark.parametrize('skip', [False, True], ids=['full', 'skip'])
@pytest.mark.parametrize('fusion', list(FUSIONS))
@pytest.mark.parametrize('name', list(GRAPHS))
def test_fused_graph_matches_the_oracle(name, fusion, skip, dt):
    from univer_ocr_amd.nn import CP
    case, ref = GRAPHS[name], reference(name)
    model = build_model(case, FUSIONS[fusion], skip)
    model.set_weights({layer: {pn: ref['weights'][f'{layer}/{pn}'].tolist() for pn in model.layers[layer].params()}
                       for layer in model.layers if model.layers[layer].params()})
    assert routes_used(model) == routes_expected(case, FUSIONS[fusion], dt)
    Xs, ys = [CP.copy(x) for x in ref['Xs']], [CP.copy(y) for y in ref['ys']]
    inputs = range(len(Xs))
    worst = Worst(dt)

    for k, pred in enumerate(model.predict(Xs)):
        worst.close(pred, ref['preds'][k], PASS_TOL, 'pass', f'pred{k}')
    if case.explicit:                                      # no loss kernel takes the output Sigmoid's derivative over
        model.forward(Xs)
        model.backward([CP.copy(g) for g in ref['Gs']])
        assert sorted(model.input_grads) == ([] if skip else list(inputs))
        for k in model.input_grads:
            worst.close(model.input_grads[k], ref['explicit_dxs'][k], GRAD_TOL, 'grad', f'explicit input_grad{k}')
        for pn, p in model.params().items():
            worst.close(p.grad, ref['explicit_grads'][pn], GRAD_TOL, 'grad', f'explicit grad {pn}')
    losses = model.compute_loss_and_gradients(Xs, ys)
    worst.close(losses_row(losses), ref['loss'], PASS_TOL, 'pass', 'loss')
    assert sorted(model.input_grads) == ([] if skip else list(inputs))
    for k in model.input_grads:
        worst.close(model.input_grads[k], ref['dxs'][k], GRAD_TOL, 'grad', f'input_grad{k}')
    assert sorted(model.params()) == sorted(ref['grads'])
    for pn, p in model.params().items():
        worst.close(p.grad, ref['grads'][pn], GRAD_TOL, 'grad', f'grad {pn}')
    model.clear_grads()
    rows = [losses_row(model.train(Xs, ys)) for _ in range(STEPS)]
    worst.close(np.array(rows), ref['step_losses'], STEP_TOL, 'step', 'step losses')
    for pn, p in model.params().items():
        worst.close(p.value, ref['stepped'][pn], STEP_TOL, 'step', f'stepped {pn}')
    print(f'{name}/{fusion}/{"skip" if skip else "full"}/{dt}: routes {sorted(routes_used(model)) or "fused only"}; ' +
          ', '.join(f'{kind} {err:.2e}' for kind, err in worst.seen.items()))
    assert not worst.failed, '; '.join(worst.failed)
    assert not model.nan_weights()
