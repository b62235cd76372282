"""The host executor's sequence of C-ABI calls, recorded without a GPU and compared with tests/launch_traces.json.

`CP._runtime` is replaced by a recorder whose `call(name, *args)` notes the call instead of launching it; arrays are
then host storage and every nn/ops.py wrapper still reaches `call`.  A trace holds, per call, the entry-point name,
every scalar exactly and every pointer as [ordinal of the allocation it lies in, byte offset] (None for null); a
`bucket_hook(model, node)` call is the entry ['bucket_hook', node] at the place where it happened.  Beside each trace:
which `layers_outputs` keys are None and which share one array.

The ordinal counts, in the order of their allocation, the allocations that the calls of one phase (predict, test,
train, forward + backward) name.  Which arguments share a buffer, in one call and from call to call, is all there, and
so is which of two buffers is the older one (the inputs and parameters among themselves, they before the outputs of
the first layer, and so on): an exchange of two buffers shows.  How many arrays a model allocates while it is built,
and in the phases before, is not there, so that the same launch is the same entry in most cases.

Traced: every net x every fusion setting x skip_input_grads off / on x float32 / float64 / float16, and three
hand-built graphs.

launch_traces.json is this project's own recorded output, written by

    python tests/test_launch_trace.py --write

It pins the executor (nn/models.py): a change there that is meant to leave behaviour alone must pass against the
file as it is; only a change that is meant to alter the launch sequence regenerates it.
"""
import bisect
import contextlib
import ctypes
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
EXPECTED = os.path.join(ROOT, 'tests', 'launch_traces.json')

NETS = ('Monochrome', 'Paragraph', 'Line', 'Char')
FUSIONS = {'unfused': None, 'fused': {}, 'fused_nopairs': {'pairs': False}, 'fused_nowindows': {'windows': False}}
DTYPES = ('float32', 'float64', 'float16')


class Recorder:
    """Stands where gpu.Runtime stands: the part of its interface that nn/ops.py and nn/models.py use."""
    device = torch.device('cpu')
    side_on = False

    def __init__(self):
        self.trace = []
        self.bases, self.spans, self.kept = [], {}, []     # sorted base addresses; base -> (index in kept, bytes)
        self.named = []                                    # the pointer entries of the trace: [index in kept, offset]

    def register(self, array):
        """An array handed out by CP.empty / CP.copy: kept until the case ends, so that no address is reused."""
        self.kept.append(array)
        if array.nbytes:
            assert array.ptr not in self.spans
            self.spans[array.ptr] = (len(self.kept) - 1, array.nbytes)
            bisect.insort(self.bases, array.ptr)
        return array

    def name_pointer(self, address):
        if address is None:
            return None
        at = bisect.bisect_right(self.bases, address) - 1
        if at >= 0:
            index, nbytes = self.spans[self.bases[at]]
            if address < self.bases[at] + nbytes:
                self.named.append([index, address - self.bases[at]])
                return self.named[-1]
        raise AssertionError(f'pointer {address:#x} lies in no array handed out by CP.empty / CP.copy')

    def call(self, name, *args):
        from univer_ocr_amd.hip import lib as hiplib
        kinds = hiplib._PROTOS[name][1:]                   # (the context comes first)
        assert len(kinds) == len(args), f'{name}: {len(args)} arguments for {len(kinds)} parameters'
        entry = [name]
        for kind, arg in zip(kinds, args):
            if kind is ctypes.c_void_p:
                entry.append(self.name_pointer(arg))
            elif isinstance(arg, ctypes.Array):
                entry.append(list(arg))
            else:
                assert arg is None or type(arg) in (int, float), f'{name}: argument {arg!r}'
                entry.append(arg)
        self.trace.append(entry)

    def keep(self, *arrays):
        pass

    def side(self, *keep):
        return contextlib.nullcontext()

    def take(self):
        """The calls since the last take, the allocations that they name numbered in the order of their allocation."""
        ordinals = {index: ordinal for ordinal, index in enumerate(sorted({index for index, _ in self.named}))}
        for pointer in self.named:
            pointer[0] = ordinals[pointer[0]]
        trace, self.trace, self.named = self.trace, [], []
        return trace


@contextlib.contextmanager
def recording(dtype):
    from univer_ocr_amd.nn import CP
    rec = Recorder()
    empty, copy = CP.empty, CP.copy
    # the backend as it is on a machine without a GPU, whatever this machine has and earlier tests left behind
    during = {'_runtime': rec, 'dtype': np.dtype(dtype), 'has_device': staticmethod(lambda: False),
              'lazy_losses': False, 'loss_arena': None, 'f16_grad_scale_log2': None,
              'empty': staticmethod(lambda *a, **k: rec.register(empty(*a, **k))),
              'copy': staticmethod(lambda *a, **k: rec.register(copy(*a, **k)))}
    saved = {name: CP.__dict__[name] for name in during}
    for name, value in during.items():
        setattr(CP, name, value)
    try:
        yield rec
    finally:
        for name, value in saved.items():
            setattr(CP, name, value)


def outputs_of(model):
    """`layers_outputs` of the last forward: the keys that are None, and the groups of keys that are one array."""
    groups = {}
    for key, value in model.layers_outputs.items():
        if value is not None:
            groups.setdefault(id(value), []).append(str(key))
    return {'keys': [str(k) for k in model.layers_outputs],
            'none': [str(k) for k, v in model.layers_outputs.items() if v is None],
            'shared': sorted(g for g in groups.values() if len(g) > 1)}


def run_phases(rec, model, Xs, ys):
    """predict, test, train_begin + train_finish, and forward + backward(grads): the path without loss folding."""
    from univer_ocr_amd.nn import CP
    Xs, ys = [CP.copy(x) for x in Xs], [CP.copy(y) for y in ys]
    model.bucket_hook = lambda _model, node: rec.trace.append(['bucket_hook', node])
    rec.take()                                             # (what building the model launched is not the executor's)
    phases = {}
    model.predict(Xs)
    phases['predict'] = {'calls': rec.take(), 'outputs': outputs_of(model)}
    model.test(Xs, ys)
    phases['test'] = {'calls': rec.take(), 'outputs': outputs_of(model)}
    model.train_begin(Xs, ys)
    model.train_finish()
    phases['train'] = {'calls': rec.take(), 'outputs': outputs_of(model), 'input_grads': sorted(model.input_grads)}
    predicted = model.forward(Xs)
    model.backward([np.ones(p.shape) for p in predicted])
    phases['forward_backward'] = {'calls': rec.take(), 'outputs': outputs_of(model),
                                  'input_grads': sorted(model.input_grads)}
    return phases


def configure(model, fusion, skip):
    if fusion is not None:
        model.enable_fusion(True, **fusion)
    if skip:
        model.skip_input_grads()
    return model


def trace_net(net, fusion, skip, dtype):
    from univer_ocr_amd.my_model.model import NET_MAKERS
    from univer_ocr_amd.nn.optimizers import Momentum
    with recording(dtype) as rec:
        shape = (2, 32, 64, 1) if net == 'Char' else (2, 16, 32, 1)
        model = configure(NET_MAKERS[net](shape, Momentum(lr=0.01, momentum=0.9)), FUSIONS[fusion], skip)
        out_shape = model.get_output_shapes([shape])[0]
        return run_phases(rec, model, [np.zeros(shape)], [np.zeros(out_shape)])


def make_narrow_windows():
    """Windows + flatten + dense behind an 8-channel feature map: the dense layer's sizes suit the implicit GEMM, the
    channel count does not, so the fused graph runs these three layers one by one."""
    from univer_ocr_amd.nn.layers import (Conv2DToBatchedFixedWidthed, Convolutional2D, Flatten, FullyConnected,
                                          LeakyRelu)
    from univer_ocr_amd.nn.models import Sequential
    from univer_ocr_amd.nn.optimizers import Momentum
    opt = Momentum(lr=0.01, momentum=0.9)
    model = Sequential([Convolutional2D((3, 3), out_channels=8, padding=1, optimizer=opt), LeakyRelu(0.01),
                        Conv2DToBatchedFixedWidthed(8), Flatten(), FullyConnected(n_output=32, optimizer=opt),
                        LeakyRelu(0.01), FullyConnected(n_output=5, optimizer=opt)])
    shape = (2, 4, 16, 1)
    model.initialize([shape])
    return model, [np.zeros(shape)], [np.zeros((32, 5))]


def make_nested():
    """tests/golden/graph_models.npz 'nested': Sequential sub-models, both inputs consumed twice."""
    from univer_ocr_amd.nn.layers import Concat, Convolutional2D, LeakyRelu, MaxPool2D
    from univer_ocr_amd.nn.losses import SegmentationDice2D
    from univer_ocr_amd.nn.models import Model, Sequential
    from univer_ocr_amd.nn.regularizations import L1, L2

    def sub(out_ch):
        return Sequential([Convolutional2D((2, 2), out_channels=out_ch, regularizer=L2(0.1)), LeakyRelu(0.01),
                           Convolutional2D((2, 2), out_channels=out_ch, regularizer=L1(0.1)), MaxPool2D((2, 2))])
    layers = {'row_1': sub(2), 'row_2': sub(3), 'concat_rows': Concat(), 'concat_inputs': Concat(),
              'row_inputs': sub(2), 'concat_all': Concat(), 'pool_1': MaxPool2D((2, 2)),
              'pool_2': MaxPool2D((2, 2)), 'conv_end': Convolutional2D((2, 2), out_channels=3)}
    relations = {'row_1': 0, 'row_2': 1, 'concat_rows': ['row_1', 'row_2'], 'concat_inputs': [0, 1],
                 'row_inputs': 'concat_inputs', 'concat_all': ['concat_rows', 'row_inputs'],
                 'pool_1': 'concat_all', 'pool_2': 'pool_1', 'conv_end': 'pool_2', 0: 'conv_end'}
    model = Model(layers, relations, loss=SegmentationDice2D())
    shapes = [(3, 18, 18, 3)] * 2
    model.initialize(shapes)
    return model, [np.zeros(s) for s in shapes], [np.zeros((3, 1, 1, 3))]


def make_dag():
    """tests/golden/graph_models.npz 'dag' with activations: a LeakyRelu consumed by an output AND by a layer (its
    gradients are summed), and one consumed by a single dense layer (its gradient folds into that layer's dx)."""
    from univer_ocr_amd.nn.layers import Concat, Convolutional2D, Flatten, FullyConnected, LeakyRelu, MaxPool2D
    from univer_ocr_amd.nn.losses import SigmoidCrossEntropy
    from univer_ocr_amd.nn.models import Model
    layers = {'conv1': Convolutional2D((2, 2), out_channels=3), 'act1': LeakyRelu(0.01),
              'conv2': Convolutional2D((2, 2), out_channels=3), 'conv3': Convolutional2D((2, 2), out_channels=3),
              'concat': Concat(), 'pool': MaxPool2D(2), 'flatten': Flatten(), 'dense1': FullyConnected(n_output=3),
              'act_d1': LeakyRelu(0.01), 'dense2': FullyConnected(n_output=3), 'act_d2': LeakyRelu(0.01),
              'dense3': FullyConnected(n_output=3)}
    relations = {'conv1': 0, 'act1': 'conv1', 'conv2': 1, 'conv3': 2, 'concat': ['act1', 'conv2', 'conv3'],
                 'pool': 'concat', 'flatten': 'pool', 'dense1': 'flatten', 'act_d1': 'dense1', 'dense2': 'act_d1',
                 'act_d2': 'dense2', 'dense3': 'act_d2', 0: 'act_d1', 1: 'dense3'}
    model = Model(layers, relations, loss=SigmoidCrossEntropy())
    shapes = [(2, 5, 5, 2)] * 3
    model.initialize(shapes)
    return model, [np.zeros(s) for s in shapes], [np.zeros((2, 3))] * 2


HAND_BUILT = {'narrow_windows': make_narrow_windows, 'nested': make_nested, 'dag': make_dag}


def trace_hand_built(graph, fusion, skip):
    with recording('float32') as rec:
        model, Xs, ys = HAND_BUILT[graph]()
        return run_phases(rec, configure(model, FUSIONS[fusion], skip), Xs, ys)


def net_cases():
    return [f'{net}-{fusion}-{"skip" if skip else "full"}-{dtype}'
            for net, fusion, skip, dtype in itertools.product(NETS, FUSIONS, (False, True), DTYPES)]


def hand_built_cases():
    return [f'{graph}-{setting}' for graph in HAND_BUILT for setting in ('unfused-full', 'fused-full', 'fused-skip')]


def trace_case(case):
    parts = case.split('-')
    if parts[0] in HAND_BUILT:
        return trace_hand_built(parts[0], parts[1], parts[2] == 'skip')
    return trace_net(parts[0], parts[1], parts[2] == 'skip', parts[3])


def pack(traces):
    """The file's form: every distinct call, `layers_outputs` record and phase once, in order of first appearance, and
    below them indices into these lists (the same launch recurs in most cases, the same phase in many)."""
    tables = {'calls': ({}, []), 'outputs': ({}, []), 'phases': ({}, [])}

    def index(table, entry):
        seen, entries = tables[table]
        key = json.dumps(entry, sort_keys=True)
        if key not in seen:
            seen[key] = len(entries)
            entries.append(entry)
        return seen[key]
    cases = {case: {phase: index('phases', dict(rec, calls=[index('calls', e) for e in rec['calls']],
                                                outputs=index('outputs', rec['outputs'])))
                    for phase, rec in phases.items()} for case, phases in traces.items()}
    return dict({table: entries for table, (_, entries) in tables.items()}, cases=cases)


def unpack(packed, case):
    phases = {phase: packed['phases'][i] for phase, i in packed['cases'][case].items()}
    return {phase: dict(rec, calls=[packed['calls'][i] for i in rec['calls']],
                        outputs=packed['outputs'][rec['outputs']]) for phase, rec in phases.items()}


def write(packed, f):
    """One entry of each list, and one case, per line."""
    def compact(value):
        return json.dumps(value, separators=(',', ':'), sort_keys=True)
    parts = [f'"{table}":[\n' + ',\n'.join(map(compact, packed[table])) + '\n]'
             for table in ('calls', 'outputs', 'phases')]
    parts.append('"cases":{\n' + ',\n'.join(f'"{case}":{compact(packed["cases"][case])}'
                                            for case in sorted(packed['cases'])) + '\n}')
    f.write('{' + ',\n'.join(parts) + '}\n')


@pytest.fixture(scope='module')
def expected():
    with open(EXPECTED) as f:
        return json.load(f)


def test_every_case_is_in_the_file(expected):
    assert sorted(expected['cases']) == sorted(net_cases() + hand_built_cases())


@pytest.mark.parametrize('case', net_cases() + hand_built_cases())
def test_launch_trace(case, expected):
    got = json.loads(json.dumps(trace_case(case)))         # (tuples -> lists, as the file has them)
    want = unpack(expected, case)
    for phase in want:
        assert got[phase]['outputs'] == want[phase]['outputs'], phase
        assert got[phase].get('input_grads') == want[phase].get('input_grads'), phase
        for i, (a, b) in enumerate(zip(got[phase]['calls'], want[phase]['calls'])):
            assert a == b, f'{phase}: call {i}'
        assert len(got[phase]['calls']) == len(want[phase]['calls']), phase
    assert sorted(got) == sorted(want)


def test_traces_show_what_they_are_meant_to(expected):
    """The recorded file covers the paths it was recorded for (a guard against a generator that went blind)."""
    def names(case, phase):
        return [e[0] for e in unpack(expected, case)[phase]['calls'] if e[0] != 'bucket_hook']
    assert names('Monochrome-fused-full-float32', 'train')[:3] == ['uocr_conv_pair_fwd', 'uocr_seg_loss',
                                                                   'uocr_conv_pair_bwd']
    assert 'uocr_conv_pair_fwd' not in names('Monochrome-fused_nopairs-full-float32', 'train')
    assert 'uocr_upconv2x_fwd' in names('Line-fused-full-float32', 'predict')
    assert 'uocr_upconv2x_fwd' not in names('Line-fused-full-float64', 'predict')
    assert 'uocr_fixed_width_fwd' not in names('Char-fused-full-float32', 'predict')
    assert 'uocr_fixed_width_fwd' in names('Char-fused_nowindows-full-float32', 'predict')
    assert 'uocr_fixed_width_fwd' in names('narrow_windows-fused-full', 'predict')
    assert 'uocr_dense_fwd_act' in names('narrow_windows-fused-full', 'predict')
    for graph in ('nested', 'dag'):
        assert 'uocr_add' in names(f'{graph}-fused-full', 'forward_backward')
    assert unpack(expected, 'Line-fused-skip-float32')['train']['input_grads'] == []
    outputs = unpack(expected, 'Monochrome-fused-full-float32')['predict']['outputs']
    assert len(outputs['none']) == 2 and len(outputs['shared']) == 1


# -- the step list is compiled once ------------------------------------------------------------------------------
@pytest.fixture
def compile_counter(monkeypatch):
    from univer_ocr_amd.nn import plan
    calls = []
    inner = plan.compile_steps

    def counting(*args, **kwargs):
        calls.append(1)
        return inner(*args, **kwargs)
    monkeypatch.setattr(plan, 'compile_steps', counting)
    return calls


def test_step_list_is_built_once(compile_counter):
    from univer_ocr_amd.my_model.model import make_line
    with recording('float32'):
        model = make_line((2, 16, 32, 1)).enable_fusion()
        X, y = np.zeros((2, 16, 32, 1)), np.zeros((2, 16, 32, 2))
        for _ in range(3):
            model.forward([X])
        for _ in range(2):
            model.train_begin(X, y)
        model.train_finish()
    assert len(compile_counter) == 1


def test_step_list_is_rebuilt_after_a_change_of_the_graph(compile_counter):
    from univer_ocr_amd.my_model.model import make_line
    with recording('float32'):
        model = make_line((2, 16, 32, 1))
        X = np.zeros((2, 16, 32, 1))
        model.forward([X])
        assert len(compile_counter) == 1
        for n, change in enumerate([lambda: model.enable_fusion(), lambda: model.skip_input_grads(),
                                    lambda: model.initialize([(2, 16, 32, 1)])], 2):
            change()
            assert len(compile_counter) == n - 1               # dropped, not rebuilt, by the change itself
            model.forward([X])
            model.forward([X])
            assert len(compile_counter) == n


if __name__ == '__main__':
    if sys.argv[1:] != ['--write']:
        sys.exit('usage: python tests/test_launch_trace.py --write')
    packed = pack({case: trace_case(case) for case in net_cases() + hand_built_cases()})
    with open(EXPECTED, 'w') as f:
        write(packed, f)
    print(f'{EXPECTED}: {len(packed["cases"])} cases, {len(packed["calls"])} distinct calls, '
          f'{os.path.getsize(EXPECTED)} bytes')
