"""What running a step leaves behind, checked on the host under the recording backend of tests/test_launch_trace.py
(no GPU): every net x every fusion setting x float32 / float16.

  * events: one train step reports exactly one 'forward' and one 'backward' event for every layer whose step produces
    a tensor (PLAIN, FUSED, PAIR -- under its second conv --, UP, WINDOWS), and none for an ALIAS or ABSORBED layer;
  * nothing is kept: after that step no layer has a non-empty `_mem` and no step holds an array, but for the 576 floats
    of per-phase weights that an UP step allocates once (`weff_buf`); after two forwards without a backward a step
    holds what the second one saved;
  * the layer classes have their own pass only: the fused variants and the state they parked on layers are gone.
"""
import numpy as np
import pytest

from test_launch_trace import FUSIONS, NETS, configure, recording

REMOVED = ('forward_fused', 'backward_fused', 'forward_up', 'backward_up', 'forward_pair', 'backward_pair',
           'forward_windows', 'backward_windows', '_fused_out', 'fused_activation', '_weff', '_weff_buf')
CASES = [(net, fusion, dtype) for net in NETS for fusion in FUSIONS for dtype in ('float32', 'float16')]


def make_net(net, fusion):
    """The net at the shapes of the launch traces, a tracker that records and prints nothing attached; its input and
    its label as device arrays."""
    from univer_ocr_amd.my_model.model import NET_MAKERS
    from univer_ocr_amd.nn import CP
    from univer_ocr_amd.nn.optimizers import Momentum
    from univer_ocr_amd.nn.progress_tracker import ProgressTracker
    shape = (2, 32, 64, 1) if net == 'Char' else (2, 16, 32, 1)
    model = configure(NET_MAKERS[net](shape, Momentum(lr=0.01, momentum=0.9)), FUSIONS[fusion], False)
    tracker = ProgressTracker(handler=lambda *a: None)
    model.init_progress_tracker(tracker)
    out_shape = model.get_output_shapes([shape])[0]
    return model, tracker, CP.copy(np.zeros(shape)), CP.copy(np.zeros(out_shape))


def arrays_of(step):
    from univer_ocr_amd.nn.gpu import DeviceArray
    return {name: value for name, value in vars(step).items() if isinstance(value, DeviceArray)}


@pytest.mark.parametrize('net,fusion,dtype', CASES)
def test_one_train_step_one_event_each_way_and_nothing_kept(net, fusion, dtype):
    from univer_ocr_amd.nn import plan
    with recording(dtype):
        model, tracker, X, y = make_net(net, fusion)
        model.train_begin([X], [y])
        model.train_finish()
        steps = model._compiled().steps
    assert sorted(step.node for step in steps) == sorted(model.layers)
    for step in steps:
        counts = {phase: event.counter for phase, event in tracker.layers[step.node].items()}
        if step.kind in (plan.ALIAS, plan.ABSORBED):
            assert counts == {}, (step.node, step.kind)
        else:
            assert counts == {'forward': 1, 'backward': 1}, (step.node, step.kind)
        assert set(arrays_of(step)) <= {'weff_buf'}, (step.node, step.kind)
    assert not {name: layer._mem for name, layer in model.layers.items() if layer._mem}


@pytest.mark.parametrize('net,fusion,dtype', CASES)
def test_a_second_forward_overwrites_what_the_first_saved(net, fusion, dtype):
    from univer_ocr_amd.nn import plan
    with recording(dtype):                                 # (the recorder keeps every array: no address comes back)
        model, _, X, _ = make_net(net, fusion)
        model.predict([X])
        first = dict(model.layers_outputs)
        model.predict([X])
        outputs = model.layers_outputs
        for step in model._compiled().steps:
            if step.kind not in (plan.FUSED, plan.PAIR, plan.UP, plan.WINDOWS):
                assert not arrays_of(step), (step.node, step.kind)
                continue
            source = step.sources[0]
            assert step.x is (X if isinstance(source, int) else outputs[source]), step.node
            assert step.y is outputs[step.node] and step.y is not first[step.node], step.node
            held = arrays_of(step)
            if 'weff_buf' in held:                         # float32, 4 -> 4 channels: borrowed until the backward
                assert step.kind == plan.UP and held.pop('weff') is held.pop('weff_buf')
            assert sorted(held) == ['x', 'y'], (step.node, held)


def test_the_layer_classes_have_their_own_pass_only():
    from univer_ocr_amd.nn.layers import Convolutional2D, FullyConnected
    with recording('float32'):
        for net in NETS:
            model, _, X, y = make_net(net, 'fused')
            model.train_begin([X], [y])
            model.train_finish()
            model.predict([X])
            for layer in list(model.layers.values()) + [Convolutional2D, FullyConnected]:
                assert not [name for name in REMOVED if hasattr(layer, name)], layer
