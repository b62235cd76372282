"""Runtime lanes on the device: a lane scope that is left by an exception, an option the library refuses, and one conv
launched on a lane against the same launch on the main lane, with the launch reports of both."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STRIDE, PADDING = (1, 1), (1, 1)


@pytest.fixture(scope='module')
def rt():
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    CP.set_dtype('float32')
    runtime = CP.runtime()
    return CP, runtime, runtime.add_lane(workspace_mb=16)          # the one extra lane of this module


@pytest.fixture(scope='module')
def conv(rt):
    CP = rt[0]
    rng = np.random.default_rng(41)
    return (CP.copy(rng.standard_normal((1, 4, 4, 1))), CP.copy(rng.standard_normal((3, 3, 1, 1))),
            CP.copy(rng.standard_normal(1)))


def test_an_exception_inside_a_lane_scope_restores_context_and_stream(rt):
    import torch
    _, runtime, index = rt
    current, stream = runtime.current, torch.cuda.current_stream()
    with pytest.raises(RuntimeError, match='inside the lane'):
        with runtime.lane(index) as lane_stream:
            assert runtime.current is runtime.lanes[index] and torch.cuda.current_stream() == lane_stream != stream
            raise RuntimeError('inside the lane')
    assert runtime.current is current and runtime.ctx is current.handle
    assert torch.cuda.current_stream() == stream


def test_a_refused_option_leaves_the_context_alone(rt):
    from univer_ocr_amd.hip import HipError
    _, runtime, _ = rt
    current = runtime.current
    with pytest.raises(HipError, match="unknown option 'no_such_option'"):
        runtime.set_option('no_such_option', 1)
    assert runtime.current is current and 'no_such_option' not in runtime._options


def test_a_conv_on_a_lane_equals_the_conv_on_the_main_lane(rt, conv):
    from univer_ocr_amd.nn import ops
    CP, runtime, index = rt
    x, w, b = conv
    on_main = ops.conv2d_fwd(x, w, b, STRIDE, PADDING)
    runtime.synchronize()                                          # x, w and b were copied on the main stream
    with runtime.lane(index):
        on_lane = ops.conv2d_fwd(x, w, b, STRIDE, PADDING)
        runtime.synchronize()
    got, expected = CP.asnumpy(on_lane), CP.asnumpy(on_main)
    assert got.shape == (1, 4, 4, 1) and np.any(expected != 0)
    assert got.tobytes() == expected.tobytes()


def test_launch_reports_belong_to_the_lane_of_the_launch(rt, conv):
    from univer_ocr_amd.nn import ops
    CP, runtime, index = rt
    x, w, b = conv
    ops.conv2d_fwd(x, w, b, STRIDE, PADDING)
    forward = runtime.last_conv()
    dy = CP.copy(np.ones((1, 4, 4, 1)))
    ops.conv2d_bwd_data(dy, w, x.shape, STRIDE, PADDING)
    main = runtime.last_conv()
    assert forward[0] == 0 and main[0] == 1 and forward[1] != 0 != main[1]
    runtime.synchronize()
    with runtime.lane(index):
        ops.conv2d_bwd_data(dy, w, x.shape, STRIDE, PADDING)
        assert runtime.last_conv() == main
        ops.conv2d_fwd(x, w, b, STRIDE, PADDING)
        assert runtime.last_conv() == forward                      # the lane reports its own latest launch
        runtime.synchronize()
    assert runtime.last_conv() == main                             # and the main lane still its own
