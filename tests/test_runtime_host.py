"""CPU tests of nn.gpu.Runtime's bookkeeping: which context a call goes to, the scoped switch `on`, options, deferred
weight-gradient groups, side streams and the context factory -- against a library that only records what it is asked."""
import ctypes as C
import types

import pytest

from univer_ocr_amd.hip import HipError
from univer_ocr_amd.nn import gpu
from univer_ocr_amd.nn.gpu import Lane, Runtime

CU_COUNT = 16                      # what the fake uocr_device_info reports
SET_STREAM, SET_OPTION = 'uocr_ctx_set_stream', 'uocr_ctx_set_option'


def plain(arg):
    if isinstance(arg, C.c_void_p):
        return arg.value
    if isinstance(arg, C.Array) and arg._type_ is not C.c_char:
        return list(arg)
    return '&' if isinstance(arg, C.Array) or hasattr(arg, '_obj') else arg       # (an out parameter: a buffer or byref)


class FakeLib:
    """Every uocr_* attribute is a function that records (name, context handle, arguments) in `calls` and returns 0, or
    the code that `fail_on` ordered for this call.  Contexts get the handles 1, 2, 3, ..., events 101, 102, ..."""

    def __init__(self):
        self.calls, self.failing, self.failed = [], {}, None
        self.contexts, self.events = 0, 100

    def fail_on(self, name, nth=1, code=-7):
        """the nth call of `name` from now on returns `code`"""
        self.failing[name] = [nth, code]

    def names(self):
        return [name for name, _, _ in self.calls]

    def __getattr__(self, name):
        if not name.startswith('uocr_'):
            raise AttributeError(name)
        return lambda *args: self.called(name, args)

    def called(self, name, args):
        if name == 'uocr_last_error':
            return f'the fake refused {self.failed}'.encode()
        if name == 'uocr_event_destroy':                  # (whenever an Event is collected: not part of any sequence)
            return 0
        if name == 'uocr_ctx_get_stream':
            return 0x2000 + args[0].value
        if name in self.failing:
            self.failing[name][0] -= 1
            if self.failing[name][0] == 0:
                self.failed = name
                self.calls.append((name + ' FAILED', None, ()))
                return self.failing.pop(name)[1]
        if name in ('uocr_ctx_create', 'uocr_ctx_create_cu_mask'):
            self.contexts += 1
            args[-1]._obj.value = self.contexts
            self.calls.append((name, None, tuple(plain(a) for a in args[:-1])))
        elif name == 'uocr_event_create':
            self.events += 1
            args[0]._obj.value = self.events
            self.calls.append((name, None, ()))
        else:
            if name == 'uocr_device_info':
                args[3]._obj.value = CU_COUNT
            self.calls.append((name, args[0].value, tuple(plain(a) for a in args[1:])))
        return 0


@pytest.fixture
def rt():
    """A Runtime without a device: the state initialiser on a bare object, streams from a counter, the main context made
    by the factory as Runtime.__init__ makes it (handle 1, stream 0x1001)."""
    runtime = object.__new__(Runtime)
    runtime.device_index, runtime.device, made = 0, 'no device', []

    def stream(priority=0, external=None):
        made.append((priority, external))
        return types.SimpleNamespace(cuda_stream=0x1000 + len(made) if external is None else external)
    runtime._stream, runtime.streams_made = stream, made
    main = Lane(stream())
    runtime._init_state(FakeLib(), main)
    runtime._open(main, 'main context', 1 << 20)
    assert runtime.lib.calls == [('uocr_ctx_create', None, (0, 1 << 20)), (SET_STREAM, 1, (0x1001,))]
    assert runtime.current is main and runtime.lanes == [main] and runtime.ctx is main.handle
    assert main.handle.value == 1 and runtime.launches == 1
    del runtime.lib.calls[:]
    return runtime


# ---- call ----------------------------------------------------------------------------------------------------------
def test_calls_go_to_the_current_handle_and_are_counted(rt):
    before = rt.launches
    rt.call('uocr_memset_zero', 0x50, 64)
    lane = rt.lanes[rt.add_lane()]
    with rt.on(lane):
        rt.call('uocr_fill', 1, 0x60, 2.0, 8)
        assert rt.ctx is lane.handle
    rt.call('uocr_stream_sync')
    sent = [c for c in rt.lib.calls if c[0] in ('uocr_memset_zero', 'uocr_fill', 'uocr_stream_sync')]
    assert sent == [('uocr_memset_zero', 1, (0x50, 64)), ('uocr_fill', 2, (1, 0x60, 2.0, 8)), ('uocr_stream_sync', 1, ())]
    assert rt.launches == before + 4                       # (the three and the lane's uocr_ctx_set_stream)


def test_a_nonzero_code_raises_with_the_librarys_message(rt):
    rt.lib.fail_on('uocr_fill', code=-4)
    with pytest.raises(HipError, match=r'uocr_fill failed \(-4\): the fake refused uocr_fill'):
        rt.call('uocr_fill', 1, 0x60, 2.0, 8)
    assert rt.launches == 2                                # a refused call counts too, as it always did
    rt.call('uocr_fill', 1, 0x60, 2.0, 8)


# ---- on ------------------------------------------------------------------------------------------------------------
def test_on_restores_the_previous_context_on_every_exit(rt):
    main, a, b = rt.lanes[0], Lane(None, C.c_void_p(7)), Lane(None, C.c_void_p(8))
    with rt.on(a) as entered:
        assert entered is a and rt.current is a and rt.ctx is a.handle
    assert rt.current is main
    with pytest.raises(RuntimeError, match='inside'):
        with rt.on(a):
            raise RuntimeError('inside')
    assert rt.current is main
    with rt.on(a):
        with rt.on(b):
            assert rt.current is b
            with pytest.raises(KeyError):
                with rt.on(main):
                    raise KeyError('nested')
            assert rt.current is b
        assert rt.current is a
    assert rt.current is main and rt.ctx is main.handle


def test_ctx_cannot_be_assigned(rt):
    with pytest.raises(AttributeError):
        setattr(rt, 'ctx', C.c_void_p(9))


# ---- options -------------------------------------------------------------------------------------------------------
def test_set_option_goes_to_every_lane_then_to_every_side_stream(rt):
    first, second = rt.add_lane(), rt.add_lane()
    rt.side_on = True
    with rt.on(rt.lanes[second]), rt.side():
        pass
    with rt.side():
        pass
    sides = (rt.lanes[second].side.handle.value, rt.lanes[0].side.handle.value)
    assert sides == (4, 5) and rt.lanes[first].side is None
    del rt.lib.calls[:]
    rt.set_option('mfma', 2.0)
    assert rt.lib.calls == [(SET_OPTION, h, (b'mfma', 2)) for h in (1, 2, 3, 5, 4)]      # lanes in order, then their sides
    assert rt._options == {'mfma': 2} and rt.current is rt.lanes[0]


def test_set_option_that_fails_restores_the_context_and_records_nothing(rt):
    rt.add_lane()
    rt.set_option('fast_paths', 0)
    del rt.lib.calls[:]
    rt.lib.fail_on(SET_OPTION, nth=2, code=-2)
    with pytest.raises(HipError, match=r'uocr_ctx_set_option failed \(-2\)'):
        rt.set_option('mfma', 2)
    assert rt.lib.names() == [SET_OPTION, SET_OPTION + ' FAILED']
    assert rt.current is rt.lanes[0] and rt._options == {'fast_paths': 0}


def test_a_lane_made_later_starts_from_the_librarys_defaults(rt):
    rt.set_option('mfma', 2)
    del rt.lib.calls[:]
    index = rt.add_lane(workspace_mb=3, priority=-1)
    assert index == 1 and rt.streams_made[-1] == (-1, None)
    assert rt.lib.calls == [('uocr_ctx_create', None, (0, 3 << 20)), (SET_STREAM, 2, (rt.lanes[1].stream.cuda_stream,))]


# ---- deferred weight gradients -------------------------------------------------------------------------------------
def test_defer_wgrad_brackets_the_block_and_holds_arrays_of_its_lane_only(rt):
    other = rt.lanes[rt.add_lane()]
    rt.side_on = True
    del rt.lib.calls[:]
    rt.keep('before')                                       # no group is open: nothing is held
    assert rt.current.held is None
    with rt.defer_wgrad():
        assert rt.lib.calls == [('uocr_wgrad_defer_begin', 1, ())]
        held = rt.current.held
        rt.keep('x', 'dy')
        assert held == ['x', 'dy']
        with rt.on(other):
            rt.keep('on another lane')
            rt.flush_deferred()                             # no group there: no call
        with rt.side():
            rt.keep('inside a side scope')
        assert held == ['x', 'dy'] and other.held is None and rt.current.side.held is None
        with pytest.raises(HipError, match='already open on this lane'):
            with rt.defer_wgrad():
                pass
        assert rt.current.held is held
        with rt.on(other), rt.defer_wgrad():                # another lane may have a group of its own
            rt.keep('theirs')
            assert other.held == ['theirs'] and held == ['x', 'dy']
        del rt.lib.calls[:]
        rt.flush_deferred()
        assert rt.lib.calls == [('uocr_wgrad_defer_flush', 1, (1,))] and held == [] and rt.current.held is held
        rt.keep('later')                                    # still recording
        assert held == ['later']
    assert rt.lib.calls[1:] == [('uocr_wgrad_defer_flush', 1, (0,))] and held == [] and rt.current.held is None
    del rt.lib.calls[:]
    rt.flush_deferred()
    assert rt.lib.calls == []
    with rt.defer_wgrad():                                  # and a new group can be opened
        pass
    assert rt.lib.names() == ['uocr_wgrad_defer_begin', 'uocr_wgrad_defer_flush']


def test_a_failing_last_flush_is_swallowed_only_under_another_exception(rt):
    rt.lib.fail_on('uocr_wgrad_defer_flush')
    with pytest.raises(HipError, match='uocr_wgrad_defer_flush failed'):
        with rt.defer_wgrad():
            rt.keep('x')
    assert rt.current.held is None
    rt.lib.fail_on('uocr_wgrad_defer_flush')
    with pytest.raises(ValueError, match='the block'):
        with rt.defer_wgrad():
            raise ValueError('the block')
    assert rt.current.held is None and rt.lib.names()[-1] == 'uocr_wgrad_defer_flush FAILED'
    rt.lib.fail_on('uocr_wgrad_defer_begin')
    with pytest.raises(HipError, match='uocr_wgrad_defer_begin failed'):
        with rt.defer_wgrad():
            raise AssertionError('entered')
    assert rt.current.held is None


# ---- side streams --------------------------------------------------------------------------------------------------
def test_side_is_a_no_op_unless_side_on(rt):
    with rt.side('x'):
        rt.call('uocr_stream_sync')
    assert rt.lib.calls == [('uocr_stream_sync', 1, ())] and rt.current.side is None
    rt.join_side()
    assert len(rt.lib.calls) == 1


def test_side_fork_and_join_call_by_call(rt):
    lane = rt.lanes[rt.add_lane()]
    rt.set_option('mfma', 2)
    rt.set_option('fast_paths', 0)
    rt.set_option('mfma', 1)                               # replayed where it was first set: insertion order
    rt.side_on = True
    del rt.lib.calls[:]
    with rt.on(lane):
        with rt.side('x', 'dy'):
            side = lane.side
            assert rt.current is side and side.handle.value == 3 and side.keep == ['x', 'dy'] and side.dirty
            rt.call('uocr_conv2d_bwd_weight')
        assert rt.current is lane
        fork, join = side.fork_ev.handle.value, side.join_ev.handle.value
        assert (fork, join) == (101, 102)
        assert rt.lib.calls == [
            ('uocr_event_create', None, ()), ('uocr_event_create', None, ()),
            ('uocr_ctx_create', None, (0, 128 << 20)),
            (SET_STREAM, 3, (side.stream.cuda_stream,)),
            (SET_OPTION, 3, (b'mfma', 1)), (SET_OPTION, 3, (b'fast_paths', 0)),
            ('uocr_event_record', 2, (fork,)), ('uocr_stream_wait_event', 3, (fork,)),
            ('uocr_conv2d_bwd_weight', 3, ())]
        del rt.lib.calls[:]
        with rt.side('x2'):                                # the second entry forks again on the side it has
            pass
        assert lane.side is side and side.keep == ['x', 'dy', 'x2']
        assert rt.lib.calls == [('uocr_event_record', 2, (fork,)), ('uocr_stream_wait_event', 3, (fork,))]
        del rt.lib.calls[:]
    rt.join_side()                                         # the main lane has no side: no call
    assert rt.lib.calls == []
    with rt.on(lane):
        rt.join_side()
        assert rt.lib.calls == [('uocr_event_record', 3, (join,)), ('uocr_stream_wait_event', 2, (join,))]
        assert side.keep == [] and not side.dirty and rt.current is lane
        rt.join_side()                                     # not dirty any more: no call
        assert len(rt.lib.calls) == 2


def test_side_workspace_follows_the_environment(rt, monkeypatch):
    monkeypatch.setenv('UOCR_SIDE_WORKSPACE_MB', '5')
    rt.side_on = True
    with rt.side():
        pass
    assert ('uocr_ctx_create', None, (0, 5 << 20)) in rt.lib.calls


def test_side_scope_restores_the_lane_when_the_block_raises(rt):
    rt.side_on = True
    with pytest.raises(RuntimeError, match='kernel failed'):
        with rt.side('x'):
            raise RuntimeError('kernel failed')
    assert rt.current is rt.lanes[0] and rt.current.side.dirty


def test_a_failing_join_restores_the_lane(rt):
    rt.side_on = True
    with rt.side('x'):
        pass
    rt.lib.fail_on('uocr_event_record')
    with pytest.raises(HipError, match='uocr_event_record failed'):
        rt.join_side()
    assert rt.current is rt.lanes[0] and rt.current.side.dirty and rt.current.side.keep == ['x']


def test_a_capture_joins_the_side_before_it_ends(rt):
    rt.side_on = True
    with rt.side('x'):
        pass
    del rt.lib.calls[:]
    capture = gpu._Capture(rt, None)
    capture._mem, capture.graph = None, gpu.Graph(rt, None, None)
    capture.__exit__(None, None, None)
    assert rt.lib.names() == ['uocr_event_record', 'uocr_stream_wait_event', 'uocr_graph_end_capture']
    assert [handle for _, handle, _ in rt.lib.calls] == [2, 1, 1]


# ---- the context factory -------------------------------------------------------------------------------------------
def test_a_lane_whose_stream_cannot_be_bound_is_destroyed(rt):
    rt.lib.fail_on(SET_STREAM, code=-3)
    with pytest.raises(HipError, match=r'^lane: uocr_ctx_set_stream failed \(-3\): the fake refused'):
        rt.add_lane()
    assert rt.lib.calls[-1] == ('uocr_ctx_destroy', 2, ())
    assert rt.current is rt.lanes[0] and len(rt.lanes) == 1 and rt.ctx is rt.lanes[0].handle


def test_a_side_stream_whose_set_up_fails_is_destroyed(rt):
    rt.set_option('mfma', 2)
    rt.side_on = True
    for failing in (SET_STREAM, SET_OPTION):
        rt.lib.fail_on(failing)
        with pytest.raises(HipError, match=f'^side stream: {failing} failed'):
            with rt.side('x'):
                raise AssertionError('entered')
        assert rt.lib.calls[-1][0] == 'uocr_ctx_destroy' and rt.lib.calls[-1][1] == rt.lib.contexts
        assert rt.current is rt.lanes[0] and rt.current.side is None
    with rt.side('x'):                                     # and the next use makes one
        assert rt.current is rt.lanes[0].side


def test_a_context_that_cannot_be_created_names_what_it_was(rt):
    for name, make, what in (('uocr_ctx_create', rt.add_lane, r'\(lane\)'),
                             ('uocr_ctx_create_cu_mask', lambda: rt.add_lane(xcds=(2,)), r'\(lane on XCDs \[2\]\)')):
        rt.lib.fail_on(name, code=-5)
        with pytest.raises(HipError, match=f'{what} failed with code -5'):
            make()
    rt.side_on = True
    rt.lib.fail_on('uocr_ctx_create', code=-5)
    with pytest.raises(HipError, match=r'\(side stream\) failed with code -5'):
        rt.side().__enter__()
    assert 'uocr_ctx_destroy' not in rt.lib.names() and len(rt.lanes) == 1 and rt.current is rt.lanes[0]


def test_a_lane_on_xcds_gets_the_cu_mask_and_the_librarys_stream(rt):
    index = rt.add_lane(workspace_mb=2, xcds=[1, 0, 1])
    lane = rt.lanes[index]
    mask = sum(1 << cu for cu in range(CU_COUNT) if cu % 8 in (0, 1))
    assert rt.lib.calls == [('uocr_device_info', 1, ('&', 256, '&', '&')),
                            ('uocr_ctx_create_cu_mask', None, (0, 2 << 20, [mask], 1))]
    assert rt.streams_made[-1] == (0, 0x2000 + 2) and lane.stream.cuda_stream == 0x2002 and lane.handle.value == 2
    assert rt.current is rt.lanes[0]
