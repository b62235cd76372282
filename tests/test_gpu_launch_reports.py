"""The launch reports (uocr_ctx_last_*) as a whole: a new context reports zeros through every getter, a getter refuses a
null pointer in any position before it writes anything, and a launcher writes its own report and no other.  What each
report says about its launcher is checked where that launcher is tested."""
import ctypes as C

import numpy as np
import pytest

from test_host_logic import launch_report_getters

pytestmark = pytest.mark.gpu


def read_all(lib, hiplib, handle):
    """{getter: values} of context `handle`, every out pre-set to -1; every getter must return 0"""
    reports = {}
    for name in launch_report_getters():
        outs = [pointer._type_(-1) for pointer in hiplib._PROTOS[name][1:]]
        assert getattr(lib, name)(handle, *[C.byref(out) for out in outs]) == 0, name
        reports[name] = tuple(out.value for out in outs)
    return reports


def assert_all_zero(reports):
    assert len(reports) == 14
    for name, values in reports.items():
        assert values == (0,) * len(values), f'{name} of a new context: {values}'


def test_a_new_context_reports_zeros_and_null_pointers_are_refused():
    from univer_ocr_amd.hip import lib as hiplib
    lib = hiplib.get_lib()
    handle = C.c_void_p()
    assert lib.uocr_ctx_create(0, 0, C.byref(handle)) == 0
    try:
        assert_all_zero(read_all(lib, hiplib, handle))
        for name in launch_report_getters():
            types = [pointer._type_ for pointer in hiplib._PROTOS[name][1:]]
            for null in range(len(types)):
                outs = [t(-1) for t in types]
                args = [None if k == null else C.byref(out) for k, out in enumerate(outs)]
                assert getattr(lib, name)(handle, *args) != 0, f'{name}: null pointer {null} was accepted'
                assert all(out.value == -1 for out in outs), f'{name}: wrote before refusing null pointer {null}'
    finally:
        lib.uocr_ctx_destroy(handle)


def test_a_launcher_writes_its_own_report_only():
    from univer_ocr_amd.hip import lib as hiplib
    from univer_ocr_amd.nn import CP, ops
    CP.use_gpu(0)
    CP.set_dtype('float32')
    rt = CP.runtime()
    rng = np.random.default_rng(0)
    x, w, b = (CP.copy(rng.random(shape), np.float32) for shape in ((1, 4, 4, 1), (3, 3, 1, 1), (1,)))
    ops.conv2d_fwd(x, w, b, (1, 1), (1, 1))
    conv = rt.last_conv()
    assert conv[0] == 0 and conv[1] != 0
    ops.label_components(CP.copy(rng.random((1, 8, 8, 1)), np.float32))
    assert rt.last_conv() == conv, 'the labelling call changed the conv report'
    assert rt.last_label()[2] >= 1
    rt.call('uocr_stream_sync')
    handle = C.c_void_p()
    assert rt.lib.uocr_ctx_create(rt.device_index, 0, C.byref(handle)) == 0
    try:
        assert_all_zero(read_all(rt.lib, hiplib, handle))
    finally:
        rt.lib.uocr_ctx_destroy(handle)
