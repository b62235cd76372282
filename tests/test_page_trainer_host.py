"""CPU tests of PageTrainer's host logic: the hooks taken off for a graph capture come back on every way out, the
side_wgrad / group_wgrad options select the nets they always did, and the page context mapping exists once."""
import contextlib
import types

import pytest

from univer_ocr_amd.my_model import model as page_model
from univer_ocr_amd.my_model import trainer as page_trainer

NETS = ('Monochrome', 'Paragraph', 'Line', 'Char')


def test_collectives_off_restores_the_hooks_on_every_exit():
    def sync(model):
        pass

    def hook(model, node):
        pass
    net = types.SimpleNamespace(grad_sync=sync, bucket_hook=hook)
    with page_trainer._collectives_off(net):
        assert net.grad_sync is None and net.bucket_hook is None
    assert net.grad_sync is sync and net.bucket_hook is hook
    with pytest.raises(RuntimeError, match='capture failed'):
        with page_trainer._collectives_off(net):
            net.bucket_hook = lambda model, node: None         # (the capture installs its cut here)
            raise RuntimeError('capture failed')
    assert net.grad_sync is sync and net.bucket_hook is hook


class RecordingRuntime:
    """Stand-in for nn.gpu.Runtime: logs what a capture does instead of doing it."""

    def __init__(self):
        self.log = []

    @contextlib.contextmanager
    def capture(self, pool):
        graph = f'graph {sum(entry == "begin" for entry in self.log)}'
        self.log.append('begin')
        try:
            yield graph
        finally:
            self.log.append('end')

    def flush_deferred(self):
        self.log.append('flush')


def test_cut_capture_closes_one_graph_before_it_opens_the_next():
    rt = RecordingRuntime()
    with page_trainer._CutCapture(rt, pool=None) as whole:
        rt.log.append('work')
    assert whole.graphs == ['graph 0'] and rt.log == ['begin', 'work', 'end']
    rt = RecordingRuntime()
    with page_trainer._CutCapture(rt, pool=None) as cut:
        rt.log.append('head')
        cut.cut()
        rt.log.append('tail')
    assert cut.graphs == ['graph 0', 'graph 1']
    assert rt.log == ['begin', 'head', 'flush', 'end', 'begin', 'tail', 'end']      # deferred work goes into the graph cut off
    rt = RecordingRuntime()
    with pytest.raises(RuntimeError, match='kernel failed'):
        with page_trainer._CutCapture(rt, pool=None):
            raise RuntimeError('kernel failed')
    assert rt.log == ['begin', 'end']                                               # no capture is left open


def selected_by_the_former_blocks(argument, value, default):
    """The two blocks PageTrainer.__init__ held before they became one helper: (argument, environment value or None,
    default) -> the nets whose flag is set."""
    if argument is None:
        argument = tuple(n for n in (default if value is None else value).split(',') if n)
    return {name for name in NETS if name in argument or 'all' in argument}


@pytest.mark.parametrize('variable, default', [('UOCR_SIDE_WGRAD', ''), ('UOCR_GROUP_WGRAD', 'all'), ('UOCR_GROUP_WGRAD', 'Char')])
@pytest.mark.parametrize('argument, value', [(('Line', 'Char'), 'Monochrome'), (('all',), None), ((), 'all'),
                                             (None, 'Char'), (None, 'all'), (None, 'Line,Char'), (None, ''), (None, None)])
def test_wgrad_nets_selects_what_the_two_blocks_did(monkeypatch, variable, default, argument, value):
    if value is None:
        monkeypatch.delenv(variable, raising=False)
    else:
        monkeypatch.setenv(variable, value)
    got = page_trainer._wgrad_nets(argument, variable, default, NETS)
    assert got == selected_by_the_former_blocks(argument, value, default)
    if argument is None and value is None:                     # the defaults themselves
        assert got == {'': set(), 'all': set(NETS), 'Char': {'Char'}}[default]
    if argument is None and value == 'Line,Char':
        assert got == {'Line', 'Char'}


def test_page_context_mapping_exists_once(monkeypatch):
    expected = {'monochrome_X': 'image', 'monochrome_y': 'monochrome',
                'paragraph_X': 'monochrome', 'paragraph_y': 'paragraph',
                'line_X': 'monochrome', 'line_y': 'line',
                'char_X': 'char_lines', 'char_y': 'char_labels'}
    assert page_model.TRAIN_PAGE_CONTEXT == expected
    assert list(page_model.TRAIN_PAGE_CONTEXT) == list(expected)           # (the order contexts are filled in)
    assert page_trainer.TRAIN_PAGE_CONTEXT is page_model.TRAIN_PAGE_CONTEXT
    wanted = []

    def get(layer_tags):
        wanted.extend(layer_tags)
        return {tag: None for tag in layer_tags}
    monkeypatch.setattr(page_model.CP, 'copy', lambda array: array)
    context = page_model.make_context_maker(page_model.Modes.TRAIN_PAGE)(get)
    assert wanted == sorted(set(expected.values())) and list(context) == list(expected)
