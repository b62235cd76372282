"""The page systems of my_model/model.py as whoever runs them sees them, recorded without a GPU and compared with
tests/page_system_traces.json: what every builder assembles under every combination of the four options, which context
keys every stage of every system reads and files on three small pages, and which options the flags of the two command
lines deliver.  Public names only: the builders, the components and selectors of the systems they return, the six stage
classes of my_model/crop.py (stood in for by token makers) and the nets' predict / train / test.

page_system_traces.json is this project's own recorded output, written by

    python tests/test_page_systems_host.py --write

at the commit before the builders were folded into one stage chain; a change that keeps every system as it is leaves
the file alone."""
import itertools
import json
import os
import re
import sys
from unittest import mock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
EXPECTED = os.path.join(ROOT, 'tests', 'page_system_traces.json')

OPTION_VALUES = {'find_rotation': (False, True), 'rotation_search': ('host', 'device'),
                 'line_labelling': ('paragraph', 'page'), 'char_batching': ('line', 'page')}
PAGE_SHAPE, CHAR_SHAPE = (1, 32, 48, 1), (1, 32, 24, 1)
# lines per paragraph: a paragraph without lines in the middle, one at the end, a page without paragraphs
PAGES = {'2,0,1': [2, 0, 1], '1,0': [1, 0], 'empty': []}
RESULTS = ('text', 'text_scores', 'read_text', 'expected_text', 'char_pred', 'line_pred', 'losses')
FLAGS = ('--device-search', '--page-line-labels', '--page-char-pass')


def builders():
    """{name: (options it takes, build(**options) -> (system, models or None, names or None), context labels)}"""
    from univer_ocr_amd.my_model import evaluate, model, predict
    labels = ('monochrome_pred', 'paragraph_pred', 'line', 'char')
    both = lambda crops, shape: lambda **kw: model.make_evaluate_system(shape, crops=crops, **kw)
    loaded = lambda crops, shape: lambda **kw: (evaluate.load_evaluate_system(shape, None, crops, **kw), None, None)
    return {
        'make_model_system(TRAIN_LINE)': (('find_rotation', 'rotation_search'), lambda **kw: model.make_model_system(
            PAGE_SHAPE, mode=model.Modes.TRAIN_LINE, **kw), labels[:3]),
        'make_train_char_system': (('find_rotation', 'rotation_search', 'line_labelling'),
                                   lambda **kw: model.make_train_char_system(CHAR_SHAPE, **kw), labels),
        'make_predict_system': (tuple(OPTION_VALUES), lambda **kw: model.make_predict_system(PAGE_SHAPE, **kw),
                                ('monochrome_X',)),
        'make_evaluate_system(true)': (tuple(OPTION_VALUES), both('true', CHAR_SHAPE), labels),
        'make_evaluate_system(predicted)': (tuple(OPTION_VALUES), both('predicted', PAGE_SHAPE), ('monochrome_X', 'char')),
        'load_model_system': (tuple(OPTION_VALUES), lambda **kw: (predict.load_model_system(PAGE_SHAPE, **kw), None, None),
                              ('monochrome_X',)),
        'load_evaluate_system(true)': (tuple(OPTION_VALUES), loaded('true', CHAR_SHAPE), labels),
        'load_evaluate_system(predicted)': (tuple(OPTION_VALUES), loaded('predicted', PAGE_SHAPE), ('monochrome_X', 'char')),
    }


# what a system built by load_* is called stage by stage: it returns no names
NAMES_OF = {'load_model_system': 'make_predict_system', 'load_evaluate_system(true)': 'make_evaluate_system(true)',
            'load_evaluate_system(predicted)': 'make_evaluate_system(predicted)'}


def combinations(taken):
    """every combination of the options `taken`, and the defaults ({}) in front"""
    return [{}] + [dict(zip(taken, values)) for values in itertools.product(*(OPTION_VALUES[key] for key in taken))]


def key_of(name, options):
    return name + ''.join(f' {key}={value}' for key, value in options.items())


# ---- shape ---------------------------------------------------------------------------------------------------------------
def plain(value):
    if isinstance(value, np.ndarray):
        return value.tolist()
    if isinstance(value, (np.integer, np.floating, np.bool_)):
        return value.item()
    return value if isinstance(value, (type(None), bool, int, float, str, list, tuple, dict)) else repr(type(value))


def shape_of(system, models, names):
    from univer_ocr_amd.my_model.model import PackedLinesComponent
    from univer_ocr_amd.nn.model_system import ModelComponent
    components = []
    for component in system.components:
        record = {'class': type(component).__name__}
        if isinstance(component, ModelComponent):
            selector = component.selector
            record.update(name=component.name, delist_result=component.delist_result, selector=type(selector).__name__,
                          labels=[selector.X_label, selector.y_label, selector.pred_label])
            if models is not None:
                assert component.model is models[component.name]
            if isinstance(component, PackedLinesComponent):
                record.update(gap=component.gap, max_columns=component.max_columns)
        else:
            stage = component.stage
            record['stage'] = None if stage is None else type(stage).__name__
            record['attributes'] = None if stage is None else {key: plain(value) for key, value in sorted(vars(stage).items())}
        components.append(record)
    return {'names': names, 'models': None if models is None else list(models), 'components': components}


def record_shapes():
    """every builder under every combination of its options: {key: index into the list of distinct shapes}"""
    distinct, index = [], {}
    for name, (taken, build, _) in builders().items():
        for options in combinations(taken):
            shape = json.loads(json.dumps(shape_of(*build(**options))))
            if shape not in distinct:
                distinct.append(shape)
            index[key_of(name, options)] = distinct.index(shape)
    return {'distinct': distinct, 'index': index}


# ---- context traffic -----------------------------------------------------------------------------------------------------
class LoggedContext(dict):
    """a context that notes (stage, 'get' | 'get?' | 'set', key) once each, in the order of first appearance"""

    def __init__(self, values):
        dict.__init__(self, values)
        self.stage, self.log = 'system', []

    def note(self, kind, key):
        if [self.stage, kind, key] not in self.log:
            self.log.append([self.stage, kind, key])

    def __getitem__(self, key):
        self.note('get', key)
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        self.note('get?', key)
        return dict.get(self, key, default)

    def __setitem__(self, key, value):
        self.note('set', key)
        dict.__setitem__(self, key, value)

    def setdefault(self, key, default=None):
        self.note('get?', key)
        if key not in self:
            self.note('set', key)
        return dict.setdefault(self, key, default)

    def update(self, *args, **kwargs):
        items = dict(*args, **kwargs)
        for key in items:
            self.note('set', key)
        dict.update(self, items)


class Page:
    lines = []            # lines per paragraph of the page the token stages are on


class TokenParagraphs:
    def __init__(self, find_rotation=False, eps=1.0, max_components=4096, search='host'):
        pass

    def __call__(self, mask, arrays, divisible_by=None):
        assert divisible_by == (16, 16)
        return [[f'crop({a} in {mask}, p{p})' for p in range(len(Page.lines))] for a in arrays]


class TokenLines:
    def __init__(self, zoomed_height=32, minimal_width=8, max_components=4096, labelling='paragraph'):
        pass

    def __call__(self, masks, arrays):
        assert len(masks) == len(Page.lines) and all(len(per_array) == len(masks) for per_array in arrays)
        return [[[f'line({a} by {m}, l{n})' for n in range(count)] for a, m, count in zip(per_array, masks, Page.lines)]
                for per_array in arrays]


class TokenLabels:
    def __call__(self, arrays):
        return [[f'labels({line})' for line in paragraph] for paragraph in arrays]


class TokenText:
    def __call__(self, predictions):
        return [[f'text({line})' for line in paragraph] for paragraph in predictions]


class TokenScores:
    def __init__(self, similar=True):
        pass

    def __call__(self, predictions, labels):
        assert [len(p) for p in predictions] == [len(p) for p in labels], 'ScoreText refuses nestings that differ'
        return tuple([[f'{what}({a} | {b})' for a, b in zip(p, q)] for p, q in zip(predictions, labels)]
                     for what in ('score', 'read', 'expected'))


TOKEN_STAGES = {'CropParagraphs': TokenParagraphs, 'CropAndRotateParagraphs': TokenParagraphs, 'CropLines': TokenLines,
                'LabelChars': TokenLabels, 'PredToText': TokenText, 'ScoreText': TokenScores}


def token_net(model, name):
    """predict / train / test of `model` file a token as the only output and return it, or a small loss dict"""
    def run(kind):
        def step(X, y=None):
            model.layers_outputs, model.outputs_count = [f'{name}({X})'], 1
            return model.layers_outputs[0] if kind == 'predict' else {'output_losses': [f'{kind} {name}({X} | {y})']}
        return step
    model.predict, model.train, model.test = run('predict'), run('train'), run('test')


def traffic_of(build, names, labels, modes):
    """{mode: {page: {'log': ..., the results that are there}}} of one system, built once with the token stages in place"""
    from univer_ocr_amd.my_model import crop
    from univer_ocr_amd.nn.model_system import ModelComponent
    with mock.patch.multiple(crop, **TOKEN_STAGES):
        system = build()[0]
    assert len(system.components) == len(names)
    context = None

    def staged(name, run):
        def component_run(ctx):
            context.stage = name
            run(ctx)
        return component_run
    for name, component in zip(names, system.components):
        if isinstance(component, ModelComponent):
            token_net(component.model, name)
        for mode in modes:
            setattr(component, mode, staged(name, getattr(component, mode)))
    record = {}
    for mode in modes:
        record[mode] = {}
        for page, Page.lines in PAGES.items():
            context = LoggedContext({label: label for label in labels})
            getattr(system, mode)(context)
            record[mode][page] = {'log': context.log, **{key: dict.get(context, key) for key in RESULTS if key in context}}
    return record


def record_traffic():
    made = builders()
    record = {}
    for name, (taken, build, labels) in made.items():
        names = build()[2] or made[NAMES_OF[name]][1]()[2]
        supervised = name in ('make_model_system(TRAIN_LINE)', 'make_train_char_system')
        line = {'char_batching': 'line'} if 'char_batching' in taken else {}
        record[name] = traffic_of(lambda: build(**line), names, labels, ('predict', 'train', 'test') if supervised else ('predict',))
    return record


# ---- command lines -------------------------------------------------------------------------------------------------------
def record_command_lines():
    """what predict.main and evaluate.main hand to predict_text / evaluate_text: no flag, each flag, all three"""
    import tempfile

    from univer_ocr_amd.my_model import evaluate, predict
    from univer_ocr_amd.nn import CP
    record = {'predict': {}, 'evaluate': {}}
    with tempfile.TemporaryDirectory() as folder, mock.patch.object(CP, 'use_gpu', staticmethod(lambda device_index=None: None)):
        path = os.path.join(folder, 'page.npy')
        np.save(path, np.zeros((16, 16)))
        for flags in [()] + [(flag,) for flag in FLAGS] + [FLAGS]:
            seen = []
            with mock.patch.object(predict, 'predict_text', lambda page, *args, **kw: seen.append([list(args), kw]) or []):
                predict.main([path, *flags])
            report = evaluate.TextReport(*range(9))
            with mock.patch.object(evaluate, 'evaluate_text', lambda pages, *args, **kw: seen.append([list(args), kw]) or report):
                with mock.patch('builtins.print'):
                    evaluate.main(['--pages', '3', *flags])
            record['predict'][' '.join(flags)], record['evaluate'][' '.join(flags)] = seen
    return record


def record_all():
    return json.loads(json.dumps({'shapes': record_shapes(), 'traffic': record_traffic(), 'command_lines': record_command_lines()}))


# ---- the tests -----------------------------------------------------------------------------------------------------------
def expected():
    with open(EXPECTED) as fp:
        return json.load(fp)


def test_every_builder_assembles_what_it_did_under_every_option():
    got, want = json.loads(json.dumps(record_shapes())), expected()['shapes']
    assert sorted(got['index']) == sorted(want['index'])
    for key in want['index']:
        assert got['distinct'][got['index'][key]] == want['distinct'][want['index'][key]], key


def test_every_stage_reads_and_files_the_context_keys_it_did():
    got, want = json.loads(json.dumps(record_traffic())), expected()['traffic']
    assert sorted(got) == sorted(want)
    for name in want:
        for mode in want[name]:
            for page in want[name][mode]:
                assert got[name][mode][page] == want[name][mode][page], (name, mode, page)
        assert got[name] == want[name], name


def test_the_flags_of_both_command_lines_deliver_the_options_they_did():
    assert json.loads(json.dumps(record_command_lines())) == expected()['command_lines']


def test_the_record_covers_what_it_is_for():
    want = expected()
    assert len(want['shapes']['index']) == 5 + 9 + 6 * 17 and len(want['shapes']['distinct']) > 5 + 9 + 3 * 17 - 10
    predicted = want['traffic']['make_evaluate_system(predicted)']['predict']
    assert predicted['1,0']['text'] == [[predicted['1,0']['text'][0][0]], []] and len(predicted['1,0']['text_scores']) == 2
    assert predicted['empty']['text'] == [] and 'char_pred' not in predicted['empty'] and len(predicted['2,0,1']['log']) > 25
    assert [len(p) for p in predicted['2,0,1']['char_pred']] == [2, 0, 1]
    assert set(want['traffic']['make_train_char_system']) == {'predict', 'train', 'test'}
    both = want['command_lines']['predict'][' '.join(FLAGS)][1]
    assert (both['rotation_search'], both['line_labelling'], both['char_batching']) == ('device', 'page', 'page')


if __name__ == '__main__':
    if sys.argv[1:] != ['--write']:
        sys.exit('usage: python tests/test_page_systems_host.py --write')
    record = record_all()
    text = json.dumps(record, indent=1, sort_keys=True)
    # (a list of plain values on one line)
    text = re.sub(r'\[\n\s+([^\[\]{}]*?)\n\s+\]', lambda m: '[' + re.sub(r',\n\s+', ', ', m.group(1)) + ']', text)
    assert json.loads(text) == record
    with open(EXPECTED, 'w') as fp:
        fp.write(text + '\n')
    print(f'wrote {EXPECTED}')
