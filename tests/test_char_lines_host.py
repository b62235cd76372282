"""Host side of the packed Char pass: the layout of the lines of a page in strips (nn/ops.py: pack_layout), the proof with
the float64 oracle that a strip with 4 zero columns between neighbours and its gaps set back to zero after every conv +
LeakyReLU gives every line what the line gets alone -- and that neither a gap of 3 nor a pass without the re-zeroing
does --, the C ABI of csrc/pack_lines.hip as header and binding declare it, and the option of make_predict_system."""

import numpy as np
import pytest

from oracle import nn_oracle as O

NEW_SYMBOLS = ('uocr_pack_lines', 'uocr_zero_gaps', 'uocr_ctx_last_pack_lines')
WIDTHS = [24, 40, 17, 8, 9]


# ---- layout --------------------------------------------------------------------------------------------------------------
def test_layout_starts_are_the_widths_before_plus_four_columns_each():
    from univer_ocr_amd.nn.ops import pack_layout
    (segments, strip_w), = pack_layout(WIDTHS)
    assert [index for index, _, _ in segments] == list(range(len(WIDTHS))) and [w for _, _, w in segments] == WIDTHS
    assert [x0 for _, x0, _ in segments] == [sum(WIDTHS[:k]) + 4 * k for k in range(len(WIDTHS))]
    assert strip_w == sum(WIDTHS) + 4 * (len(WIDTHS) - 1), 'no gap at the outer ends'
    (segments, strip_w), = pack_layout([8, 8], gap=7)
    assert segments == [(0, 0, 8), (1, 15, 8)] and strip_w == 23
    (segments, strip_w), = pack_layout(np.array([11]))
    assert segments == [(0, 0, 11)] and strip_w == 11


def test_layout_respects_the_cap_keeps_the_order_and_splits_no_line():
    from univer_ocr_amd.nn.ops import pack_layout
    strips = pack_layout(WIDTHS, max_columns=48)
    assert [[(i, w) for i, _, w in segments] for segments, _ in strips] == [[(0, 24)], [(1, 40)], [(2, 17), (3, 8), (4, 9)]]
    assert strips[2] == ([(2, 0, 17), (3, 21, 8), (4, 33, 9)], 42)
    assert all(strip_w <= 48 and strip_w == segments[-1][1] + segments[-1][2] for segments, strip_w in strips)
    assert [len(s) for s, _ in pack_layout(WIDTHS, max_columns=68)] == [2, 3], '24 + 4 + 40 = 68 fits, 17 more does not'
    assert [len(s) for s, _ in pack_layout(WIDTHS, max_columns=67)] == [1, 2, 2]
    rng = np.random.default_rng(11)
    widths = rng.integers(8, 300, 200).tolist()
    strips = pack_layout(widths, max_columns=1000)
    assert [i for segments, _ in strips for i, _, _ in segments] == list(range(200)), 'every line once, in order'
    for k, (segments, strip_w) in enumerate(strips):
        assert strip_w <= 1000 and [w for i, _, w in segments] == [widths[i] for i, _, _ in segments]
        assert [x0 for _, x0, _ in segments] == [sum(w for _, _, w in segments[:j]) + 4 * j for j in range(len(segments))]
        if k + 1 < len(strips):
            assert strip_w + 4 + strips[k + 1][0][0][2] > 1000, 'a strip holds as many lines as fit'


def test_layout_a_line_over_the_cap_stands_alone_gap_three_raises_nothing_gives_nothing():
    from univer_ocr_amd.nn.ops import pack_layout
    strips = pack_layout([8, 100, 9, 10], max_columns=48)
    assert strips == [([(0, 0, 8)], 8), ([(1, 0, 100)], 100), ([(2, 0, 9), (3, 13, 10)], 23)]
    assert pack_layout([]) == []
    with pytest.raises(ValueError, match='left padding'):
        pack_layout(WIDTHS, gap=3)
    assert pack_layout(WIDTHS, gap=5)[0][1] == sum(WIDTHS) + 5 * 4
    with pytest.raises(ValueError, match='width 0'):
        pack_layout([8, 0])


# ---- exactness, with the oracle's functions ----------------------------------------------------------------------------
CH, DENSE = 6, (20, 12, 10)            # a Char-shaped chain with small channel and dense sizes


def _chain_params():
    rng = np.random.default_rng(7)
    convs = [(rng.standard_normal((5, 3, cin, CH)) / np.sqrt(15 * cin), rng.standard_normal(CH) * 0.5) for cin in (1, CH, CH)]
    sizes = (8 * CH,) + DENSE
    dense = [rng.standard_normal((n_in + 1, n_out)) / np.sqrt(n_in) for n_in, n_out in zip(sizes, sizes[1:])]
    return convs, dense


def _chain(X, params, keep=None):
    """the Char net's layers (oracle/nn_oracle.py: char_spec) on X: (1, 32, W, 1); keep: the segments [(x0, w), ...] outside
    of which every conv + LeakyReLU output is set back to zero"""
    convs, dense = params
    for w, b in convs:
        X = O.leaky_relu_fwd(O.conv2d_fwd(X, w, b, stride=(2, 1), padding=(0, 1)), 0.01)
        if keep is not None:
            mask = np.zeros(X.shape[2], bool)
            for x0, width in keep:
                mask[x0:x0 + width] = True
            X = X * mask[None, None, :, None]
    X = O.fixed_width_fwd(X, 8)
    X = X.reshape(X.shape[0], -1)
    for i, w in enumerate(dense):
        X = O.dense_fwd(X, w)
        if i + 1 < len(dense):
            X = O.leaky_relu_fwd(X, 0.01)
    return X


def _worst_line_error(lines, alone, params, gap, rezero):
    """max over the lines of |packed - alone| / scale, rows [x0, x0 + w) of the strip's output against the line's own"""
    starts = [sum(WIDTHS[:k]) + gap * k for k in range(len(WIDTHS))]
    strip = np.zeros((1, 32, starts[-1] + WIDTHS[-1], 1))
    for x, x0, w in zip(lines, starts, WIDTHS):
        strip[:, :, x0:x0 + w] = x
    segments = list(zip(starts, WIDTHS))
    out = _chain(strip, params, segments if rezero else None)
    assert out.shape == (strip.shape[2], DENSE[-1])
    scale = max(np.max(np.abs(a)) for a in alone)
    return [np.max(np.abs(out[x0:x0 + w] - a)) / scale for (x0, w), a in zip(segments, alone)]


def test_gap_of_four_with_rezeroing_is_exact_and_nothing_less_is():
    from univer_ocr_amd.nn.ops import PACK_GAP, pack_layout
    params = _chain_params()
    rng = np.random.default_rng(8)
    lines = [rng.random((1, 32, w, 1)) for w in WIDTHS]
    alone = [_chain(x, params) for x in lines]
    assert all(a.shape == (w, DENSE[-1]) for a, w in zip(alone, WIDTHS))
    (segments, _), = pack_layout(WIDTHS)
    assert PACK_GAP == 4 and [x0 for _, x0, _ in segments] == [sum(WIDTHS[:k]) + 4 * k for k in range(len(WIDTHS))]
    exact = _worst_line_error(lines, alone, params, 4, True)
    narrow = _worst_line_error(lines, alone, params, 3, True)
    stale = _worst_line_error(lines, alone, params, 4, False)
    print(f'gap 4, re-zeroed {max(exact):.2e}; gap 3, re-zeroed {max(narrow):.2e}; gap 4, not re-zeroed {max(stale):.2e}')
    assert max(exact) <= 1e-12, 'every column of a line sees what its own padding shows it'
    assert max(narrow) > 1e-3, "with 3 columns the first windows of a line reach into its neighbour's last column"
    assert max(stale) > 1e-3, 'without the re-zeroing the gaps hold leaky(bias) after the first conv'


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points():
    from univer_ocr_amd.hip import lib as hiplib
    lib = hiplib.get_lib()
    assert lib.uocr_abi_version() == 4
    for name in NEW_SYMBOLS:
        assert getattr(lib, name)
    # without a context all three refuse with UOCR_ERR_ARG before touching anything
    assert lib.uocr_pack_lines(None, 0, 0, None, None, 32, 1, None, None, 8) == -1
    assert lib.uocr_zero_gaps(None, 0, None, 32, 8, 1, 0, None, None) == -1
    assert lib.uocr_ctx_last_pack_lines(None, None, None, None) == -1


# ---- the option ----------------------------------------------------------------------------------------------------------
def test_predict_system_takes_line_or_page_and_nothing_else():
    from univer_ocr_amd.my_model.model import PackedLinesComponent, make_predict_system
    from univer_ocr_amd.nn.model_system import ModelComponent
    with pytest.raises(ValueError, match='char_batching'):
        make_predict_system((1, 32, 32, 1), char_batching='x')
    for form, kind in (('line', ModelComponent), ('page', PackedLinesComponent)):
        system, models, names = make_predict_system((1, 32, 32, 1), find_rotation=False, char_batching=form)
        char = system.components[names.index('Char')]
        assert type(char) is kind and char.model is models['Char'] and char.name == 'Char'
    default, _, names = make_predict_system((1, 32, 32, 1), find_rotation=False)
    assert type(default.components[names.index('Char')]) is ModelComponent, 'the default stays the pass per line'


def test_predict_text_and_main_pass_the_option_on(monkeypatch, tmp_path):
    from univer_ocr_amd.my_model import predict
    from univer_ocr_amd.nn import CP
    seen = []

    class System:
        def predict(self, context):
            context['text'] = [['line']]

    def load(shape, weights_path, find_rotation, rotation_search, line_labelling, char_batching='line'):
        seen.append(char_batching)
        return System()
    monkeypatch.setattr(predict, 'load_model_system', load)
    monkeypatch.setattr(CP, 'use_gpu', staticmethod(lambda device_index=None: None))
    page = np.zeros((1, 16, 16, 1))
    assert predict.predict_text(page) == [['line']] and predict.predict_text(page, char_batching='page') == [['line']]
    np.save(tmp_path / 'page.npy', page[0, :, :, 0])
    predict.main([str(tmp_path / 'page.npy')])
    predict.main([str(tmp_path / 'page.npy'), '--page-char-pass'])
    assert seen == ['line', 'page', 'line', 'page']
    monkeypatch.undo()
    names = predict.make_predict_system((1, 32, 48, 1))[2]
    system = predict.load_model_system((1, 32, 48, 1), char_batching='page')
    assert type(system.components[names.index('Char')]).__name__ == 'PackedLinesComponent'
    with pytest.raises(ValueError, match='char_batching'):
        predict.predict_text(page, char_batching='strip')


def test_forward_refuses_segments_that_do_not_fit():
    from univer_ocr_amd.my_model.model import make_char
    char = make_char((1, 32, 16, 1))
    X = np.zeros((1, 32, 20, 1))
    for segments in ([(0, 21)], [(8, 8), (0, 8)], [(0, 8), (7, 8)], [(-1, 8)], [(0, 0)]):
        with pytest.raises(ValueError, match='segments'):
            char.forward(X, keep_columns=segments)
