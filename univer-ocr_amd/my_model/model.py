"""Builders of the four OCR nets (reference: my_model/model.py:26-304) on the HIP backend:
same function names, layer names ('Monochrome/conv_1', 'Paragraph/up_2/conv_block/conv_1', ...),
channel counts, kernel sizes and losses, so `model_weights.json` files are interchangeable.

  Monochrome  conv3x3(1->16) LeakyReLU conv3x3(16->1) Sigmoid, Dice               (model.py:108-135)
  Paragraph   2 x [conv5x5 s2] down, 2 x [upsample2 + conv5x5] up, conv5x5 Sigmoid, width 1, Dice (:138-191)
  Line        same topology, width 4, 2 output maps, Dice                          (:194-247)
  Char        3 x conv(5x3, stride (2,1), pad (0,1), 64 ch) LeakyReLU, fixed-width(8) windows,
              dense 512->1024->128->162, softmax cross-entropy                     (:250-304)

Every conv carries L2(0.01) (model.py:36-39).  Of the stages that sit between the nets in the
reference's model system (host code, interpreter/), ParagraphCrop, LineCrop, CharLabel and PredToText run on the device
(my_model/crop.py): TRAIN_LINE is `make_model_system(mode=Modes.TRAIN_LINE)`, and `make_train_char_system` assembles
[ParagraphCrop, LineCrop, CharLabel, Char], the reference's TRAIN_CHAR system.  Both take `find_rotation=True` for the
reference's default ParagraphCrop, the one with the rotation search (CropAndRotateParagraphs); their own default stays
the upright crop; `rotation_search='device'` lets the device walk that search, one call per page.
`make_predict_system` chains the four nets through the device stages -- a page goes in, text comes out
(my_model/predict.py) -- with the rotation search on, as the reference has it in that mode.  The PREDICT,
TRAIN_CHAR and TRAIN_ALL members of `Modes` are not routed through `make_model_system` and say where their systems are.
`make_evaluate_system` puts CharLabel in front of Char and TextScore behind PredToText in either chain: what the Char
net read, scored against the labels that travel with the crops (my_model/evaluate.py adds the lines up).
`make_mask_evaluate_system` scores the other three nets, each on its true input: [Monochrome, Paragraph, Line, MaskScore].
"""
from enum import Enum

import numpy as np

from ..nn.gpu import CP
from ..nn.help_func import make_list_if_not
from ..nn.layers import (
    Concat, Conv2DToBatchedFixedWidthed, Convolutional2D, Flatten, FullyConnected, LeakyRelu, Sigmoid,
    Upsample2D)
from ..nn.losses import SegmentationDice2D, SoftmaxCrossEntropy
from ..nn.model_system import IterableSelector, ModelComponent, ModelSystem, RawFunctionComponent, StringSelector
from ..nn.models import Model
from ..nn.optimizers import Adam
from ..nn.progress_tracker import track_function
from ..nn.regularizations import L2

CHAR_INPUT_HEIGHT = 32
CHAR_FIXED_WIDTH = 8
N_CHARS = 162            # len(primitives.CHARS): tab, space, 66 Cyrillic, 10 digits, 52 Latin, 32 punctuation
BITS_COUNT = next(b for b in range(1, 32) if 2 ** b >= N_CHARS + 1)   # primitives/__init__.py:44: ceil(log2(len(CHARS) + 1)) = 8
OUTPUT_CHANNELS = {'monochrome': 1, 'paragraph': 1, 'line': 2}   # constants.py:19-29 LAYER_NAMES


def make_divisible_by(arr, y, x):
    """model.py:26-34 (host side): zero-pad H, W up to the next multiple -- always adds at least 1."""
    b, h, w, c = arr.shape
    add_y, add_x = y - h % y, x - w % x
    out = np.zeros((b, h + add_y, w + add_x, c))
    out[:, add_y // 2:add_y // 2 + h, add_x // 2:add_x // 2 + w, :] = arr
    return out


def make_conv(out_ch, kernel_size=(5, 5), padding=2, **kwargs):
    return Convolutional2D(kernel_size, out_channels=out_ch, padding=padding, regularizer=L2(0.01), **kwargs)


def make_conv_block(out_chs, last_sigmoid=False, **kwargs):
    out_chs = make_list_if_not(out_chs)
    layers, relations, prev = {}, {}, 0
    for i, out_ch in enumerate(out_chs, 1):
        conv_name = f'conv_{i}'
        layers[conv_name] = make_conv(out_ch, **kwargs)
        relations[conv_name] = prev
        if i == len(out_chs) and last_sigmoid:
            act_name, act = 'sigmoid', Sigmoid()
        else:
            act_name, act = f'leaky_relu_{i}', LeakyRelu(0.01)
        layers[act_name] = act
        relations[act_name] = conv_name
        prev = act_name
    relations[0] = prev
    return Model(layers, relations)


def make_up(out_chs, **kwargs):
    return Model(layers={'upsample': Upsample2D(2), 'concat': Concat(),
                         'conv_block': make_conv_block(out_chs, **kwargs)},
                 relations={'upsample': 1, 'concat': ['upsample', 0], 'conv_block': 'concat', 0: 'conv_block'})


def make_single_up(out_chs, **kwargs):
    return Model(layers={'upsample': Upsample2D(2), 'conv_block': make_conv_block(out_chs, **kwargs)},
                 relations={'upsample': 0, 'conv_block': 'upsample', 0: 'conv_block'})


def wrap(name, model, **kwargs):
    return Model(layers={name: model}, relations={name: 0, 0: name}, **kwargs)


def _defaults(optimizer):
    return {'optimizer': Adam(lr=1e-2) if optimizer is None else optimizer, 'trainable': True}


def make_monochrome(input_shape, optimizer=None):
    kwargs = _defaults(optimizer)
    block = make_conv_block([16, OUTPUT_CHANNELS['monochrome']], last_sigmoid=True, kernel_size=(3, 3),
                            padding=1, **kwargs)
    model = Model(layers={'Monochrome': block}, relations={'Monochrome': 0, 0: 'Monochrome'},
                  loss=SegmentationDice2D())
    model.initialize(input_shape)
    return model


def _make_unet(root, width, out_ch, input_shape, optimizer):
    kwargs = _defaults(optimizer)
    depth = 2
    layers = {}
    for i in range(1, depth + 1):
        layers[f'down_{i}'] = make_conv_block([width], kernel_size=(5, 5), padding=2, stride=2, **kwargs)
    for i in range(1, depth + 1):
        layers[f'up_{i}'] = make_single_up([width], kernel_size=(5, 5), padding=2, **kwargs)
    layers['end'] = make_conv_block([out_ch], last_sigmoid=True, kernel_size=(5, 5), padding=2, **kwargs)
    relations = {'down_1': 0}
    for i in range(1, depth):
        relations[f'down_{i + 1}'] = f'down_{i}'
    relations[f'up_{depth}'] = f'down_{depth}'
    for i in range(1, depth):
        relations[f'up_{i}'] = f'up_{i + 1}'
    relations['end'] = 'up_1'
    relations[0] = 'end'
    model = wrap(root, Model(layers=layers, relations=relations), loss=SegmentationDice2D())
    model.initialize(input_shape)
    return model


def make_paragraph(input_shape, optimizer=None):
    return _make_unet('Paragraph', 1, OUTPUT_CHANNELS['paragraph'], input_shape, optimizer)


def make_line(input_shape, optimizer=None):
    return _make_unet('Line', 4, OUTPUT_CHANNELS['line'], input_shape, optimizer)


def make_dense_block(out_counts, **kwargs):
    out_counts = make_list_if_not(out_counts)
    layers, relations, prev = {}, {}, 0
    for i, n_out in enumerate(out_counts, 1):
        name = f'dense_{i}'
        layers[name] = FullyConnected(n_output=n_out, **kwargs)
        relations[name] = prev
        prev = name
        if i < len(out_counts):
            act = f'leaky_relu_{i}'
            layers[act] = LeakyRelu(0.01)
            relations[act] = name
            prev = act
    relations[0] = prev
    return Model(layers, relations)


def make_char(input_shape, optimizer=None):
    batch_size, _, width, in_channels = input_shape
    kwargs = _defaults(optimizer)
    layers = {
        'conv_block': make_conv_block([64, 64, 64], kernel_size=(5, 3), padding=(0, 1), stride=(2, 1), **kwargs),
        'fixed_width': Conv2DToBatchedFixedWidthed(CHAR_FIXED_WIDTH),
        'flatten': Flatten(),
        'dense_block': make_dense_block([1024, 128, N_CHARS], **kwargs),
    }
    relations = {'conv_block': 0, 'fixed_width': 'conv_block', 'flatten': 'fixed_width',
                 'dense_block': 'flatten', 0: 'dense_block'}
    model = wrap('Char', Model(layers=layers, relations=relations), loss=SoftmaxCrossEntropy())
    model.initialize((batch_size, CHAR_INPUT_HEIGHT, width, in_channels))
    return model


NET_MAKERS = {'Monochrome': make_monochrome, 'Paragraph': make_paragraph, 'Line': make_line, 'Char': make_char}


def _make_net(name, input_shape, optimizer, progress_tracker, weights):
    """the net `name` of NET_MAKERS with its progress tracker attached and `weights` set (None: neither)"""
    model = NET_MAKERS[name](input_shape, optimizer)
    if progress_tracker is not None:
        model.init_progress_tracker(progress_tracker, name)
    if weights is not None:
        model.set_weights(weights)
    return model


def _map_nested(func, value):
    """`func` on every array of a (possibly nested) list / dict structure."""
    if isinstance(value, list):
        return [_map_nested(func, item) for item in value]
    if isinstance(value, dict):
        return {key: _map_nested(func, item) for key, item in value.items()}
    return func(value)


def _make_move_component(func, labels):
    def move(context):
        for source, target in labels:
            context[target] = _map_nested(func, context[source])
    return RawFunctionComponent(move)


def make_move_from_gpu_component(labels):
    """model.py:307-320: context[new] = host copy of context[old] for every (old, new) pair; lists and dicts are walked."""
    return _make_move_component(CP.asnumpy, labels)


def make_move_to_gpu_component(labels):
    """model.py:323-334: the other direction."""
    return _make_move_component(CP.copy, labels)


def make_char_label_component(progress_tracker=None, source='cropped_2_char', target='char_labels'):
    """model.py:614-623 (make_char_label_component) and :640-643 (move_to_gpu_char_label) as one component: the nested
    list context[source][paragraph][line] of cropped `char` arrays becomes context[target][paragraph][line], the
    (W, N_CHARS) labels of the Char net, in one kernel call for the page (my_model/crop.py: LabelChars).  Nothing visits
    the host."""
    from .crop import LabelChars
    label_chars = LabelChars()

    @track_function('CharLabel', 'forward', progress_tracker)
    def char_label(context):
        context[target] = label_chars(context[source])

    return RawFunctionComponent(char_label)


def make_pred_to_text_component(progress_tracker=None, source='char_pred', target='text', lines=None):
    """model.py:647-656 (make_pred_to_text_component) without its move component: the nested list
    context[source][paragraph][line] of the Char net's raw outputs becomes context[target][paragraph][line], the text of
    every line as a str, in one kernel call for the page (my_model/crop.py: PredToText); only the ids visit the host.
    A page without a line never reaches the Char net, so context[source] is missing there: the text is [].  lines: the
    label of the nested list of line crops the predictions were made from -- the text then has one entry per paragraph
    of context[lines], [] for the paragraphs without lines at the end of the page, which a CharSelector never files."""
    from .crop import PredToText
    pred_to_text = PredToText()

    @track_function('PredToText', 'forward', progress_tracker)
    def to_text(context):
        predictions = list(context.get(source, []))
        if lines is not None:
            predictions += [[] for _ in range(len(context[lines]) - len(predictions))]
        context[target] = pred_to_text(predictions)

    return RawFunctionComponent(to_text)


def make_text_score_component(progress_tracker=None, pred='char_pred', labels='char_labels', target='text_scores',
                              read='read_text', expected='expected_text', lines=None, similar=True):
    """No counterpart in the reference: context[pred][paragraph][line], the Char net's raw outputs, are scored against
    context[labels][paragraph][line], the labels of the same columns: context[target][p][l] = (distance, expected
    length, read length), context[read][p][l] and context[expected][p][l] the two readings as str, in one kernel call and
    one readback for the page (my_model/crop.py: ScoreText).  A page without a line never reaches the Char net, so
    context[pred] is missing there: everything is [].  lines: as in make_pred_to_text_component, the label of the nested
    list of line crops -- one entry per paragraph of context[lines], [] for the paragraphs without lines at the end of
    the page.  similar: the halves of a look-alike pair count as one character (my_model/crop.py: canonical_ids)."""
    from .crop import ScoreText
    score_text = ScoreText(similar=similar)

    @track_function('TextScore', 'forward', progress_tracker)
    def text_score(context):
        predictions = list(context.get(pred, []))
        if lines is not None:
            predictions += [[] for _ in range(len(context[lines]) - len(predictions))]
        truth = list(context.get(labels, []))[:len(predictions)] if predictions else []
        context[target], context[read], context[expected] = score_text(predictions, truth)

    return RawFunctionComponent(text_score, score_text)


def make_paragraph_crop_component(find_rotation=False, progress_tracker=None, sources=('monochrome_pred', 'line'),
                                  targets=('cropped_monochrome', 'cropped_line'), rotation_search='host'):
    """model.py:552-576 (make_paragraph_crop_component) as a device component: the stage labels context['paragraph_pred']
    and cuts every context[source] to every paragraph, padded to multiples of 16: context[target][paragraph]
    (my_model/crop.py: CropParagraphs; with find_rotation=True CropAndRotateParagraphs, the reference's default, whose
    angle search walks its rounds on the host, or with rotation_search='device' in one call on the device)."""
    from .crop import CropAndRotateParagraphs, CropParagraphs
    crop_paragraphs = (CropAndRotateParagraphs(find_rotation=True, search=rotation_search) if find_rotation
                       else CropParagraphs(find_rotation=False))
    if len(sources) != len(targets):
        raise ValueError(f'make_paragraph_crop_component: {len(sources)} sources for {len(targets)} targets')

    @track_function('ParagraphCrop', 'forward', progress_tracker)
    def paragraph_crop(context):
        crops = crop_paragraphs(context['paragraph_pred'], [context[source] for source in sources], divisible_by=(16, 16))
        context.update(zip(targets, crops))

    return RawFunctionComponent(paragraph_crop, crop_paragraphs)


def make_line_crop_component(progress_tracker=None, mask='cropped_line', sources=('cropped_monochrome', 'cropped_char'),
                             targets=('cropped_2_monochrome', 'cropped_2_char'), empty_page_ok=False,
                             line_labelling='paragraph'):
    """model.py:595-612 (make_line_crop_component) as a device component: context[mask][paragraph] is the paragraph's
    (1, H, W, 2) line mask (the reference reads it as `line_pred_cpu`, in TRAIN_CHAR the renamed `cropped_line_cpu`,
    :635-637), context[source][paragraph] a companion array; context[target][paragraph][line] becomes the line cut out
    of it, turned upright, zoomed to CHAR_INPUT_HEIGHT rows and padded to CHAR_FIXED_WIDTH columns
    (my_model/crop.py: CropLines).  One kernel call for the page; the host reads the component tables only.
    empty_page_ok: a missing context[mask] is a page without paragraphs (a LineSelector that met none files nothing).
    line_labelling: 'paragraph' labels the two masks of every paragraph in calls of their own, 'page' all masks of the
    page in ONE label_batch call with one readback (my_model/crop.py: CropLines)"""
    from .crop import CropLines
    crop_lines = CropLines(CHAR_INPUT_HEIGHT, CHAR_FIXED_WIDTH, labelling=line_labelling)
    if len(sources) != len(targets):
        raise ValueError(f'make_line_crop_component: {len(sources)} sources for {len(targets)} targets')

    @track_function('LineCrop', 'forward', progress_tracker)
    def line_crop(context):
        masks = context.get(mask, []) if empty_page_ok else context[mask]
        context.update(zip(targets, crop_lines(masks, [context[source] for source in sources])))

    return RawFunctionComponent(line_crop, crop_lines)


class LineSelector(IterableSelector):
    """One sample per paragraph (model.py:353-373): context[X_label][p], context[y_label][p]; the prediction of
    paragraph p is filed at context[pred_label][p].  The position starts over with every bind."""

    def __init__(self, X_label, y_label, pred_label):
        IterableSelector.__init__(self, X_label, y_label, pred_label)
        self.paragraph_id = 0

    def __call__(self, context):
        IterableSelector.__call__(self, context)
        self.paragraph_id = 0

    def get(self):
        Xs, ys = self.context[self.X_label], self.context[self.y_label]
        for self.paragraph_id in range(len(Xs)):
            yield Xs[self.paragraph_id], ys[self.paragraph_id]

    def get_X(self):
        Xs = self.context[self.X_label]
        for self.paragraph_id in range(len(Xs)):
            yield Xs[self.paragraph_id]

    @staticmethod
    def _grown(store, index):
        """`store`, with empty entries appended until position `index` exists (a paragraph without lines leaves a gap)"""
        while index >= len(store):
            store.append([])
        return store

    def put(self, pred):
        per_paragraph = self.context.setdefault(self.pred_label, [])
        self._grown(per_paragraph, self.paragraph_id)[self.paragraph_id] = pred


class CharSelector(LineSelector):
    """One sample per line of every paragraph (model.py:376-400): context[X_label][p][l]; predictions are filed at
    context[pred_label][p][l].  Paragraphs may hold different numbers of lines."""

    def __init__(self, X_label, y_label, pred_label):
        LineSelector.__init__(self, X_label, y_label, pred_label)
        self.line_id = 0

    def __call__(self, context):
        LineSelector.__call__(self, context)
        self.line_id = 0

    def get(self):
        Xs, ys = self.context[self.X_label], self.context[self.y_label]
        for self.paragraph_id in range(len(Xs)):
            for self.line_id in range(len(Xs[self.paragraph_id])):
                yield Xs[self.paragraph_id][self.line_id], ys[self.paragraph_id][self.line_id]

    def get_X(self):
        Xs = self.context[self.X_label]
        for self.paragraph_id in range(len(Xs)):
            for self.line_id in range(len(Xs[self.paragraph_id])):
                yield Xs[self.paragraph_id][self.line_id]

    def put(self, pred):
        per_paragraph = self.context.setdefault(self.pred_label, [])
        per_line = self._grown(per_paragraph, self.paragraph_id)[self.paragraph_id]
        self._grown(per_line, self.line_id)[self.line_id] = pred


class PackedLinesComponent(ModelComponent):
    """The Char net over ALL lines of a page in one pass per strip (predict only; train and test stay one optimizer step
    per line, the reference's semantics).  The lines the selector yields -- (1, CHAR_INPUT_HEIGHT, W, 1), W >=
    CHAR_FIXED_WIDTH -- are laid side by side with `gap` zero columns between neighbours (ops.pack_layout, ops.pack_lines),
    the model runs once on the strip with the gaps set back to zero after every conv + LeakyReLU
    (Model.forward(keep_columns=...)), and the prediction of a line is the row range [x0, x0 + w) of the strip's (strip_w,
    N_CHARS) output: a view that keeps the strip's output alive, filed where CharSelector.put files the per-line pass's.
    Exact, not approximate: every column of a line sees what its own padding shows it alone.
    max_columns: the widest strip; a page with more columns takes several passes."""

    def __init__(self, name, model, selector, delist_result=False, gap=4, max_columns=32768):
        ModelComponent.__init__(self, name, model, selector, delist_result)
        self.gap, self.max_columns = gap, max_columns

    def predict(self, context):
        from ..nn import ops
        from ..nn.gpu import DeviceArray
        selector = self.selector
        selector(context)
        lines, places = [], []
        for X in selector.get_X():
            lines.append(X)
            places.append((selector.paragraph_id, selector.line_id))
        for a in lines:
            if not isinstance(a, DeviceArray) or a.ndim != 4 or (a.shape[0], a.shape[1], a.shape[3]) != (1, CHAR_INPUT_HEIGHT, 1) \
                    or a.shape[2] < CHAR_FIXED_WIDTH or a.dtype != lines[0].dtype:
                raise ValueError(f'{self.name}: the lines of a page are (1, {CHAR_INPUT_HEIGHT}, W, 1) device arrays of one '
                                 f'dtype, W >= {CHAR_FIXED_WIDTH}, got {getattr(a, "shape", type(a))} {getattr(a, "dtype", "")}')
        for segments, strip_w in ops.pack_layout([a.shape[2] for a in lines], self.gap, self.max_columns):
            strip = ops.pack_lines(lines, (segments, strip_w))
            outputs = self.model.forward(strip, keep_columns=[(x0, w) for _, x0, w in segments])
            for index, x0, w in segments:
                views = [DeviceArray(out.t[x0:x0 + w]) for out in outputs]
                context['prediction'][self.name] = views
                selector.paragraph_id, selector.line_id = places[index]
                selector.put(views[0] if self.delist_result else views)


# what the modes that still raise are waiting for (the reference's component order, model.py:489-500)
_MISSING_STAGE = {
    'TRAIN_CHAR': 'this mode is not routed through the device LineCrop stage yet: build the system [ParagraphCrop, '
                  'LineCrop, CharLabel, Char] with make_train_char_system and its context with '
                  'make_train_char_context_maker',
    'TRAIN_ALL': 'the nets have not been chained through the device ParagraphCrop / LineCrop / CharLabel stages yet '
                 '(TRAIN_CHAR alone is make_train_char_system)',
    'PREDICT': 'the system that ends in PredToText is built by make_predict_system (my_model/predict.py runs it)',
}


class Modes(Enum):
    TRAIN_MONOCHROME = 0
    TRAIN_PARAGRAPH = 1
    TRAIN_LINE = 2
    TRAIN_CHAR = 3
    TRAIN_ALL = 4
    PREDICT = 5
    TRAIN_PAGE = 6        # this backend: all four nets on device-resident page / line batches


# {context label: dataset layer tag} of Modes.TRAIN_PAGE (make_context_maker, trainer.PageTrainer.make_context)
TRAIN_PAGE_CONTEXT = {'monochrome_X': 'image', 'monochrome_y': 'monochrome',
                      'paragraph_X': 'monochrome', 'paragraph_y': 'paragraph',
                      'line_X': 'monochrome', 'line_y': 'line',
                      'char_X': 'char_lines', 'char_y': 'char_labels'}


def _context_maker(mapping):
    """dataset layers -> context dict {label: the layer `tag` on the device} for mapping = {label: tag}"""
    def make_context(dataset_get_func, args=(), kwargs={}):
        layers = dataset_get_func(*args, layer_tags=sorted(set(mapping.values())), **kwargs)
        return {label: CP.copy(layers[tag]) for label, tag in mapping.items()}
    return make_context


def make_context_maker(mode=Modes.PREDICT):
    """model.py:412-483: dataset layers -> context dict with every array moved to the device."""
    wanted = {
        Modes.TRAIN_MONOCHROME: {'monochrome_X': 'image', 'monochrome_y': 'monochrome'},
        Modes.TRAIN_PARAGRAPH: {'paragraph_X': 'monochrome', 'paragraph_y': 'paragraph'},
        Modes.TRAIN_PAGE: TRAIN_PAGE_CONTEXT,
        # model.py:438-447 keeps these three on the host (`*_cpu`) for its host crop stage; here the crop runs on the device
        Modes.TRAIN_LINE: {'monochrome_pred': 'monochrome', 'paragraph_pred': 'paragraph', 'line': 'line'},
        Modes.PREDICT: {'monochrome_X': 'image'},
    }
    if mode not in wanted:
        raise NotImplementedError(
            f'{mode.name} has no context maker here: {_MISSING_STAGE[mode.name]} '
            f'(the device stages are in my_model/crop.py)')
    return _context_maker(wanted[mode])


# What differs between the page systems, as (predicted, labelled, last).  predicted: Monochrome, Paragraph and Line stand in
# front of the crops they feed and LineCrop reads Line's prediction (a missing one is an empty page) -- else the true `line`
# layer rides through ParagraphCrop and is LineCrop's mask; labelled: the `char` layer rides through both crop stages and
# CharLabel reads it; last: the stage the system ends after, the supervised one where it is a net.
_CUTS = {'TRAIN_LINE': (False, False, 'Line'), 'TRAIN_CHAR': (False, True, 'Char'), 'PREDICT': (True, False, 'PredToText'),
         'true': (False, True, 'TextScore'), 'predicted': (True, True, 'TextScore')}


def _page_chain(cut, net=None, tracker=None, find_rotation=False, rotation_search='host', line_labelling='paragraph',
                similar=True):
    """The chain every page system is a cut of, in the reference's component order (model.py:489-500): [(name, make)] of
    the stages that _CUTS[cut] holds.  make() builds the component: net(name, selector class, X label, y label, prediction
    label) that of a net, a make_*_component that of a device stage of my_model/crop.py, with the labels it reads and
    files.  Nothing is built before that, so the names of a cut need no further argument."""
    predicted, labelled, last = _CUTS[cut]
    riders = ('monochrome_pred',) + ('line',) * (not predicted) + ('char',) * labelled      # through ParagraphCrop
    companions = tuple(layer for layer in riders if layer != 'line')                         # through LineCrop too
    cropped = lambda prefix, layers: tuple(prefix + layer.removesuffix('_pred') for layer in layers)
    chain = (
        ('Monochrome', predicted, lambda: net('Monochrome', StringSelector, 'monochrome_X', None, 'monochrome_pred')),
        ('Paragraph', predicted, lambda: net('Paragraph', StringSelector, 'monochrome_pred', None, 'paragraph_pred')),
        ('ParagraphCrop', True, lambda: make_paragraph_crop_component(
            find_rotation, tracker, riders, cropped('cropped_', riders), rotation_search)),
        ('Line', predicted or last == 'Line', lambda: net(
            'Line', LineSelector, 'cropped_monochrome', 'cropped_line', 'line_pred')),
        ('LineCrop', True, lambda: make_line_crop_component(
            tracker, 'line_pred' if predicted else 'cropped_line', cropped('cropped_', companions),
            cropped('cropped_2_', companions), empty_page_ok=predicted, line_labelling=line_labelling)),
        ('CharLabel', labelled, lambda: make_char_label_component(tracker, 'cropped_2_char', 'char_labels')),
        ('Char', True, lambda: net('Char', CharSelector, 'cropped_2_monochrome', 'char_labels', 'char_pred')),
        ('PredToText', True, lambda: make_pred_to_text_component(tracker, 'char_pred', 'text', lines='cropped_2_monochrome')),
        ('TextScore', True, lambda: make_text_score_component(tracker, 'char_pred', 'char_labels', 'text_scores',
                                                              lines='cropped_2_monochrome', similar=similar)),
    )
    end = [name for name, _, _ in chain].index(last) + 1
    return [(name, make) for name, present, make in chain[:end] if present]


def _make_page_system(who, cut, input_shape, optimizer, progress_tracker, weights, char_batching='line', **options):
    """(model_system, models, names) of the cut `cut` of _page_chain, which takes the `options`.  char_batching is checked
    here (`who`: the builder in the message), the other options by the stages they reach.  input_shape is the page's where
    the nets stand in front -- the Char net then takes lines of 64 columns -- and else the one net's own; a net gets its
    `y` where the system ends after it."""
    if char_batching not in ('line', 'page'):
        raise ValueError(f"{who}: char_batching must be 'line' or 'page', got {char_batching!r}")
    predicted, _, last = _CUTS[cut]
    models = {}

    def net(name, selector, X, y, pred):
        shape = (input_shape[0], CHAR_INPUT_HEIGHT, 64, 1) if name == 'Char' and predicted else input_shape
        models[name] = _make_net(name, shape, optimizer, progress_tracker, weights)
        kind = PackedLinesComponent if name == 'Char' and char_batching == 'page' else ModelComponent
        return kind(name, models[name], selector(X, y if name == last else None, pred), delist_result=True)
    chain = _page_chain(cut, net, progress_tracker, **options)
    return ModelSystem([make() for _, make in chain]), models, [name for name, _ in chain]


def make_model_system(input_shape, optimizer=None, progress_tracker=None, weights=None, mode=Modes.PREDICT,
                      char_input_shape=None, find_rotation=False, rotation_search='host'):
    """model.py:486-717 for the device-resident modes.  Returns (model_system, models, names).

    TRAIN_LINE is the system [ParagraphCrop, Line] (names ['ParagraphCrop', 'Line']): the crop stage labels
    context['paragraph_pred'], cuts context['monochrome_pred'] and context['line'] to every paragraph, pads the crops to
    multiples of 16 (make_divisible_by) and files them as context['cropped_monochrome'] / ['cropped_line']; the Line net
    then takes one step per paragraph through a LineSelector and files line_pred[paragraph].  That equals the reference's
    TRAIN_LINE system (model.py:585-593) built with find_rotation=False, minus its move_to_gpu component: no array
    visits the host between the stages (the crop stage reads back the component table only).  find_rotation=True (TRAIN_LINE
    only) puts CropAndRotateParagraphs in the ParagraphCrop slot: the reference's default, every paragraph turned by the
    angle of its rotation search; rotation_search='device' lets the device walk that search (one call per page)."""
    if mode is Modes.TRAIN_LINE:
        return _make_page_system('make_model_system', 'TRAIN_LINE', input_shape, optimizer, progress_tracker, weights,
                                 find_rotation=find_rotation, rotation_search=rotation_search)
    if find_rotation:
        raise ValueError(f'find_rotation=True: {mode.name} has no ParagraphCrop stage')
    plan = {
        Modes.TRAIN_MONOCHROME: ['Monochrome'],
        Modes.TRAIN_PARAGRAPH: ['Paragraph'],
        Modes.TRAIN_PAGE: ['Monochrome', 'Paragraph', 'Line', 'Char'],
    }
    if mode not in plan:
        raise NotImplementedError(
            f'{mode.name} is not assembled by make_model_system: {_MISSING_STAGE[mode.name]}; '
            f'use TRAIN_MONOCHROME / TRAIN_PARAGRAPH / TRAIN_LINE / TRAIN_PAGE')
    components, models = [], {}
    for name in plan[mode]:
        shape = input_shape
        if name == 'Char':
            shape = char_input_shape or (input_shape[0], CHAR_INPUT_HEIGHT, 64, 1)
        model = _make_net(name, shape, optimizer, progress_tracker, weights)
        key = name.lower()
        components.append(ModelComponent(name, model, StringSelector(f'{key}_X', f'{key}_y', f'{key}_pred'),
                                         delist_result=True))
        models[name] = model
    return ModelSystem(components), models, list(plan[mode])


def make_train_char_context_maker():
    """model.py:449-459 (the TRAIN_CHAR context) for `make_train_char_system`: the layers monochrome, paragraph, line and
    char of one page, moved to the device (the reference keeps them on the host for its host stages)."""
    return _context_maker({'monochrome_pred': 'monochrome', 'paragraph_pred': 'paragraph', 'line': 'line', 'char': 'char'})


def make_train_char_system(input_shape, optimizer=None, progress_tracker=None, weights=None, find_rotation=False,
                           rotation_search='host', line_labelling='paragraph'):
    """model.py:632-645: the reference's TRAIN_CHAR system built with find_rotation=False (or, with find_rotation=True,
    as the reference builds it: CropAndRotateParagraphs in the ParagraphCrop slot, its angle search on the host or, with
    rotation_search='device', on the device), minus its rename and move
    components -- no array visits the host between the stages.  Returns (model_system, {'Char': model},
    ['ParagraphCrop', 'LineCrop', 'CharLabel', 'Char']).
      ParagraphCrop  labels context['paragraph_pred'], cuts context['monochrome_pred'], ['line'] and ['char'] to every
                     paragraph and pads the crops to multiples of 16: context['cropped_monochrome' / '_line' / '_char']
      LineCrop       finds the lines of every paragraph in cropped_line and cuts them out of cropped_monochrome and
                     cropped_char: context['cropped_2_monochrome'][p][l], ['cropped_2_char'][p][l]
      CharLabel      context['char_labels'][p][l] from cropped_2_char
      Char           one step per line through a CharSelector; predictions at context['char_pred'][p][l]
    input_shape is the Char net's, (batch, *, width, channels): its height is CHAR_INPUT_HEIGHT.  line_labelling:
    'paragraph' or 'page', how LineCrop labels its masks (make_line_crop_component)."""
    return _make_page_system('make_train_char_system', 'TRAIN_CHAR', input_shape, optimizer, progress_tracker, weights,
                             find_rotation=find_rotation, rotation_search=rotation_search, line_labelling=line_labelling)


def make_predict_system(input_shape, progress_tracker=None, weights=None, find_rotation=True, rotation_search='host',
                        line_labelling='paragraph', char_batching='line'):
    """model.py:688-717: the reference's PREDICT system without its rename and move components -- a page goes in as
    context['monochrome_X'] (1, H, W, 1), H and W multiples of 16 (make_divisible_by), and context['text'][p][l] comes
    out.  No array visits the host between the stages: only the component tables, the probe extents of the rotation
    search and the final ids are read back.  Returns (model_system, models, names), names = ['Monochrome', 'Paragraph',
    'ParagraphCrop', 'Line', 'LineCrop', 'Char', 'PredToText'].
      Monochrome     monochrome_X -> monochrome_pred
      Paragraph      reads monochrome_pred (the reference renames it to paragraph_X) -> paragraph_pred
      ParagraphCrop  labels paragraph_pred, cuts monochrome_pred to every paragraph, turned by the angle of its rotation
                     search (find_rotation=True, the reference's default in this mode), in make_divisible_by's frame:
                     cropped_monochrome[p]
      Line           one pass per paragraph through a LineSelector -> line_pred[p]
      LineCrop       finds the lines of every paragraph in line_pred and cuts them out of cropped_monochrome:
                     cropped_2_monochrome[p][l]
      Char           one pass per line through a CharSelector (char_batching='page': one per page) -> char_pred[p][l]
      PredToText     text[p][l] from char_pred
    The nets are built for input_shape and take every size they meet afterwards (crops are multiples of 16, lines 32
    rows high and at least 8 columns wide).  rotation_search: 'host' walks the 13 rounds of the angle search on the
    host, a readback per round; 'device' makes it one call and one readback per page (my_model/crop.py).
    line_labelling: 'paragraph' or 'page', how LineCrop labels its masks (make_line_crop_component).
    char_batching: 'line' runs the Char net once per line, 'page' once per page on all lines laid side by side
    (PackedLinesComponent): the same predictions from one pass."""
    return _make_page_system('make_predict_system', 'PREDICT', input_shape, None, progress_tracker, weights, char_batching,
                             find_rotation=find_rotation, rotation_search=rotation_search, line_labelling=line_labelling)


EVALUATE_NAMES = {crops: [name for name, _ in _page_chain(crops)] for crops in ('true', 'predicted')}


def make_evaluate_context_maker(crops):
    """the context of make_evaluate_system(crops=...) from one page of a dataset: with 'true' the label layers the crop
    stages read (the TRAIN_CHAR context), with 'predicted' the image, as in PREDICT, and the `char` layer that rides
    through the crop stages beside it"""
    if crops not in EVALUATE_NAMES:
        raise ValueError(f"make_evaluate_context_maker: crops must be 'true' or 'predicted', got {crops!r}")
    if crops == 'true':
        return make_train_char_context_maker()
    return _context_maker({'monochrome_X': 'image', 'char': 'char'})


def make_evaluate_system(input_shape, progress_tracker=None, weights=None, crops='true', find_rotation=None,
                         rotation_search='host', line_labelling='paragraph', char_batching='line', similar=True):
    """What the Char net reads, scored against the labels that travel with the crops.  Returns (model_system, models,
    names); run it with `predict`: context['text_scores'][p][l] = (distance, expected length, read length),
    context['read_text'][p][l], context['expected_text'][p][l] and, as in PREDICT, context['text'][p][l].
      crops='true'       the Char net alone: the TRAIN_CHAR chain on the page's true layers (make_train_char_system),
                         [ParagraphCrop, LineCrop, CharLabel, Char, PredToText, TextScore]; input_shape is the Char
                         net's; find_rotation defaults to False, as there
      crops='predicted'  end to end: the PREDICT chain (make_predict_system) with `char` among the sources of
                         ParagraphCrop and LineCrop and CharLabel in front of Char, [Monochrome, Paragraph,
                         ParagraphCrop, Line, LineCrop, CharLabel, Char, PredToText, TextScore]; input_shape is the
                         page's; find_rotation defaults to True, as there
    The labels are cut, turned and zoomed by the same boxes as the pixels the net sees, so label and prediction cover the
    same columns whatever the crop stages found.  rotation_search, line_labelling, char_batching: as in
    make_predict_system; similar: as in make_text_score_component."""
    if crops not in EVALUATE_NAMES:
        raise ValueError(f"make_evaluate_system: crops must be 'true' or 'predicted', got {crops!r}")
    find_rotation = (crops == 'predicted') if find_rotation is None else find_rotation
    return _make_page_system('make_evaluate_system', crops, input_shape, None, progress_tracker, weights, char_batching,
                             find_rotation=find_rotation, rotation_search=rotation_search, line_labelling=line_labelling,
                             similar=similar)


MASK_NETS = ('monochrome', 'paragraph', 'line')
MASK_EVALUATE_NAMES = ['Monochrome', 'Paragraph', 'Line', 'MaskScore']


def make_mask_score_component(progress_tracker=None, nets=MASK_NETS, target='mask_scores', rules=None):
    """No counterpart in the reference: for every net of `nets`, context[f'{net}_pred'] is scored against
    context[f'{net}_y'], both (1, H, W, C): context[target][net][channel] = the MaskScore of that channel (nn/ops.py),
    prediction and truth thresholded by the rule of the stage that reads the net (my_model/crop.py: MASK_RULES, or
    `rules`) and labelled by the code the stages use."""
    from .crop import MASK_RULES, ScoreMasks
    score_masks = ScoreMasks(MASK_RULES if rules is None else rules)

    @track_function('MaskScore', 'forward', progress_tracker)
    def mask_score(context):
        context[target] = {net: score_masks(net, context[f'{net}_pred'], context[f'{net}_y']) for net in nets}

    return RawFunctionComponent(mask_score, score_masks)


def make_mask_evaluate_context_maker():
    """the context of make_mask_evaluate_system from one page of a dataset: every mask net's true input and its truth, the
    labels TRAIN_PAGE_CONTEXT gives them (image -> monochrome, monochrome -> paragraph, monochrome -> line)"""
    return _context_maker({label: tag for label, tag in TRAIN_PAGE_CONTEXT.items() if not label.startswith('char')})


def make_mask_evaluate_system(input_shape, progress_tracker=None, weights=None, rules=None):
    """How good the three mask nets are, each on its TRUE input at page size.  Returns (model_system, models, names),
    names = ['Monochrome', 'Paragraph', 'Line', 'MaskScore']; run it with `predict` on a context of
    make_mask_evaluate_context_maker: context['mask_scores'][net][channel] is a MaskScore (net = 'monochrome', 'paragraph',
    'line'; 1, 1 and 2 channels), the predictions stay at context[f'{net}_pred'].  Thresholds are the stages' own --
    Paragraph 'mean' (ParagraphCrop), Line 'mean_max' per channel (LineCrop), Monochrome the number 0.5 with caps 0,
    foreground against foreground -- and the truth of each net is thresholded by the rule of its prediction.  input_shape
    is the page's, (1, H, W, 1) with H and W multiples of 16."""
    models, components = {}, []
    for name in MASK_EVALUATE_NAMES[:3]:
        models[name] = _make_net(name, input_shape, None, progress_tracker, weights)
        key = name.lower()
        components.append(ModelComponent(name, models[name], StringSelector(f'{key}_X', None, f'{key}_pred'),
                                         delist_result=True))
    components.append(make_mask_score_component(progress_tracker, rules=rules))
    return ModelSystem(components), models, list(MASK_EVALUATE_NAMES)
