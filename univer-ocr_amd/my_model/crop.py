"""The stages that sit between the nets, on the device.

CropParagraphs is the reference's CropAndRotateParagraphs (interpreter/interpreter.py:351-378) with
`find_rotation=False`: label the paragraph layer (label_layer, :16-21), take one bounding box per component
(ndimage.find_objects, :303) and cut every companion array to it, zeroed outside the component (:304-308).  With no
rotation angle `_func` (:314-348) hands the crops back unchanged, so that is the whole stage.  Arrays stay in HBM: the
labelling, the boxes and the crops are kernels of libuniver_hip.so (nn/ops.py: label_components, masked_crop); the only
thing the host reads is the component table (64 bytes per paragraph).  There is no worker pool.

CropAndRotateParagraphs is the same stage with the reference's default, `find_rotation=True` (:319-347).  Per paragraph
the reference runs a ternary search over 0..180 degrees for the angle at which the order-0 rotation of the component's
mask is lowest -- 13 rounds of two probes at EPS = 1, each probe a full ndimage.rotate and a find_objects on a worker
process -- rotates the mask once more for the region its pixels cover, rotates every companion crop at order 1 and cuts
it to that region; an angle outside [EPS, 180 - EPS] means "not rotated".  Here a probe is four ints: the kernel behind
nn/ops.py: rotated_extent asks of every pixel of the would-be rotated plane whether it is set and keeps the extent, no
rotated array is written.  `search_angle` restates the search on the host; all paragraphs of a page walk through it in
lock step, so a round is ONE call holding both probes of every paragraph, one more call gets the regions at the final
angles, and ONE rotate_crop call produces all arrays of all rotated paragraphs, make_divisible_by's frame included: 14
extent calls and 1 crop call per page, whatever the number of paragraphs, 16 bytes read back per probe.  The geometry
(matrix, offset, shape of the rotated plane) is computed on the host as scipy computes it (nn/ops.py:
rotation_geometry).  Unrotated paragraphs go through masked_crop as in CropParagraphs.  search='device' hands the 13
rounds to the device (nn/ops.py: rotation_search): the search tree does not depend on the data, so every angle it can
visit is tabulated once and the device walks it for all paragraphs, round after round in stream order -- 1 search call
with 1 readback, 1 extent call and 1 crop call per page.  The default stays the host search.

LabelChars is the reference's LabelChar (interpreter/interpreter.py:524-571): the `char` layer tag of every cropped line
-- bit layers first, then letter_spacing -- becomes the (W, N_CHARS) one-hot labels the Char net trains on.  Per line:
threshold at (mean + max) / 2 of the whole array, read every pixel's bits as a class number (least significant bit
first; a number that is no class is "unknown"), let every column vote over its rows (the first candidate from the top
wins a tie, "unknown" is one candidate) and write a one-hot row, or a zero row where "unknown" won.  The reference does
this in a Python loop per pixel on a worker pool, between a device-to-host and a host-to-device copy of every line; here
all lines of all paragraphs of a page are ONE kernel call (nn/ops.py: char_label) and nothing leaves HBM.

CropLines is the reference's CropRotateAndZoomLines (interpreter/interpreter.py:421-523).  Per paragraph, the two
channels of the line mask (line_top, line_bottom) are thresholded at (mean + max) / 2 of their own and labelled
(:437-453; label_layer's second threshold at the mean changes nothing) -- nn/ops.py: label_components with 'mean_max'.
The host reads the two component tables, nothing else, and `arrange_lines` restates rearrange_lines (:42-82) on the
centres of mass: which bottom belongs to which top, which way the text runs, the reading order.  A line's box is the
union of its two components' boxes (:494-502); every companion array is cut to it unmasked, turned by a multiple of 90
degrees so that the text reads left to right, zoomed to 32 rows at order 0 and zero-padded to 8 columns (:504-523).  All
lines of all paragraphs and all arrays of a page are ONE kernel call (nn/ops.py: line_crop); there is no worker pool.
labelling='page' labels the masks of ALL paragraphs of the page in one call (nn/ops.py: label_batch): both channels of
every mask are read in place, no split, one launch chain and one readback of a few rows per mask, instead of one split,
two labelling calls and four readbacks per paragraph.  The default stays 'paragraph'.

PredToText is the reference's PredToText (interpreter/interpreter.py:574-614): the Char net's raw output of every line,
(W, N_CHARS) with one row per column window, becomes the line's text.  Per row the columns that EQUAL the row's maximum
are candidates (several on an exact tie; none where the maximum is 0 or the row holds a NaN); the candidates of a line
are walked in order with the last emitted character at hand: the tab (id 0) resets it and emits nothing, a character
"similar" to it -- the other half of one of 18 Cyrillic / Latin look-alike pairs, or the character itself if it HAS a
pair -- is dropped, everything else is emitted.  So "aa" reads "a" and "bb" stays "bb": the reference's behaviour, kept
as it is.  `pred_to_text_rules` restates that walk in NumPy.  The device decides every emission from two adjacent
candidates (the remembered character always lies in the pair class of the last candidate that was not the tab), for all
lines of all paragraphs of a page in ONE kernel call (nn/ops.py: pred_to_text), a second one only for lines with tied
rows; the host reads back the ids and nothing else.  The reference copies every prediction to the host and hands it to
a worker pool.

ScoreText has no counterpart in the reference (its nn/metrics.py is a stub): per line, the Char net's raw output and the
one-hot labels of the same columns are read by ONE rule -- the first maximum of every row, one id per run of equal ids,
the tab and rows without a maximum end a run -- and compared by the unit-cost edit distance, two ids matching when the
table `canonical_ids` maps them to one id (by default the halves of a look-alike pair, whose glyphs the generator draws
from the same pixels).  All lines of a page are ONE kernel call (nn/ops.py: text_score) and one readback of the scores
and ids; DESIGN.md section 8 says why the score is not taken between context['text'] and the typed text.

ScoreMasks has none either (nn/metrics.py: binary_classification_metrics is the pixel half of it, and nothing there calls
it): every channel of a mask net's prediction and of its truth is thresholded by ONE rule -- the rule of the stage that
reads the net: 'mean' for ParagraphCrop, 'mean_max' for LineCrop, a number for Monochrome --, both are labelled by the
code the stages use (uocr_label_batch) and the overlap counts of the two label planes give the pixel numbers and how many
of the true components the prediction found (nn/ops.py: mask_score, uocr_label_overlap).
"""
import string

import numpy as np

from ..nn import ops
from .model import CHAR_FIXED_WIDTH, CHAR_INPUT_HEIGHT

QUARTER_TURNS = {None: 0, 90: 1, 180: 2, 270: 3}     # the reference's `rotation` -> np.rot90's k


def arrange_lines(top_centers, bottom_centers):
    """rearrange_lines (interpreter.py:42-82) on the (y, x) centres of mass of a paragraph's line_top and line_bottom
    components, both in label order: returns (top_ids, bottom_ids, rotation) -- line i of the paragraph is made of top
    component top_ids[i] and bottom component bottom_ids[i] (0-based), rotation is None, 90, 180 or 270 -- or None where
    the reference raises: no top, no bottom, or the first top's centre on the first bottom's.
      * every top takes the bottom whose centre is nearest, the first in label order on a tie; a bottom may serve two tops
        or none
      * the direction is the first top's centre minus the centre of the FIRST bottom in label order (not the paired
        one); the reference's `*= 1000` loop only pushes positive components past the image, so the sign decides:
        |dy| > |dx|: dy < 0 upright, lines by y ascending; dy > 0 180, by y descending;
        otherwise: dx < 0 270, by x ascending; dx > 0 90, by x descending
      * tops are sorted by their own centres and the paired bottoms SEPARATELY by theirs, both stably"""
    top = np.asarray(top_centers, np.float64).reshape(-1, 2)
    bottom = np.asarray(bottom_centers, np.float64).reshape(-1, 2)
    if not len(top) or not len(bottom):
        return None
    paired = np.array([int(np.argmin([np.linalg.norm(t - b) for b in bottom])) for t in top])
    dy, dx = top[0] - bottom[0]
    if abs(dy) > abs(dx):
        rotation, key = (None, top[:, 0]) if dy < 0 else (180, -top[:, 0])
        bottom_key = bottom[paired, 0] if dy < 0 else -bottom[paired, 0]
    elif dx < 0:
        rotation, key, bottom_key = 270, top[:, 1], bottom[paired, 1]
    elif dx > 0:
        rotation, key, bottom_key = 90, -top[:, 1], -bottom[paired, 1]
    else:
        return None
    return (np.argsort(key, kind='stable').tolist(), paired[np.argsort(bottom_key, kind='stable')].tolist(), rotation)


def line_boxes(top_boxes, bottom_boxes, top_ids, bottom_ids):
    """_func1 (interpreter.py:494-502): per line (y0, x0, height, width) of the union of its two components' boxes
    (boxes: y0, y1, x0, x1, half-open)"""
    result = []
    for t, b in zip(top_ids, bottom_ids):
        (ty0, ty1, tx0, tx1), (by0, by1, bx0, bx1) = top_boxes[t], bottom_boxes[b]
        y0, y1, x0, x1 = min(ty0, by0), max(ty1, by1), min(tx0, bx0), max(tx1, bx1)
        result.append((int(y0), int(x0), int(y1 - y0), int(x1 - x0)))
    return result


def label_page(who, mask, arrays, max_components):
    """What both paragraph stages do first: mask and arrays go to the device and are checked (`who`: the stage's name in
    the messages), the mask is labelled at its mean (label_layer).  Returns (arrays, components, number of paragraphs)."""
    mask = ops.as_device(mask)
    if mask.ndim != 4 or mask.shape[0] != 1 or mask.shape[3] != 1:
        raise ValueError(f'{who}: the mask must have shape (1, H, W, 1), got {mask.shape} '
                         f'(the reference labels one page at a time, datasets.py:18,39)')
    arrays = [ops.as_device(a) for a in arrays]
    for a in arrays:
        if a.ndim != 4 or a.shape[:3] != mask.shape[:3]:
            raise ValueError(f'{who}: array {a.shape} does not match the mask {mask.shape}')
    components = ops.label_components(mask, 'mean', max_components)
    return arrays, components, int(components.count[0])


def nest_like(flat, nested):
    """the next items of `flat` (a list, or an iterator that several calls draw from), one per item of every list of
    `nested`, in `nested`'s nesting"""
    items = iter(flat)
    return [[next(items) for _ in inner] for inner in nested]


class CropParagraphs:
    def __init__(self, find_rotation=False, max_components=4096):
        if find_rotation:
            raise NotImplementedError(
                'CropParagraphs(find_rotation=True): the rotation search (interpreter.py:316-333, a ternary search over '
                'ndimage.rotate of the paragraph mask) is not part of this class: use CropAndRotateParagraphs, or '
                'find_rotation=False')
        self.max_components = max_components

    def angles_of(self, components, paragraphs):
        """the angle (degrees, or None) every paragraph is turned by: here none is"""
        return [None] * paragraphs

    def __call__(self, mask, arrays, divisible_by=None):
        """mask: (1, H, W, 1) DeviceArray, arrays: list of (1, H, W, C) DeviceArrays.  Returns
        result[array_id][paragraph_id], paragraphs in scipy's label order.  divisible_by=(y, x) adds the zero frame of
        make_divisible_by (my_model/model.py:26-34), which the reference applies to every crop right after this stage.
        Every paragraph is turned by its angle (self.angles[p] afterwards: degrees, or None for a paragraph cut upright);
        a paragraph whose rotated mask has no set pixel -- the reference raises there -- is cut upright too."""
        arrays, components, paragraphs = label_page(type(self).__name__, mask, arrays, self.max_components)
        angles = self.angles_of(components, paragraphs)
        rotated = [p for p in range(paragraphs) if angles[p] is not None]
        regions = {}
        if rotated:
            extents = ops.rotated_extent(components, 0, [(p + 1, angles[p]) for p in rotated])
            regions = {p: tuple(int(v) for v in extent) for p, extent in zip(rotated, extents) if extent[1] > extent[0]}
        for p in rotated:
            if p not in regions:
                angles[p] = None
        self.angles = angles
        turned = iter(ops.rotate_crop([(a, components, 0, p + 1, angles[p], regions[p]) for a in arrays for p in sorted(regions)],
                                      divisible_by) if regions else [])
        return [[next(turned) if p in regions else ops.masked_crop(a, components, 0, p + 1, divisible_by)
                 for p in range(paragraphs)] for a in arrays]


def search_steps(eps=1.0):
    """The ternary search of CropAndRotateSingleParagraph._func (interpreter.py:321-336) as a generator: it yields the two
    probe angles (a, b) of a round, is sent their heights (height_a, height_b), and returns the angle -- None outside
    [eps, 180 - eps] -- through StopIteration.  The interval shrinks to two thirds per round whatever the heights: 13
    rounds at eps = 1."""
    low, high = 0.0, 180.0
    while high - low > eps:
        a = low + (high - low) / 3
        b = high - (high - low) / 3
        height_a, height_b = yield a, b
        if height_a < height_b:
            high = b
        else:
            low = a
    angle = (high + low) / 2
    return angle if eps <= angle <= 180.0 - eps else None


def search_angle(height_of, eps=1.0):
    """interpreter.py:321-336 for one paragraph: height_of(angle) is the height of the paragraph's mask rotated by
    `angle` degrees at order 0 (FindObjectHeightInRotated._func, :228-231).  Returns the angle in degrees, or None."""
    steps = search_steps(eps)
    try:
        a, b = next(steps)
        while True:
            a, b = steps.send((height_of(a), height_of(b)))
    except StopIteration as done:
        return done.value


class CropAndRotateParagraphs(CropParagraphs):
    def __init__(self, find_rotation=True, eps=1.0, max_components=4096, search='host'):
        """search: 'host' walks the rounds on the host (find_angles), 'device' leaves them to ONE rotation_search call;
        an eps whose tree the device cannot walk (nn/ops.py: search_table) keeps to the host search."""
        if search not in ('host', 'device'):
            raise ValueError(f"CropAndRotateParagraphs: search must be 'host' or 'device', got {search!r}")
        self.find_rotation, self.eps, self.max_components, self.search = find_rotation, eps, max_components, search
        if search == 'device' and find_rotation:
            try:
                ops.search_table(eps)
            except ValueError:
                self.search = 'host'

    def find_angles(self, components, paragraphs):
        """the reference's angle (degrees, or None) of paragraphs 1..`paragraphs` of image 0: all searches in lock step,
        one rotated_extent call per round.  A probe without a set pixel has height 0 (the reference raises there)."""
        searches = [search_steps(self.eps) for _ in range(paragraphs)]
        angles, probes, order, heights = [None] * paragraphs, {}, range(paragraphs), None
        while True:
            for i, p in enumerate(order):      # every search still running gets its two heights (None: it starts)
                try:
                    probes[p] = searches[p].send(heights and (heights[2 * i], heights[2 * i + 1]))
                except StopIteration as done:
                    angles[p] = done.value
                    probes.pop(p, None)
            if not probes:
                return angles
            order = sorted(probes)
            extents = ops.rotated_extent(components, 0, [(p + 1, angle) for p in order for angle in probes[p]])
            heights = [int(y1 - y0) for y0, y1, _, _ in extents]

    def angles_of(self, components, paragraphs):
        """the angles of the search, walked on the host or by the device"""
        if not self.find_rotation or not paragraphs:
            return [None] * paragraphs
        if self.search == 'device':
            return list(ops.rotation_search(components, 0, range(1, paragraphs + 1), self.eps)[0])
        return self.find_angles(components, paragraphs)


class CropLines:
    def __init__(self, zoomed_height=CHAR_INPUT_HEIGHT, minimal_width=CHAR_FIXED_WIDTH, max_components=4096,
                 labelling='paragraph'):
        """labelling: 'paragraph' labels the two masks of every paragraph in calls of their own, 'page' the masks of all
        paragraphs in ONE label_batch call"""
        if labelling not in ('paragraph', 'page'):
            raise ValueError(f"CropLines: labelling must be 'paragraph' or 'page', got {labelling!r}")
        self.zoomed_height, self.minimal_width = zoomed_height, minimal_width    # (None: no zoom / no padding, :511, :516)
        self.max_components, self.labelling = max_components, labelling

    def find_lines(self, masks):
        """per paragraph (rotation, [(y0, x0, height, width) per line in reading order]) from masks[p]: (1, H, W, 2);
        (None, []) for a paragraph where the reference would raise"""
        if self.labelling == 'page':
            entries = [(mask, channel) for mask in masks for channel in (0, 1)]
            both = ops.label_batch(entries, 'mean_max', self.max_components)
            tables = [(top.center_of_mass, top.boxes, bottom.center_of_mass, bottom.boxes)
                      for top, bottom in zip(both[0::2], both[1::2])]
        else:
            components = []
            for mask in masks:
                _, h, w, _ = mask.shape
                top, bottom = ops.split(mask, [(1, h, w, 1), (1, h, w, 1)])
                components.append((ops.label_components(top, 'mean_max', self.max_components),
                                   ops.label_components(bottom, 'mean_max', self.max_components)))
            tables = [(top.center_of_mass[0], top.boxes[0], bottom.center_of_mass[0], bottom.boxes[0])
                      for top, bottom in components]                # (the component tables: the only host traffic)
        found = []
        for top_centers, top_boxes, bottom_centers, bottom_boxes in tables:
            arranged = arrange_lines(top_centers, bottom_centers)
            if arranged is None:
                found.append((None, []))
            else:
                top_ids, bottom_ids, rotation = arranged
                found.append((rotation, line_boxes(top_boxes, bottom_boxes, top_ids, bottom_ids)))
        return found

    def __call__(self, masks, arrays):
        """masks[p]: (1, H, W, 2) DeviceArrays, line_top in channel 0 and line_bottom in channel 1; arrays[a][p]:
        (1, H, W, C) DeviceArrays of the same H, W.  Returns result[a][p][line], the nesting of the reference, every
        line (1, zoomed_height, >= minimal_width, C), lines in reading order.  Where the reference would raise -- a
        paragraph without a line_top component, without a line_bottom component, or whose first top and first bottom
        share a centre -- the paragraph yields no lines.  One kernel call for the page."""
        masks = [ops.as_device(m) for m in masks]
        arrays = [[ops.as_device(a) for a in per_array] for per_array in arrays]
        for mask in masks:
            if mask.ndim != 4 or mask.shape[0] != 1 or mask.shape[3] != 2:
                raise ValueError(f'CropLines: a mask must have shape (1, H, W, 2) -- line_top, line_bottom -- got {mask.shape}')
        for per_array in arrays:
            if len(per_array) != len(masks):
                raise ValueError(f'CropLines: {len(per_array)} arrays for {len(masks)} masks (one per paragraph)')
            for a, mask in zip(per_array, masks):
                if a.ndim != 4 or a.shape[:3] != mask.shape[:3]:
                    raise ValueError(f'CropLines: array {a.shape} does not match the mask {mask.shape}')
        found = self.find_lines(masks)
        entries = [(per_array[p], y0, x0, bh, bw, QUARTER_TURNS[rotation])
                   for per_array in arrays for p, (rotation, boxes) in enumerate(found) for y0, x0, bh, bw in boxes]
        crops = iter(ops.line_crop(entries, self.zoomed_height, self.minimal_width))
        return [nest_like(crops, [boxes for _, boxes in found]) for _ in arrays]


class LabelChars:
    def __init__(self, bits=None, n_chars=None):
        from . import model
        self.bits = model.BITS_COUNT if bits is None else bits
        self.n_chars = model.N_CHARS if n_chars is None else n_chars

    def __call__(self, arrays):
        """arrays[paragraph][line]: (1, H, W, C) DeviceArrays.  Returns the labels, (W, n_chars) each, in the same nesting
        (a paragraph without lines stays [], a page without paragraphs []); one kernel call for the page."""
        flat = [ops.as_device(line) for paragraph in arrays for line in paragraph]
        return nest_like(ops.char_label(flat, self.bits, self.n_chars), arrays)


def _alphabet(first, yo):
    """the 33 letters from code point `first` on with `yo` in its place after the sixth (Unicode keeps it apart)"""
    letters = [chr(first + i) for i in range(32)]
    return ''.join(letters[:6] + [yo] + letters[6:])


# the reference's character table (primitives/__init__.py:6-13), restated: tab, space, the Cyrillic lower and upper case
# alphabets, the digits, the Latin ones, ASCII punctuation.  The position of a character is its class in the Char net.
CYRILLIC_LOWER, CYRILLIC_UPPER = _alphabet(0x430, '\u0451'), _alphabet(0x410, '\u0401')
CHARS = '\t ' + CYRILLIC_LOWER + CYRILLIC_UPPER + string.digits + string.ascii_lowercase + string.ascii_uppercase + string.punctuation
# the look-alike pairs (primitives/__init__.py:16-37) as positions in CHARS: (Cyrillic, Latin)
SIMILAR_PAIRS = (
    (2, 78), (7, 82), (17, 92), (19, 93), (20, 80), (22, 102), (24, 101),                      # a e o p c y x
    (35, 104), (37, 105), (40, 108), (46, 114), (48, 116), (50, 118), (49, 111), (52, 119),    # A B E K M O H P
    (53, 106), (54, 123), (57, 127))                                                           # C T X


def pair_classes(pairs=SIMILAR_PAIRS, n_chars=len(CHARS)):
    """cls[id] = the index of the pair that id belongs to, -1 for an id without a pair"""
    cls = np.full(n_chars, -1, np.int32)
    for index, pair in enumerate(pairs):
        for char_id in pair:
            assert cls[char_id] == -1, 'a character lies in one pair at most'
            cls[char_id] = index
    return cls


def pred_to_text_rules(prediction, cls=None):
    """PredToText._func1 (interpreter.py:596-614) restated: the ids emitted for one prediction (W, n_chars), as a list.
    1. the maximum of every row; a row whose maximum == 0 (-0.0 too) contributes nothing
    2. every column that equals its row's maximum is a candidate -- none in a row with a NaN --, by row, then by column
    3. the walk: id 0 forgets the remembered id; an id whose pair holds the remembered id is skipped; every other id is
       emitted and remembered
    cls: the pair index of every id (default: the 18 pairs of CHARS)."""
    prediction = np.asarray(prediction)
    cls = pair_classes() if cls is None else np.asarray(cls)
    with np.errstate(invalid='ignore'):
        maxima = np.max(prediction, axis=1)
        candidates = (prediction == maxima[:, None]) & (maxima != 0.0)[:, None]
    emitted, remembered = [], None
    for _, char_id in np.argwhere(candidates).tolist():
        if char_id == 0:
            remembered = None
        elif remembered is None or cls[char_id] < 0 or cls[remembered] != cls[char_id]:
            emitted.append(char_id)
            remembered = char_id
    return emitted


def adjacent_rule(candidates, cls):
    """what the device evaluates instead of the walk: candidate i is emitted iff it is not the tab and not (paired, with
    a candidate before it that is not the tab and lies in the same pair)"""
    s = list(candidates)
    return [cur for i, cur in enumerate(s)
            if cur != 0 and not (cls[cur] >= 0 and i > 0 and s[i - 1] != 0 and cls[s[i - 1]] == cls[cur])]


class PredToText:
    def __init__(self, chars=CHARS, pairs=SIMILAR_PAIRS):
        self.chars, self.cls = chars, pair_classes(pairs, len(chars))

    def __call__(self, predictions):
        """predictions[paragraph][line]: (W, n_chars) DeviceArrays, the Char net's raw output.  Returns the text of every
        line as a str in the same nesting (a paragraph without lines stays [], a page without paragraphs []); one kernel
        call for the page, two when a row holds a tie."""
        flat = [ops.as_device(line) for paragraph in predictions for line in paragraph]
        return nest_like((''.join(self.chars[i] for i in ids) for ids in ops.pred_to_text(flat, self.cls)), predictions)


def canonical_ids(pairs=SIMILAR_PAIRS, n_chars=len(CHARS), similar=True):
    """canon[id] for ScoreText: the id itself, and with similar=True the Cyrillic member of its look-alike pair for both
    members: two ids match when their entries are equal"""
    canon = np.arange(n_chars, dtype=np.int32)
    if similar:
        for cyrillic, latin in pairs:
            canon[latin] = cyrillic
    return canon


class ScoreText:
    def __init__(self, chars=CHARS, pairs=SIMILAR_PAIRS, similar=True):
        self.chars, self.canon = chars, canonical_ids(pairs, len(chars), similar)

    def __call__(self, predictions, labels):
        """predictions[paragraph][line], labels[paragraph][line]: (W, n_chars) DeviceArrays, the Char net's raw output and
        the labels of the same columns.  Returns (scores, read_text, expected_text) in the same nesting: per line the
        ints (distance, expected length, read length) and the two readings as str (a paragraph without lines stays [],
        a page without paragraphs []); one kernel call and one readback for the page."""
        if [len(paragraph) for paragraph in predictions] != [len(paragraph) for paragraph in labels]:
            raise ValueError(f'ScoreText: predictions for {[len(p) for p in predictions]} lines per paragraph, labels for '
                             f'{[len(p) for p in labels]}')
        flat = lambda nested: [ops.as_device(line) for paragraph in nested for line in paragraph]
        scores, read, expected = ops.text_score(flat(predictions), flat(labels), self.canon, want_ids=True)
        text = lambda ids: ''.join(self.chars[i] for i in ids)
        return (nest_like((tuple(int(v) for v in row) for row in scores), predictions),
                nest_like(map(text, read), predictions), nest_like(map(text, expected), predictions))


# the rule each mask net's reader applies, and the cap of its score: Monochrome's 0.5 is foreground against foreground
MASK_RULES = {'monochrome': (0.5, 0), 'paragraph': ('mean', 64), 'line': ('mean_max', 64)}


class ScoreMasks:
    def __init__(self, rules=MASK_RULES):
        self.rules = dict(rules)

    def __call__(self, net, prediction, truth):
        """prediction, truth: (1, H, W, C) DeviceArrays of the net `net` of self.rules.  Returns [MaskScore per channel]:
        every channel of both thresholded by the net's rule, on its own (a labelling call and an overlap call per net)."""
        threshold, cap = self.rules[net]
        prediction, truth = ops.as_device(prediction), ops.as_device(truth)
        if prediction.shape != truth.shape:
            raise ValueError(f'ScoreMasks: {net}: a prediction of shape {prediction.shape} for a truth of shape {truth.shape}')
        return ops.mask_score([((prediction, c), (truth, c)) for c in range(prediction.shape[3])], threshold, cap=cap)
