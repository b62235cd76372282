"""How well a page was read: the systems of my_model/model.py: make_evaluate_system over the pages of a generator, the
scores of all lines added up (the reference has nothing of the kind: its nn/metrics.py is a stub).  The character error
rate is the edit distance between what the labels of the crops say and what the Char net read, over the length of the
former; `coverage` says how much of the typed text the crop stages found at all, which the error rate alone would hide.
`--masks` scores the three nets in front of the Char net instead (make_mask_evaluate_system), each on its true input: per
net and channel the pixel precision / recall / F1 / IoU and how many of the true components the prediction found under the
threshold of the stage that reads it -- a Paragraph net that joins two paragraphs loses a few pixels and half of the text.

    python -m univer_ocr_amd.my_model.evaluate [--weights model_weights.json] [--pages 8] [--seed 1234]
        [--height 256 --width 512] [--predicted-crops] [--distinct-look-alikes] [--device-search] [--page-line-labels]
        [--page-char-pass]
    python -m univer_ocr_amd.my_model.evaluate --masks [--weights model_weights.json] [--pages 8] [--seed 1234]
        [--height 256 --width 512]
"""
import json
from collections import namedtuple

from .model import (CHAR_INPUT_HEIGHT, MASK_NETS, make_evaluate_context_maker, make_evaluate_system,
                    make_mask_evaluate_context_maker, make_mask_evaluate_system)
from .predict import add_option_flags, flag_options, read_weights

TextReport = namedtuple('TextReport', 'pages lines exact_lines typed_chars expected_chars read_chars distance cer coverage')

MaskReport = namedtuple('MaskReport', 'pages tp fp fn tn expected predicted matched overflow precision recall f1 accuracy iou '
                                      'found spurious mean_matched_iou')


def load_evaluate_system(input_shape, weights_path=None, crops='true', **options):
    """make_evaluate_system with the weights of `weights_path` (a model_weights.json); a missing file, or none, leaves the
    fresh weights in place (as my_model/predict.py: load_model_system)"""
    return make_evaluate_system(input_shape, weights=read_weights(weights_path), crops=crops, **options)[0]


def evaluate_text(pages, n_pages, model_system=None, weights_path=None, crops='true', contexts=None, **options):
    """Pages 0 .. n_pages - 1 of `pages`, a PagesWithText, through `model_system` (default: load_evaluate_system for the
    pages' size, `options` to make_evaluate_system), one `predict` per page.  Returns the TextReport of all their lines:
    typed_chars from pages.texts(i), expected_chars / read_chars / distance the sums of the lines' scores, exact_lines
    the lines at distance 0, cer = distance / expected_chars (None where that is 0), coverage = expected_chars /
    typed_chars (None where that is 0).  contexts: a list that receives every page's context."""
    height, width = pages.source.height, pages.source.width
    if crops == 'predicted' and (height % 16 or width % 16):
        raise ValueError(f'evaluate_text: the nets take pages whose sides are multiples of 16, got {height} x {width}')
    if model_system is None:
        shape = (1, CHAR_INPUT_HEIGHT, 64, 1) if crops == 'true' else (1, height, width, 1)
        model_system = load_evaluate_system(shape, weights_path, crops, **options)
    make_context = make_evaluate_context_maker(crops)
    lines = exact = typed = expected = read = distance = 0
    for index in range(int(n_pages)):
        context = make_context(pages.get, (index,))
        model_system.predict(context)
        if contexts is not None:
            contexts.append(context)
        typed += sum(len(line) for paragraph in pages.texts(index) for line in paragraph)
        for d, n_expected, n_read in (score for paragraph in context['text_scores'] for score in paragraph):
            lines, exact = lines + 1, exact + (d == 0)
            expected, read, distance = expected + n_expected, read + n_read, distance + d
    return TextReport(int(n_pages), lines, exact, typed, expected, read, distance,
                      distance / expected if expected else None, expected / typed if typed else None)


def mask_report(pages, scores):
    """the MaskReport of the MaskScores of one net's channel on `pages` pages: the ints added up, every ratio taken from
    the sums (never a mean of the pages' ratios): precision, recall, f1, accuracy, iou as ops.mask_numbers has them, found =
    matched / expected, spurious = 1 - matched / predicted, mean_matched_iou over all matched components; None where a
    denominator is 0"""
    from ..nn.ops import mask_numbers
    scores = list(scores)
    tp, fp, fn, tn, expected, predicted, matched, overflow = (sum(score[k] for score in scores) for k in range(8))
    ious = [inter / (area + other - inter) for score in scores for area, best, inter, other in score.rows
            if best > 0 and 2 * inter > area + other - inter]
    return MaskReport(int(pages), tp, fp, fn, tn, expected, predicted, matched, overflow, *mask_numbers(tp, fp, fn, tn),
                      matched / expected if expected else None, 1 - matched / predicted if predicted else None,
                      sum(ious) / len(ious) if ious else None)


def evaluate_masks(pages, n_pages, model_system=None, weights_path=None, contexts=None, make_context=None, **options):
    """Pages 0 .. n_pages - 1 of `pages`, a dataset of pages with their label layers, through `model_system` (default:
    make_mask_evaluate_system for the pages' size with the weights of `weights_path`, `options` to it), one `predict` per
    page.  Returns {net: [MaskReport per channel]} for the nets 'monochrome', 'paragraph', 'line' (mask_report).
    make_context: what turns (pages.get, (index,)) into a page's context (default: make_mask_evaluate_context_maker());
    contexts: a list that receives every page's context."""
    if model_system is None:
        height, width = pages.source.height, pages.source.width
        if height % 16 or width % 16:
            raise ValueError(f'evaluate_masks: the nets take pages whose sides are multiples of 16, got {height} x {width}')
        model_system = make_mask_evaluate_system((1, height, width, 1), weights=read_weights(weights_path), **options)[0]
    make_context = make_mask_evaluate_context_maker() if make_context is None else make_context
    filed = {net: [] for net in MASK_NETS}
    for index in range(int(n_pages)):
        context = make_context(pages.get, (index,))
        model_system.predict(context)
        if contexts is not None:
            contexts.append(context)
        for net in MASK_NETS:
            filed[net].append(context['mask_scores'][net])
    return {net: [mask_report(n_pages, channel) for channel in zip(*per_page)] for net, per_page in filed.items()}


def main(argv=None):
    import argparse

    from ..nn.gpu import CP
    from .pages import GeneratedPages, PagesWithText
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    parser.add_argument('--weights', default=None, help='model_weights.json (default: fresh weights)')
    parser.add_argument('--pages', type=int, default=8, help='pages with text to read')
    parser.add_argument('--seed', type=int, default=1234, help='the stream of the page generator')
    parser.add_argument('--height', type=int, default=256)
    parser.add_argument('--width', type=int, default=512)
    parser.add_argument('--masks', action='store_true',
                        help='score the Monochrome, Paragraph and Line nets on their true inputs instead of the Char net: '
                             'pixel numbers and found components per net and channel')
    parser.add_argument('--predicted-crops', action='store_true',
                        help='end to end: paragraphs and lines as the nets find them, not the true layers')
    parser.add_argument('--distinct-look-alikes', action='store_true',
                        help='the halves of a Cyrillic / Latin look-alike pair count as different characters')
    add_option_flags(parser)
    args = parser.parse_args(argv)
    CP.use_gpu()
    pages = PagesWithText(GeneratedPages(1, args.height, args.width, seed=args.seed, length=args.pages), args.pages)
    if args.masks:
        reports = evaluate_masks(pages, args.pages, weights_path=args.weights)
        print(json.dumps({net: [report._asdict() for report in channels] for net, channels in reports.items()}))
        return reports
    report = evaluate_text(pages, args.pages, weights_path=args.weights, crops='predicted' if args.predicted_crops else 'true',
                           similar=not args.distinct_look_alikes, **flag_options(args))
    print(json.dumps(report._asdict()))
    return report


if __name__ == '__main__':
    main()
