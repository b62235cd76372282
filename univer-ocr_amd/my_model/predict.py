"""A page in, text out (reference: my_model/predict.py): the PREDICT system of my_model/model.py: make_predict_system
on one page.  Image file input stays with the caller: `predict_text` takes the page as an array,
`main` an .npy file.

    python -m univer_ocr_amd.my_model.predict page.npy [--weights model_weights.json] [--device-search] [--page-line-labels]
        [--page-char-pass]
"""
import json

import numpy as np

from ..nn.gpu import CP
from .model import make_divisible_by, make_predict_system


def read_weights(weights_path):
    """the weights of `weights_path` (a model_weights.json); a missing file, or none, gives {}: the fresh weights stay"""
    if weights_path is not None:
        try:
            with open(weights_path) as fp:
                return json.load(fp)
        except OSError:
            print(f'No {weights_path} file found')
    return {}


def load_model_system(input_shape, weights_path=None, **options):
    """predict.py:12-23: the PREDICT system with the weights of `weights_path` (a model_weights.json); a missing file,
    or none, leaves the fresh weights in place.  options: find_rotation, rotation_search, line_labelling and char_batching
    of make_predict_system, which holds their defaults."""
    return make_predict_system(input_shape, weights=read_weights(weights_path), **options)[0]


def predict_text(image, model_system=None, weights_path=None, find_rotation=True, context=None, rotation_search='host',
                 line_labelling='paragraph', char_batching='line'):
    """predict.py:48-59: `image` is one page, (1, H, W, 1) with values in [0, 1] as the reference's encode_X leaves
    them.  It is framed to multiples of 16 (make_divisible_by), moved to the device and run through `model_system`
    (default: load_model_system for the framed shape).  Returns context['text']: text[paragraph][line], a str each.
    context: a dict to run in, for whoever wants to look at the stages' results afterwards."""
    image = np.asarray(image, dtype=np.float64)
    if image.ndim != 4 or image.shape[0] != 1 or image.shape[3] != 1:
        raise ValueError(f'predict_text: the page must have shape (1, H, W, 1), got {image.shape}')
    X = make_divisible_by(image, 16, 16)
    if model_system is None:
        # (char_batching travels only when it is set: whoever stands in for load_model_system keeps the arguments it knows)
        packed = {} if char_batching == 'line' else {'char_batching': char_batching}
        model_system = load_model_system(X.shape, weights_path, find_rotation=find_rotation, rotation_search=rotation_search,
                                         line_labelling=line_labelling, **packed)
    context = {} if context is None else context
    context['monochrome_X'] = CP.copy(X)
    model_system.predict(context)
    return context['text']


def add_option_flags(parser):
    """the flags of the three options that have one, for this command line and my_model/evaluate.py's"""
    parser.add_argument('--device-search', action='store_true',
                        help='the angle search of the paragraphs in one call on the device, not round by round on the host')
    parser.add_argument('--page-line-labels', action='store_true',
                        help='the line masks of all paragraphs of the page labelled in one call, not paragraph by paragraph')
    parser.add_argument('--page-char-pass', action='store_true',
                        help='the Char net once per page on all lines laid side by side, not once per line')


def flag_options(args):
    """the options that the flags of add_option_flags stand for"""
    return {'rotation_search': 'device' if args.device_search else 'host',
            'line_labelling': 'page' if args.page_line_labels else 'paragraph',
            'char_batching': 'page' if args.page_char_pass else 'line'}


def main(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    parser.add_argument('page', help='.npy file holding the page: (H, W) or (1, H, W, 1), values in [0, 1]')
    parser.add_argument('--weights', default=None, help='model_weights.json (default: fresh weights)')
    parser.add_argument('--no-rotation', action='store_true', help='cut the paragraphs upright, without the rotation search')
    add_option_flags(parser)
    args = parser.parse_args(argv)
    page = np.load(args.page, allow_pickle=False)
    if page.ndim == 2:
        page = page[None, :, :, None]
    CP.use_gpu()
    for paragraph in predict_text(page, weights_path=args.weights, find_rotation=not args.no_rotation, **flag_options(args)):
        for line in paragraph:
            print(line)
        print()


if __name__ == '__main__':
    main()
