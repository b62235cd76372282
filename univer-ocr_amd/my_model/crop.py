"""The stages that sit between the nets, on the device.

CropParagraphs is the reference's CropAndRotateParagraphs (interpreter/interpreter.py:351-378) with
`find_rotation=False`: label the paragraph layer (label_layer, :16-21), take one bounding box per component
(ndimage.find_objects, :303) and cut every companion array to it, zeroed outside the component (:304-308).  With no
rotation angle `_func` (:314-348) hands the crops back unchanged, so that is the whole stage.  Arrays stay in HBM: the
labelling, the boxes and the crops are kernels of libuniver_hip.so (nn/ops.py: label_components, masked_crop); the only
thing the host reads is the component table (64 bytes per paragraph).  There is no worker pool.

LabelChars is the reference's LabelChar (interpreter/interpreter.py:524-571): the `char` layer tag of every cropped line
-- bit layers first, then letter_spacing -- becomes the (W, N_CHARS) one-hot labels the Char net trains on.  Per line:
threshold at (mean + max) / 2 of the whole array, read every pixel's bits as a class number (least significant bit
first; a number that is no class is "unknown"), let every column vote over its rows (the first candidate from the top
wins a tie, "unknown" is one candidate) and write a one-hot row, or a zero row where "unknown" won.  The reference does
this in a Python loop per pixel on a worker pool, between a device-to-host and a host-to-device copy of every line; here
all lines of all paragraphs of a page are ONE kernel call (nn/ops.py: char_label) and nothing leaves HBM.
"""
from ..nn import ops


class CropParagraphs:
    def __init__(self, find_rotation=False, max_components=4096):
        if find_rotation:
            raise NotImplementedError(
                'CropParagraphs(find_rotation=True): the rotation search (interpreter.py:316-333, a ternary search over '
                'ndimage.rotate of the paragraph mask) has no device kernel; use find_rotation=False')
        self.max_components = max_components

    def __call__(self, mask, arrays, divisible_by=None):
        """mask: (1, H, W, 1) DeviceArray, arrays: list of (1, H, W, C) DeviceArrays.  Returns
        result[array_id][paragraph_id], paragraphs in scipy's label order.  divisible_by=(y, x) adds the zero frame of
        make_divisible_by (my_model/model.py:26-34), which the reference applies to every crop right after this stage."""
        mask = ops.as_device(mask)
        if mask.ndim != 4 or mask.shape[0] != 1 or mask.shape[3] != 1:
            raise ValueError(f'CropParagraphs: the mask must have shape (1, H, W, 1), got {mask.shape} '
                             f'(the reference labels one page at a time, datasets.py:18,39)')
        arrays = [ops.as_device(a) for a in arrays]
        for a in arrays:
            if a.ndim != 4 or a.shape[:3] != mask.shape[:3]:
                raise ValueError(f'CropParagraphs: array {a.shape} does not match the mask {mask.shape}')
        components = ops.label_components(mask, 'mean', self.max_components)
        paragraphs = int(components.count[0])
        return [[ops.masked_crop(a, components, 0, k, divisible_by) for k in range(1, paragraphs + 1)] for a in arrays]


class LabelChars:
    def __init__(self, bits=None, n_chars=None):
        from . import model
        self.bits = model.BITS_COUNT if bits is None else bits
        self.n_chars = model.N_CHARS if n_chars is None else n_chars

    def __call__(self, arrays):
        """arrays[paragraph][line]: (1, H, W, C) DeviceArrays.  Returns the labels, (W, n_chars) each, in the same nesting
        (a paragraph without lines stays [], a page without paragraphs []); one kernel call for the page."""
        flat = [ops.as_device(line) for paragraph in arrays for line in paragraph]
        labels = iter(ops.char_label(flat, self.bits, self.n_chars))
        return [[next(labels) for _ in paragraph] for paragraph in arrays]
