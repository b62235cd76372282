"""Kernel wrappers: DeviceArray in, DeviceArray out, every byte of arithmetic in libuniver_hip.so.

This is the seam that replaces the reference's per-layer `_forward_gpu/_backward_gpu` closures
(layers/layers.py:169-197) and its CuPy expressions.  Output shapes follow the reference's
get_output_shapes; arrays returned are always NEW allocations, as in the reference.
"""
import ctypes as C
import math
from collections import namedtuple

import numpy as np

from ..hip import lib as hiplib
from ..hip.lib import HipError
from .gpu import CP, DeviceArray, DeviceScalar

ACT_CODES = {None: hiplib.ACT_NONE, 'relu': hiplib.ACT_RELU, 'leaky': hiplib.ACT_LEAKY,
             'sigmoid': hiplib.ACT_SIGMOID}


def _rt():
    return CP.runtime()


def _ints(values):
    return (C.c_int * len(values))(*values)


def _pointers(arrays):
    return (C.c_void_p * len(arrays))(*[a.ptr for a in arrays])


def _flat(groups, ctype):
    values = [v for group in groups for v in group]
    return (ctype * len(values))(*values)


def _shared_code(arrays, who, what):
    """the storage dtype code of a call: the one all its arrays have"""
    code = arrays[0].code & 0xff
    if any(a.code & 0xff != code for a in arrays):
        raise ValueError(f'{who}: the arrays of one call share {what}, got ' + ', '.join(sorted({str(a.dtype) for a in arrays})))
    return code


def _same_dtype(*arrays, grad=None):
    """dtype code of a call.  The first array is an ACTIVATION tensor and decides: float32 / float64 calls need
    every array in that type; float16 calls (UOCR_F16: binary16 activations, float32 parameters) take float16
    and float32 arrays together.  `grad`: the incoming activation gradient of a backward op -- the power-of-two
    factor it carries (DeviceArray.gscale) travels in the code's scale bits (UOCR_F16_SCALED)."""
    base = arrays[0].code & 0xff
    for a in arrays[1:]:
        other = a.code & 0xff
        if other != base and not (base == hiplib.F16 and other == hiplib.F32):
            raise HipError('mixed dtypes in one op: ' + ', '.join(str(x.dtype) for x in arrays))
    if base == hiplib.F16 and grad is not None:
        return hiplib.f16_scaled(grad.gscale)
    return base


def _like_grad(array, dy):
    """`array` is the activation gradient a backward op derived from `dy`: it carries the same factor."""
    array.gscale = dy.gscale
    return array


def f16_grad_scale_log2(kind, n):
    """log2 of the factor a loss kernel gives its float16 gradient so that it sits around 2^-4 .. 1 instead of
    around 1 / n (n = pixels per image for the segmentation losses, rows for the cross-entropies), far below
    binary16's normal range for a 2-Mpixel page.  CP.f16_grad_scale_log2 overrides."""
    if CP.f16_grad_scale_log2 is not None:
        return int(CP.f16_grad_scale_log2)
    k = int(math.floor(math.log2(max(1, n)))) - (4 if kind == 'seg' else 1)
    return max(0, min(24, k))


def as_device(x):
    """Accept host arrays at the layer boundary (the reference's layers accept whatever CP.cp is)."""
    if isinstance(x, DeviceArray):
        return x
    return CP.copy(x)


# ---- Convolutional2D ---------------------------------------------------------------------------
def conv_out_hw(h, w, ks, stride, padding):
    """convolutional.py:290-301."""
    oh = math.floor((h + 2 * padding[0] - (ks[0] - 1) - 1) / stride[0] + 1)
    ow = math.floor((w + 2 * padding[1] - (ks[1] - 1) - 1) / stride[1] + 1)
    return oh, ow


def _conv_dims(x_shape, w_shape, stride, padding):
    n, h, wd, cin = x_shape
    kh, kw, wcin, cout = w_shape
    if cin != wcin:
        raise AssertionError(f'channels mismatch: input has {cin}, weights expect {wcin}')
    oh, ow = conv_out_hw(h, wd, (kh, kw), stride, padding)
    if oh <= 0 or ow <= 0:
        raise HipError(f'convolution output is empty for input {x_shape}, kernel {(kh, kw)}')
    return (n, h, wd, cin, cout, kh, kw, stride[0], stride[1], padding[0], padding[1], oh, ow)


def conv2d_fwd(x, w, b, stride, padding, pad_value=0.0, bias=True, act=None, alpha=0.0):
    dims = _conv_dims(x.shape, w.shape, stride, padding)
    code = _same_dtype(x, w, b)
    y = CP.empty((dims[0], dims[11], dims[12], dims[4]), x.dtype)
    _rt().call('uocr_conv2d_fwd', code, x.ptr, w.ptr, b.ptr, y.ptr, *dims, float(pad_value),
               int(bool(bias)), ACT_CODES[act], float(alpha))
    return y


def conv2d_bwd_data(dy, w, x_shape, stride, padding, x_act=None, act=None, alpha=0.0):
    """dx of the conv; with `x_act` (the conv's input = output of a fused LeakyReLU / Sigmoid) the
    kernel stores dx * act'(x_act), i.e. the gradient w.r.t. that activation's INPUT."""
    dims = _conv_dims(x_shape, w.shape, stride, padding)
    code = _same_dtype(dy, w, grad=dy) if x_act is None else _same_dtype(dy, w, x_act, grad=dy)
    if dy.shape != (dims[0], dims[11], dims[12], dims[4]):
        raise AssertionError(f'grad shape {dy.shape} does not match the layer output')
    if x_act is not None and x_act.shape != tuple(x_shape):
        raise AssertionError(f'activation tensor {x_act.shape} != conv input {tuple(x_shape)}')
    dx = _like_grad(CP.empty(x_shape, dy.dtype), dy)
    _rt().call('uocr_conv2d_bwd_data', code, dy.ptr, w.ptr, dx.ptr, *dims,
               None if x_act is None else x_act.ptr, ACT_CODES[act if x_act is not None else None], float(alpha))
    return dx


def conv2d_bwd_weight(x, dy, dw, db, stride, padding, pad_value=0.0, bias=True, accumulate=True):
    dims = _conv_dims(x.shape, dw.shape, stride, padding)
    code = _same_dtype(x, dy, dw, db, grad=dy)
    with _rt().side(x, dy):               # nothing on the lane reads dw before the end of the backward pass
        _rt().call('uocr_conv2d_bwd_weight', code, x.ptr, dy.ptr, dw.ptr, db.ptr, *dims, float(pad_value),
                   int(bool(bias)), int(bool(accumulate)))
    _rt().keep(x, dy)                     # (read at the flush if the call was deferred: Runtime.defer_wgrad)


def conv_pair_fwd(x, w1, b1, w2, b2, pad_value1=0.0, bias1=True, bias2=True, alpha=0.01, act2=hiplib.ACT_NONE):
    """conv3x3(1->16) + LeakyReLU + conv3x3(16->1) [+ Sigmoid] as one kernel (float32, see univer_hip.h)."""
    n, h, wd, _ = x.shape
    code = _same_dtype(x, w1, b1, w2, b2)
    y = CP.empty((n, h, wd, 1), x.dtype)
    _rt().call('uocr_conv_pair_fwd', code, x.ptr, w1.ptr, b1.ptr, w2.ptr, b2.ptr, y.ptr, n, h, wd, w1.shape[3],
               float(pad_value1), int(bool(bias1)), int(bool(bias2)), float(alpha), int(act2))
    return y


def conv_pair_bwd(x, y, dy, w1, b1, w2, dw1, db1, dw2, db2, pad_value1=0.0, bias1=True, bias2=True, alpha=0.01,
                  act2=hiplib.ACT_NONE, need_dx=True, accumulate=True):
    n, h, wd, _ = x.shape
    code = _same_dtype(x, y, dy, w1, b1, w2, dw1, db1, dw2, db2, grad=dy)
    dx = _like_grad(CP.empty(x.shape, x.dtype), dy) if need_dx else None
    _rt().call('uocr_conv_pair_bwd', code, x.ptr, y.ptr, dy.ptr, w1.ptr, b1.ptr, w2.ptr, dw1.ptr, db1.ptr, dw2.ptr,
               db2.ptr, dx.ptr if need_dx else None, n, h, wd, w1.shape[3], float(pad_value1), int(bool(bias1)),
               int(bool(bias2)), float(alpha), int(act2), int(bool(accumulate)))
    return dx


def _up_dims(x_low_shape, w_shape, padding):
    n, hl, wl, cin = x_low_shape
    kh, kw, wcin, cout = w_shape
    assert wcin == cin
    return n, hl, wl, cin, cout, kh, kw, padding[0], padding[1]


def upconv2x_fwd(x_low, w, b, padding, bias=True, act=None, alpha=0.0, weff=None):
    """Upsample2D(2) + conv (stride 1) on the low-res tensor (float32 5x5 4->4 only, see univer_hip.h).
    `weff`: a float32 array of 576 that receives the per-phase weights for upconv2x_bwd_data of the same step."""
    dims = _up_dims(x_low.shape, w.shape, padding)
    code = _same_dtype(x_low, w, b)
    y = CP.empty((dims[0], 2 * dims[1], 2 * dims[2], dims[4]), x_low.dtype)
    _rt().call('uocr_upconv2x_fwd', code, x_low.ptr, w.ptr, b.ptr, y.ptr, *dims, int(bool(bias)), ACT_CODES[act],
               float(alpha), None if weff is None else weff.ptr)
    return y


def upconv2x_bwd_data(dy, w, x_low_shape, padding, x_act=None, act=None, alpha=0.0, weff=None):
    """`weff`: what upconv2x_fwd of this layer wrote in the same step (w unchanged since), or None."""
    dims = _up_dims(x_low_shape, w.shape, padding)
    code = _same_dtype(dy, w, grad=dy)
    dx = _like_grad(CP.empty(x_low_shape, dy.dtype), dy)
    _rt().call('uocr_upconv2x_bwd_data', code, dy.ptr, w.ptr, dx.ptr, *dims, None if x_act is None else x_act.ptr,
               ACT_CODES[act if x_act is not None else None], float(alpha), None if weff is None else weff.ptr)
    return dx


def upconv2x_bwd_weight(x_low, dy, dw, db, padding, bias=True, accumulate=True):
    dims = _up_dims(x_low.shape, dw.shape, padding)
    code = _same_dtype(x_low, dy, dw, db, grad=dy)
    with _rt().side(x_low, dy):
        _rt().call('uocr_upconv2x_bwd_weight', code, x_low.ptr, dy.ptr, dw.ptr, db.ptr, *dims, int(bool(bias)),
                   int(bool(accumulate)))


# ---- MaxPool2D ------------------------------------------------------------------------------------
def pool_out_hw(h, w, ks, stride, padding, ceil_mode):
    """maxpool.py:204-216."""
    rnd = math.ceil if ceil_mode else math.floor
    return (rnd((h + 2 * padding[0] - (ks[0] - 1) - 1) / stride[0] + 1),
            rnd((w + 2 * padding[1] - (ks[1] - 1) - 1) / stride[1] + 1))


def maxpool2d_fwd(x, ks, stride, padding, ceil_mode=False):
    n, h, wd, c = x.shape
    oh, ow = pool_out_hw(h, wd, ks, stride, padding, ceil_mode)
    y = CP.empty((n, oh, ow, c), x.dtype)
    mask = CP.empty((n, ks[0] * oh, ks[1] * ow, c), np.uint8)
    _rt().call('uocr_maxpool2d_fwd', x.code, x.ptr, y.ptr, mask.ptr, n, h, wd, c, ks[0], ks[1], stride[0],
               stride[1], padding[0], padding[1], oh, ow)
    return y, mask


def maxpool2d_bwd(dy, mask, x_shape, ks, stride, padding):
    n, h, wd, c = x_shape
    oh, ow = dy.shape[1], dy.shape[2]
    dx = _like_grad(CP.empty(x_shape, dy.dtype), dy)
    _rt().call('uocr_maxpool2d_bwd', dy.code, dy.ptr, mask.ptr, dx.ptr, n, h, wd, c, ks[0], ks[1], stride[0],
               stride[1], padding[0], padding[1], oh, ow)
    return dx


# ---- Upsample2D -----------------------------------------------------------------------------------
def upsample2d_fwd(x, scale):
    n, h, wd, c = x.shape
    y = CP.empty((n, h * scale[0], wd * scale[1], c), x.dtype)
    _rt().call('uocr_upsample2d_fwd', x.code, x.ptr, y.ptr, n, h, wd, c, scale[0], scale[1])
    return y


def upsample2d_bwd(dy, x_shape, scale):
    n, h, wd, c = x_shape
    if dy.shape != (n, h * scale[0], wd * scale[1], c):
        raise AssertionError(f'grad shape {dy.shape} does not match the upsampled shape')
    dx = _like_grad(CP.empty(x_shape, dy.dtype), dy)
    _rt().call('uocr_upsample2d_bwd', dy.code, dy.ptr, dx.ptr, n, h, wd, c, scale[0], scale[1])
    return dx


# ---- activations -----------------------------------------------------------------------------------
def act_fwd(kind, x, alpha=0.0):
    y = CP.empty(x.shape, x.dtype)
    _rt().call('uocr_act_fwd', x.code, ACT_CODES[kind], float(alpha), x.ptr, y.ptr, x.size)
    return y


def act_bwd(kind, x, dy, alpha=0.0):
    code = _same_dtype(x, dy)
    if x.size != dy.size:
        raise AssertionError(f'grad size {dy.shape} != input size {x.shape}')
    dx = _like_grad(CP.empty(dy.shape, dy.dtype), dy)
    _rt().call('uocr_act_bwd', code, ACT_CODES[kind], float(alpha), x.ptr, dy.ptr, dx.ptr, x.size)
    return dx


def act_bwd_from_output(kind, y, dy, alpha=0.0):
    code = _same_dtype(y, dy)
    dx = _like_grad(CP.empty(dy.shape, dy.dtype), dy)
    _rt().call('uocr_act_bwd_from_output', code, ACT_CODES[kind], float(alpha), y.ptr, dy.ptr, dx.ptr, y.size)
    return dx


# ---- FullyConnected ---------------------------------------------------------------------------------
def dense_fwd(x, w, act=None, alpha=0.0):
    """y = act([x, 1] . w): `act` is the LeakyRelu / Sigmoid that follows the layer (None: plain dense)."""
    m, n_in = x.shape
    if w.shape[0] != n_in + 1:
        raise AssertionError(f'weights {w.shape} do not fit input {x.shape} (bias row included)')
    y = CP.empty((m, w.shape[1]), x.dtype)
    _rt().call('uocr_dense_fwd_act', _same_dtype(x, w), x.ptr, w.ptr, y.ptr, m, n_in, w.shape[1], ACT_CODES[act],
               float(alpha))
    return y


def dense_bwd(x, w, dy, dw, accumulate=True, need_dx=True, x_act=None, x_alpha=0.0):
    """`x_act`: x is the output of that (fused) activation and dx is wanted w.r.t. the activation's INPUT."""
    m, n_in = x.shape
    n_out = w.shape[1]
    code = _same_dtype(x, w, dy, dw, grad=dy)
    dx = _like_grad(CP.empty((m, n_in), dy.dtype), dy) if need_dx else None
    rt = _rt()
    if rt.side_on and need_dx:            # dw on the lane's side stream, dx (the critical path) on the lane
        with rt.side(x, dy):
            rt.call('uocr_dense_bwd_act', code, x.ptr, w.ptr, dy.ptr, None, dw.ptr, m, n_in, n_out,
                    int(bool(accumulate)), ACT_CODES[None], 0.0)
        rt.call('uocr_dense_bwd_act', code, x.ptr, w.ptr, dy.ptr, dx.ptr, None, m, n_in, n_out, 0, ACT_CODES[x_act],
                float(x_alpha))
        return dx
    rt.call('uocr_dense_bwd_act', code, x.ptr, w.ptr, dy.ptr, dx.ptr if need_dx else None, dw.ptr, m, n_in,
            n_out, int(bool(accumulate)), ACT_CODES[x_act], float(x_alpha))
    rt.keep(x, dy)
    return dx


# ---- Conv2DToBatchedFixedWidthed + Flatten + FullyConnected as ONE implicit GEMM -------------------------
# The windows layer (convolutional.py:330-373) copies every `width`-column window of (n, h, W, c) into its own
# batch entry, Flatten strings it out as (h, j, c) and the dense layer multiplies by w[(h, j, c), n_out]: that is a
# convolution with a (h, width) kernel, padding (0, width // 2) and the output cut to W columns, whose weights
# are the dense layer's rows and whose bias is its last row.  Run through the conv entry points (the implicit-GEMM
# loaders gather the windows on the fly) the 8x larger windows tensor and its gradient never exist.
def _windows_dims(x_shape, w, width):
    n, h, wd, c = x_shape
    n_in = h * width * c
    if w.shape[0] != n_in + 1:
        raise AssertionError(f'weights {w.shape} do not fit {width}-column windows of {tuple(x_shape)} (bias row included)')
    if wd < width:
        raise AssertionError(f'Input width must be >= than output width, found: {wd} < {width}')
    dims = (n, h, wd, c, w.shape[1], h, width, 1, 1, 0, width // 2, 1, wd)
    return dims, n_in * w.shape[1] * w.t.element_size()


def windows_dense_fwd(x, w, width, act=None, alpha=0.0):
    """(n, h, W, c) -> (n * W, n_out): fixed-width windows, flatten and dense (+ its activation) in one kernel."""
    dims, bias_off = _windows_dims(x.shape, w, width)
    y = CP.empty((dims[0] * dims[2], dims[4]), x.dtype)
    _rt().call('uocr_conv2d_fwd', _same_dtype(x, w), x.ptr, w.ptr, w.ptr + bias_off, y.ptr, *dims, 0.0, 1,
               ACT_CODES[act], float(alpha))
    return y


def windows_dense_bwd(x, w, dy, dw, width, accumulate=True, x_act=None, act=None, alpha=0.0):
    """dw (bias row included) and the gradient w.r.t. x (times act'(x) when x is the output of a fused
    activation, as conv2d_bwd_data)."""
    dims, bias_off = _windows_dims(x.shape, w, width)
    code = _same_dtype(x, w, dy, dw, grad=dy)
    if dy.shape != (dims[0] * dims[2], dims[4]):
        raise AssertionError(f'grad shape {dy.shape} does not match the layer output')
    with _rt().side(x, dy):
        _rt().call('uocr_conv2d_bwd_weight', code, x.ptr, dy.ptr, dw.ptr, dw.ptr + bias_off, *dims, 0.0, 1,
                   int(bool(accumulate)))
    _rt().keep(x, dy)
    dx = _like_grad(CP.empty(x.shape, dy.dtype), dy)
    _rt().call('uocr_conv2d_bwd_data', code, dy.ptr, w.ptr, dx.ptr, *dims, None if x_act is None else x_act.ptr,
               ACT_CODES[act if x_act is not None else None], float(alpha))
    return dx


# ---- Conv2DToBatchedFixedWidthed -------------------------------------------------------------------
def fixed_width_fwd(x, width):
    n, h, wd, c = x.shape
    y = CP.empty((n * wd, h, width, c), x.dtype)
    _rt().call('uocr_fixed_width_fwd', x.code, x.ptr, y.ptr, n, h, wd, c, width)
    return y


def fixed_width_bwd(dy, x_shape, width):
    n, h, wd, c = x_shape
    dx = _like_grad(CP.empty(x_shape, dy.dtype), dy)
    _rt().call('uocr_fixed_width_bwd', dy.code, dy.ptr, dx.ptr, n, h, wd, c, width)
    return dx


# ---- Concat / sums -----------------------------------------------------------------------------------
def concat(arrays, axis=-1):
    nd = arrays[0].ndim
    axis = axis % nd
    lead = arrays[0].shape[:axis]
    rows = int(np.prod(lead)) if lead else 1
    tails = [int(np.prod(a.shape[axis:])) for a in arrays]
    out_shape = list(arrays[0].shape)
    out_shape[axis] = sum(a.shape[axis] for a in arrays)
    out = CP.empty(out_shape, arrays[0].dtype)
    total = sum(tails)
    off = 0
    esz = out.t.element_size()
    for a, cols in zip(arrays, tails):
        _same_dtype(out, a)
        _rt().call('uocr_copy_2d', out.code, out.ptr + off * esz, total, a.ptr, cols, rows, cols)
        off += cols
    return out


def split(array, shapes, axis=-1):
    """Inverse of concat: slices of `array` with the given shapes along `axis` (Concat.backward)."""
    nd = array.ndim
    axis = axis % nd
    rows = int(np.prod(array.shape[:axis])) if axis else 1
    total = int(np.prod(array.shape[axis:]))
    outs, off = [], 0
    esz = array.t.element_size()
    for shp in shapes:
        cols = int(np.prod(shp[axis:]))
        out = _like_grad(CP.empty(shp, array.dtype), array)
        _rt().call('uocr_copy_2d', out.code, out.ptr, cols, array.ptr + off * esz, total, rows, cols)
        outs.append(out)
        off += cols
    return outs


def add(a, b):
    if a.shape != b.shape:
        raise AssertionError(f'cannot add {a.shape} and {b.shape}')
    if a.gscale != b.gscale:
        raise HipError(f'cannot add gradients that carry different scales (2^{a.gscale} and 2^{b.gscale})')
    out = _like_grad(CP.empty(a.shape, a.dtype), a)
    _rt().call('uocr_add', _same_dtype(a, b), a.ptr, b.ptr, out.ptr, a.size)
    return out


def axpy(alpha, x, y):
    _rt().call('uocr_axpy', _same_dtype(x, y), float(alpha), x.ptr, y.ptr, x.size)


def scale_(x, alpha):
    _rt().call('uocr_scale', x.code, float(alpha), x.ptr, x.size)


def fill_(x, value):
    _rt().call('uocr_fill', x.code, x.ptr, float(value), x.size)


def zero_(x):
    _rt().call('uocr_memset_zero', x.ptr, x.nbytes)


def u8_to_float(src_u8, scale=1.0 / 255.0, dtype=None, out=None):
    if out is None:
        out = CP.empty(src_u8.shape, CP.dtype if dtype is None else dtype)
    elif out.shape != src_u8.shape:
        raise AssertionError(f'u8_to_float: out {out.shape} != source {src_u8.shape}')
    _rt().call('uocr_u8_to_float', out.code, src_u8.ptr, out.ptr, float(scale), out.size)
    return out


# ---- losses --------------------------------------------------------------------------------------------
def _loss_slot():
    return CP.loss_slot()


def _loss_code(pred, gt, grad, kind, n):
    """dtype code of a loss call; a float16 gradient gets its power-of-two scale here (see f16_grad_scale_log2)."""
    code = _same_dtype(pred, gt)
    if code == hiplib.F16 and grad is not None:
        grad.gscale = f16_grad_scale_log2(kind, n)
        return hiplib.f16_scaled(grad.gscale)
    return code


def _finish_loss(slot):
    return DeviceScalar(slot.t) if CP.lazy_losses else float(slot.t.item())


def seg_loss(kind, pred, gt, need_grad=True, out_act=None):
    """out_act='sigmoid': pred is a Sigmoid output and the gradient is w.r.t. the Sigmoid's input."""
    n, h, w, c = pred.shape
    if gt.shape != pred.shape:
        raise AssertionError(f'ground truth {gt.shape} != prediction {pred.shape}')
    grad = CP.empty(pred.shape, pred.dtype) if need_grad else None
    slot = _loss_slot()
    _rt().call('uocr_seg_loss', _loss_code(pred, gt, grad, 'seg', h * w), hiplib.LOSS_DICE if kind == 'dice' else hiplib.LOSS_JACCARD,
               pred.ptr, gt.ptr, grad.ptr if need_grad else None, slot.ptr, n, h * w, c, ACT_CODES[out_act])
    return _finish_loss(slot), grad


def softmax_ce(pred, gt, need_grad=True):
    m, c = pred.shape
    if gt.shape != pred.shape:
        raise AssertionError(f'ground truth {gt.shape} != prediction {pred.shape}')
    grad = CP.empty(pred.shape, pred.dtype) if need_grad else None
    slot = _loss_slot()
    _rt().call('uocr_softmax_ce', _loss_code(pred, gt, grad, 'ce', m), pred.ptr, gt.ptr, grad.ptr if need_grad else None,
               slot.ptr, m, c)
    return _finish_loss(slot), grad


def sigmoid_ce(pred, gt, need_grad=True):
    if gt.shape != pred.shape:
        raise AssertionError(f'ground truth {gt.shape} != prediction {pred.shape}')
    grad = CP.empty(pred.shape, pred.dtype) if need_grad else None
    slot = _loss_slot()
    _rt().call('uocr_sigmoid_ce', _loss_code(pred, gt, grad, 'ce', gt.shape[0]), pred.ptr, gt.ptr, grad.ptr if need_grad else None,
               slot.ptr, gt.shape[0], pred.size)
    return _finish_loss(slot), grad


def regularize(kind, w, grad, strength, slot=None, accumulate=False):
    """grad += dR/dw; returns the loss (or adds it into `slot` when given)."""
    own = slot is None
    if own:
        slot = _loss_slot()
    _rt().call('uocr_l2_reg' if kind == 'l2' else 'uocr_l1_reg', _same_dtype(w, grad), w.ptr, grad.ptr, w.size,
               float(strength), slot.ptr, int(bool(accumulate)))
    return _finish_loss(slot) if own else None


# ---- optimizers ------------------------------------------------------------------------------------------
def adam_step(w, g, v, a, lr, beta1, beta2, eps):
    _rt().call('uocr_adam_step', _same_dtype(w, g, v, a), w.ptr, g.ptr, v.ptr, a.ptr, w.size, float(lr),
               float(beta1), float(beta2), float(eps))


def _range_args(ranges):
    n = len(ranges)
    lo = (C.c_longlong * max(n, 1))(*[r[1] for r in ranges])
    hi = (C.c_longlong * max(n, 1))(*[r[2] for r in ranges])
    kind = (C.c_int * max(n, 1))(*[{'l1': 1, 'l2': 2, 1: 1, 2: 2}[r[0][0]] for r in ranges])
    strength = (C.c_double * max(n, 1))(*[float(r[0][1]) for r in ranges])
    return n, lo, hi, kind, strength


def momentum_step_fused(w, g, v, lr, momentum, ranges, zero_grad=True, hyper=None):
    """Regularisers of `ranges` = [((kind, strength), lo, hi), ...] (at most 4) + Momentum update + gradient
    reset in one pass (univer_hip.h: uocr_momentum_step_fused).  Returns the regularisation loss.  `hyper`: a
    float64 DeviceArray {lr, momentum, -, -} the kernel reads instead of the by-value arguments (HIP graphs)."""
    n, lo, hi, kind, strength = _range_args(ranges)
    slot = _loss_slot() if n else None
    _rt().call('uocr_momentum_step_fused', _same_dtype(w, g, v), w.ptr, g.ptr, v.ptr, w.size, float(lr), float(momentum),
               n, lo, hi, kind, strength, slot.ptr if n else None, int(bool(zero_grad)),
               None if hyper is None else hyper.ptr)
    return _finish_loss(slot) if n else 0


def adam_step_fused(w, g, v, a, lr, beta1, beta2, eps, ranges, zero_grad=True, hyper=None):
    n, lo, hi, kind, strength = _range_args(ranges)
    slot = _loss_slot() if n else None
    _rt().call('uocr_adam_step_fused', _same_dtype(w, g, v, a), w.ptr, g.ptr, v.ptr, a.ptr, w.size, float(lr),
               float(beta1), float(beta2), float(eps), n, lo, hi, kind, strength, slot.ptr if n else None,
               int(bool(zero_grad)), None if hyper is None else hyper.ptr)
    return _finish_loss(slot) if n else 0


def momentum_step(w, g, v, lr, momentum):
    _rt().call('uocr_momentum_step', _same_dtype(w, g, v), w.ptr, g.ptr, v.ptr, w.size, float(lr), float(momentum))


def rmsprop_step(w, g, a, lr, rho, eps):
    _rt().call('uocr_rmsprop_step', _same_dtype(w, g, a), w.ptr, g.ptr, a.ptr, w.size, float(lr), float(rho),
               float(eps))


def has_nan(x):
    flag = CP.empty((1,), np.int32)
    _rt().call('uocr_has_nan', x.code, x.ptr, x.size, flag.ptr)
    return bool(flag.t.item())


# ---- connected components / masked crops (interpreter/interpreter.py: ParagraphCrop) ---------------------------------
# what the flat lists of the page-stage calls hold, as written in the messages: rank, least and most of shape[0]
_ENTRY_FORMS = {'(1, H, W, C)': (4, 1, 1), '(N, H, W, C)': (4, 0, math.inf), '(W, n_chars)': (2, 1, math.inf)}


def _check_entries(who, arrays, form='(1, H, W, C)'):
    """every array of the flat list of a page-stage call is a DeviceArray of the form the call takes"""
    ndim, least, most = _ENTRY_FORMS[form]
    for a in arrays:
        if not isinstance(a, DeviceArray) or a.ndim != ndim or not least <= a.shape[0] <= most:
            raise ValueError(f'{who}: expected {form} device arrays, got {getattr(a, "shape", type(a))}')


def _threshold_args(who, threshold):
    """(mode, value) of the labelling calls for a threshold 'mean', 'mean_max' or a number"""
    if isinstance(threshold, str):
        if threshold not in ('mean', 'mean_max'):
            raise ValueError(f"{who}: threshold must be 'mean', 'mean_max' or a number, got {threshold!r}")
        return (hiplib.THRESH_MEAN if threshold == 'mean' else hiplib.THRESH_MEAN_MAX), 0.0
    return hiplib.THRESH_VALUE, float(threshold)


def _repeat_longer(counts, rows, caps, again):
    """The second pass of a call that had room for caps[i] rows of item i and read back every item's true count: the items
    that hold more are repeated in ONE call, again(their indices, their counts) -> (counts, rows), which must count what
    the first pass counted, and their rows take the places of the cut ones in `rows`."""
    longer = [i for i, (count, cap) in enumerate(zip(counts, caps)) if count > cap]
    if longer:
        recount, full = again(longer, [int(counts[i]) for i in longer])
        assert all(recount[k] == counts[i] for k, i in enumerate(longer))
        for k, i in enumerate(longer):
            rows[i] = full[k]


class _TableViews:
    """boxes, area and center_of_mass of int64 (count, 8) tables = first pixel, area, y0, y1, x0, x1, sum of y, sum of x;
    `_view(f)` is f of the table, or of every image's"""
    boxes = property(lambda self: self._view(lambda t: t[:, 2:6]))
    area = property(lambda self: self._view(lambda t: t[:, 1]))
    center_of_mass = property(lambda self: self._view(lambda t: t[:, 6:8] / np.maximum(t[:, 1:2], 1)))


class Components(_TableViews):
    """Result of label_components.  `.labels` stays on the device; `.count`, `.boxes`, `.area` and `.center_of_mass`
    (one entry per image) come from ONE device-to-host copy of the component table and the counts, made at the first
    access.  boxes[n] is (count, 4) = y0, y1, x0, x1, half-open as scipy's find_objects slices; center_of_mass[n] is
    (count, 2) = (y, x) as ndimage.center_of_mass of each component's boolean mask."""

    def __init__(self, labels, table, count, max_components):
        self.labels = labels
        self.max_components = max_components
        self._table_dev, self._count_dev = table, count
        self._host = None

    def _fetch(self):
        if self._host is None:
            count = self._count_dev.numpy().copy()
            table = self._table_dev.numpy()
            if count.size and int(count.max()) > self.max_components:
                raise HipError(f'label_components: an image has {int(count.max())} components, more than '
                               f'max_components = {self.max_components}')
            self._host = count, [table[n, :int(c)].copy() for n, c in enumerate(count)]
        return self._host

    @property
    def count(self):
        return self._fetch()[0]

    @property
    def table(self):
        """per image: int64 (count, 8) = first pixel, area, y0, y1, x0, x1, sum of y, sum of x"""
        return self._fetch()[1]

    def _view(self, f):
        return [f(t) for t in self.table]


def label_components(x, threshold='mean', max_components=4096):
    """Connected components of x > t, x of shape (N, H, W, 1): interpreter.py:16-21 with threshold='mean' (t = mean of
    x), :437-438 / :549 with 'mean_max' (t = (mean + max) / 2), or a number.  Every image is labelled on its own."""
    if x.ndim != 4 or x.shape[3] != 1:
        raise ValueError(f'label_components: expected (N, H, W, 1), got {x.shape}')
    n, h, w, _ = x.shape
    mode, value = _threshold_args('label_components', threshold)
    max_components = int(max_components)
    labels = CP.empty((n, h, w), np.int32)
    table = CP.empty((n, max_components, 8), np.int64)
    count = CP.zeros((n,), np.int32)
    _rt().call('uocr_label_components', x.code & 0xff, x.ptr, n, h, w, mode, value, labels.ptr, table.ptr,
               max_components, count.ptr)
    return Components(labels, table, count, max_components)


class EntryComponents(_TableViews):
    """Result of label_batch for ONE entry, on the host already: `count` (an int), `table` int64 (count, 8) = first
    pixel, area, y0, y1, x0, x1, sum of y, sum of x, and `boxes` (count, 4), `area` (count,), `center_of_mass`
    (count, 2) as Components has them per image.  `labels`: the int32 (H, W) DeviceArray, or None where none was asked
    for."""

    def __init__(self, count, table, labels=None):
        self.count, self.table, self.labels = int(count), table, labels

    def _view(self, f):
        return f(self.table)


def _label_batch_call(entries, mode, value, cap, planes):
    """ONE uocr_label_batch call with room for `cap` rows per entry and ONE device-to-host copy: the counts sit at the
    head of the buffer the tables follow in.  planes: the label planes to write, or None.  Returns (counts, [the first
    min(count, cap) rows of every entry])."""
    n = len(entries)
    arrays = [a for a, _ in entries]
    head = (4 * n + 7) & ~7                                        # (the tables are int64)
    out = CP.empty((head + n * cap * 64,), np.uint8)
    _rt().call('uocr_label_batch', _shared_code(arrays, 'label_batch', 'a dtype'), n, _pointers(arrays),
               *(_ints([a.shape[d] for a in arrays]) for d in (1, 2, 3)), _ints([ch for _, ch in entries]), mode, value,
               _pointers(planes) if planes is not None else None, C.c_void_p(out.ptr + head), cap, C.c_void_p(out.ptr))
    host = out.numpy()
    counts = host[:4 * n].view(np.int32)
    tables = host[head:].view(np.int64).reshape(n, cap, 8)
    return counts, [tables[i, :min(int(count), cap)].copy() for i, count in enumerate(counts)]


def label_batch(entries, threshold='mean', max_components=4096, cap=256, labels=False):
    """Connected components of a flat list of entries (array, channel): channel `channel` of the (1, H, W, C) DeviceArray
    `array`, read in place, thresholded at its OWN mean ('mean', interpreter.py:16-21), (mean + max) / 2 ('mean_max',
    :437-438) or at a number, whatever the sizes of the entries.  Returns one EntryComponents per entry.  ONE
    uocr_label_batch call with room for `cap` components per entry and ONE device-to-host copy of the counts and those
    rows (64 bytes a row); the entries that hold more, up to max_components, are repeated in ONE second call with the
    room their counts ask for; an entry with more than max_components raises HipError.  labels=True also writes every
    entry's int32 (H, W) label plane (EntryComponents.labels).  No call for an empty list."""
    entries = [(a, int(channel)) for a, channel in entries]
    _check_entries('label_batch', [a for a, _ in entries])
    for a, channel in entries:
        if not 0 <= channel < a.shape[3]:
            raise ValueError(f'label_batch: channel {channel} of an array of shape {a.shape}')
        if a.shape[1] < 1 or a.shape[2] < 1:
            raise ValueError(f'label_batch: an empty array, {a.shape}')
    mode, value = _threshold_args('label_batch', threshold)
    max_components, cap = int(max_components), int(cap)
    if max_components < 0 or cap < 0:
        raise ValueError(f'label_batch: max_components = {max_components}, cap = {cap}')
    if not entries:
        return []
    _shared_code([a for a, _ in entries], 'label_batch', 'a dtype')
    cap = min(cap, max_components)
    planes = [CP.empty(a.shape[1:3], np.int32) for a, _ in entries] if labels else None
    counts, tables = _label_batch_call(entries, mode, value, cap, planes)
    if int(counts.max()) > max_components:
        raise HipError(f'label_batch: an entry has {int(counts.max())} components, more than max_components = {max_components}')
    _repeat_longer(counts, tables, [cap] * len(entries),
                   lambda longer, room: _label_batch_call([entries[i] for i in longer], mode, value, max(room), None))
    return [EntryComponents(count, table, planes[i] if labels else None)
            for i, (count, table) in enumerate(zip(counts, tables))]


def masked_crop(array, components, image_index, k, divisible_by=None):
    """Component k (1-based) of image `image_index`: array * (labels == k) cut to the component's box
    (interpreter.py:304-308), as a new (1, h, w, C) DeviceArray.  divisible_by=(y, x) also adds make_divisible_by's zero
    frame (my_model/model.py:26-34: at least one row and column, the crop centred) in the same pass."""
    n, h, w, c = array.shape
    if components.labels.shape != (n, h, w):
        raise ValueError(f'masked_crop: labels {components.labels.shape} do not belong to an array of shape {array.shape}')
    y0, x0, ch, cw = _box_of(components, image_index, k, 'masked_crop')
    out_h, out_w = _framed(ch, cw, divisible_by)
    out = CP.empty((1, out_h, out_w, c), array.dtype)
    _rt().call('uocr_masked_crop', array.code & 0xff, array.ptr, components.labels.ptr, n, h, w, c, int(image_index), int(k),
               y0, x0, ch, cw, out.ptr, out_h, out_w)
    return out


# ---- paragraph rotation (interpreter/interpreter.py:188-231, :319-347: the rotation search of ParagraphCrop) ----------
def rotation_geometry(ih, iw, angle):
    """What ndimage.rotate(.., angle, axes=(2, 1), reshape=True) computes in Python before it reaches its C loop, for an
    input plane of ih x iw: (M, offset, out_shape) -- M the 2 x 2 float64 matrix [[c, s], [-s, c]], out_shape the
    (rows, columns) of the rotated plane, offset the float64 pair (in_shape - 1) / 2 - M @ ((out_shape - 1) / 2).  Output
    pixel (oy, ox) reads the source coordinate offset + M @ (oy, ox).  The angle is in degrees."""
    c, s = np.cos(np.deg2rad(angle)), np.sin(np.deg2rad(angle))
    M = np.array([[c, s], [-s, c]])
    out_shape = (np.ptp(M @ [[0, 0, ih, ih], [0, iw, 0, iw]], axis=1) + 0.5).astype(int)
    offset = (np.array([ih, iw]) - 1) / 2 - M @ ((out_shape - 1) / 2)
    return M, offset, (int(out_shape[0]), int(out_shape[1]))


def _box_of(components, image_index, k, who):
    boxes = components.boxes[image_index]
    if not 1 <= k <= len(boxes):
        raise ValueError(f'{who}: image {image_index} has components 1..{len(boxes)}, not {k}')
    y0, y1, x0, x1 = boxes[k - 1].tolist()
    return y0, x0, y1 - y0, x1 - x0


def _framed(h, w, divisible_by):
    """h x w in make_divisible_by's zero frame (my_model/model.py:26-34: at least one row and column; None: no frame)"""
    d = divisible_by
    return (h, w) if d is None else (h + d[0] - h % d[0], w + d[1] - w % d[1])


def _geometry_args(geometry):
    """matrices, offsets and plane shapes of a list of rotation_geometry results: the three arguments of the kernels"""
    return (_flat([M.reshape(-1).tolist() for M, _, _ in geometry], C.c_double),
            _flat([offset.tolist() for _, offset, _ in geometry], C.c_double), _flat([shape for _, _, shape in geometry], C.c_int))


def rotated_extent(components, image_index, probes):
    """The half-open extents (y0, y1, x0, x1) -- ndimage.find_objects -- of the set pixels of
    ndimage.rotate(labels[box] == k, angle, axes=(2, 1), order=0, reshape=True) for every probe (k, angle) of `probes`: k a
    component (1-based) of image `image_index`, the box its bounding box.  Returns an int32 (len(probes), 4) host array,
    (0, 0, 0, 0) where no pixel is set; the height FindObjectHeightInRotated._func (interpreter.py:228-231) returns is
    y1 - y0.  ONE uocr_rotated_extent call (none for an empty list); no rotated array exists anywhere, the host reads 16
    bytes per probe."""
    probes = [(int(k), float(angle)) for k, angle in probes]
    if not probes:
        return np.zeros((0, 4), np.int32)
    n, h, w = components.labels.shape
    boxes = [_box_of(components, image_index, k, 'rotated_extent') for k, _ in probes]
    geometry = [rotation_geometry(bh, bw, angle) for (_, _, bh, bw), (_, angle) in zip(boxes, probes)]
    extent = CP.empty((len(probes), 4), np.int32)
    _rt().call('uocr_rotated_extent', components.labels.ptr, n, h, w, int(image_index), len(probes),
               _ints([k for k, _ in probes]), _flat(boxes, C.c_int), *_geometry_args(geometry), extent.ptr)
    return extent.numpy().copy()


def rotate_crop(entries, divisible_by=None):
    """rotate_array(.., angle)[:, region_y, region_x, :] of interpreter.py:343-346 for a flat list of entries (array,
    components, image_index, k, angle, region): the order-1 rotation by `angle` degrees of array * (labels == k) cut to
    component k's box, cut to region = (y0, y1, x0, x1) of the rotated plane (what rotated_extent returned for (k,
    angle)).  divisible_by=(y, x) also adds make_divisible_by's zero frame, as masked_crop does.  ONE uocr_rotate_crop
    call for all entries, whatever their sizes and channel counts (none for an empty list); returns the (1, h, w, C)
    DeviceArrays in the entries' order and dtype."""
    entries = [(a, comp, int(index), int(k), float(angle), tuple(int(v) for v in region))
               for a, comp, index, k, angle, region in entries]
    if not entries:
        return []
    _check_entries('rotate_crop', [entry[0] for entry in entries], '(N, H, W, C)')
    for a, comp, index, k, angle, region in entries:
        if comp.labels.shape != a.shape[:3]:
            raise ValueError(f'rotate_crop: labels {comp.labels.shape} do not belong to an array of shape {a.shape}')
    arrays, components, index, ks, angles, _ = zip(*entries)
    code = _shared_code(arrays, 'rotate_crop', 'a dtype')
    boxes = [_box_of(comp, i, k, 'rotate_crop') for comp, i, k in zip(components, index, ks)]
    geometry = [rotation_geometry(bh, bw, angle) for (_, _, bh, bw), angle in zip(boxes, angles)]
    regions, shapes = [], []
    for (*_, (y0, y1, x0, x1)), (_, _, plane) in zip(entries, geometry):
        if not (0 <= y0 < y1 <= plane[0] and 0 <= x0 < x1 <= plane[1]):
            raise ValueError(f'rotate_crop: the region [{y0}, {y1}) x [{x0}, {x1}) is empty or not inside the rotated plane {plane}')
        regions.append((y0, x0, y1 - y0, x1 - x0))
        shapes.append(_framed(y1 - y0, x1 - x0, divisible_by))
    outs = [CP.empty((1, oh, ow, a.shape[3]), a.dtype) for a, (oh, ow) in zip(arrays, shapes)]
    _rt().call('uocr_rotate_crop', code, len(entries), _pointers(arrays), _pointers([comp.labels for comp in components]),
               _flat([a.shape for a in arrays], C.c_int), _ints(index), _ints(ks), _flat(boxes, C.c_int), *_geometry_args(geometry),
               _flat(regions, C.c_int), _pointers(outs), _flat(shapes, C.c_int))
    return outs


# ---- the rotation search on the device (interpreter.py:321-336 walked by uocr_rotation_search) -------------------------
SEARCH_MAX_ROUNDS = 16
_search_tables = {}                  # eps -> (rounds, host table); (eps, device) -> the table on that device


def search_table(eps=1.0):
    """The tree of the ternary search of my_model/crop.py: search_steps, which does not depend on the data, in heap
    order: node 0 is (low, high) = (0, 180), child 2j + 1 the branch height_a < height_b (high = b), child 2j + 2 the
    other (low = a), a and b by search_steps' own expressions.  Returns (rounds, table): table float64 (2^rounds - 1, 4),
    per node cos a, sin a, cos b, sin b -- each a scalar call of the expression rotation_geometry uses, so that a row
    equals what rotation_geometry computes for the node's angles to the bit.  Built once per eps.  ValueError where the
    device cannot walk the tree: root-to-leaf paths of different lengths, none, or more than SEARCH_MAX_ROUNDS rounds."""
    eps = float(eps)
    if eps not in _search_tables:
        levels, level = [], [(0.0, 180.0)]
        while True:
            running = [high - low > eps for low, high in level]
            if not any(running):
                break
            if not all(running):
                raise ValueError(f'search_table: at eps = {eps} some searches end after {len(levels)} rounds and others go on')
            if len(levels) == SEARCH_MAX_ROUNDS:
                raise ValueError(f'search_table: the search at eps = {eps} takes more than {SEARCH_MAX_ROUNDS} rounds')
            levels.append([(low + (high - low) / 3, high - (high - low) / 3) for low, high in level])
            level = [child for (low, high), (a, b) in zip(level, levels[-1]) for child in ((low, b), (a, high))]
        if not levels:
            raise ValueError(f'search_table: the search at eps = {eps} makes no round')
        table = np.array([[np.cos(np.deg2rad(a)), np.sin(np.deg2rad(a)), np.cos(np.deg2rad(b)), np.sin(np.deg2rad(b))]
                          for probes in levels for a, b in probes], np.float64)
        table.setflags(write=False)
        _search_tables[eps] = len(levels), table
    return _search_tables[eps]


def search_path(leaf, eps=1.0):
    """search_steps replayed with the decisions in a leaf's heap index (from the top: a 0 bit of leaf + 1 after the
    leading one is height_a < height_b): the probes [(a, b)] of every round and the angle, None outside
    [eps, 180 - eps]"""
    low, high, probes = 0.0, 180.0, []
    for decision in bin(int(leaf) + 1)[3:]:
        if not high - low > eps:
            raise ValueError(f'search_path: {leaf} lies below a leaf of the tree at eps = {eps}')
        a = low + (high - low) / 3
        b = high - (high - low) / 3
        probes.append((a, b))
        if decision == '0':
            high = b
        else:
            low = a
    if int(leaf) < 0 or high - low > eps:
        raise ValueError(f'search_path: {leaf} is no leaf of the tree at eps = {eps}')
    angle = (high + low) / 2
    return probes, (angle if eps <= angle <= 180.0 - eps else None)


def angle_of_leaf(leaf, eps=1.0):
    """the angle search_steps returns after the decisions in the leaf's heap index: degrees, or None"""
    return search_path(leaf, eps)[1]


def search_geometry(ih, iw, c, s):
    """rotation_geometry as the DEVICE evaluates it during the search, from the cosine and sine of the table: plain
    Python floats, every product and sum rounded on its own, in this order -- the definition csrc/rotate.hip:
    rs_geometry matches bit for bit.  Returns (M, offset, out_shape) as flat tuples: M = (c, s, -s, c).
    rotation_geometry's `M @ ..` goes through NumPy's matrix product, which may fuse a multiply-add: the shapes agree, the
    offsets to some 1e-13 (tests/test_rotation_search_host.py)."""
    ih, iw, c, s = int(ih), int(iw), float(c), float(s)
    row0 = (0, s * iw, c * ih, c * ih + s * iw)
    row1 = (0, c * iw, (-s) * ih, (-s) * ih + c * iw)
    out_h = int((max(row0) - min(row0)) + 0.5)
    out_w = int((max(row1) - min(row1)) + 0.5)
    hy, hx = (out_h - 1) / 2, (out_w - 1) / 2
    off0 = (ih - 1) / 2 - (c * hy + s * hx)
    off1 = (iw - 1) / 2 - ((-s) * hy + c * hx)
    return (c, s, -s, c), (off0, off1), (out_h, out_w)


def _search_table_device(eps):
    rounds, table = search_table(eps)
    key = (float(eps), str(CP.storage_device()))
    if key not in _search_tables:
        _search_tables[key] = CP.copy(table.copy(), np.float64)
    return rounds, _search_tables[key]


def rotation_search(components, image_index, ks, eps=1.0):
    """The angle search of interpreter.py:321-336 for the components `ks` (1-based) of image `image_index`, walked by the
    device: returns (angles, traces) -- angles[i] in degrees or None, as search_steps returns it, computed on the host
    from the leaf the device ended on; traces[i] float64 (rounds, 4) = a, b, height_a, height_b per round.  ONE
    uocr_rotation_search call and ONE readback of (1 + 2 * rounds) ints per component (none for an empty list).
    ValueError from search_table where the device cannot walk the tree at this eps."""
    ks = [int(k) for k in ks]
    search_table(eps)
    if not ks:
        return [], []
    rounds, table = _search_table_device(eps)
    n, h, w = components.labels.shape
    boxes = [_box_of(components, image_index, k, 'rotation_search') for k in ks]
    size = C.c_size_t()
    if hiplib.get_lib().uocr_rotation_search_workspace(len(ks), C.byref(size)) != 0:
        raise HipError(f'uocr_rotation_search_workspace failed for {len(ks)} paragraphs')
    result = CP.empty((len(ks), 1 + 2 * rounds), np.int32)
    workspace = CP.empty((size.value // 4,), np.int32)
    _rt().call('uocr_rotation_search', components.labels.ptr, n, h, w, int(image_index), len(ks), _ints(ks),
               _flat(boxes, C.c_int), rounds, table.ptr, result.ptr, workspace.ptr)
    angles, traces = [], []
    for row in result.numpy():
        probes, angle = search_path(row[0], eps)
        angles.append(angle)
        traces.append(np.column_stack([np.array(probes, np.float64), row[1:].reshape(rounds, 2).astype(np.float64)]))
    return angles, traces


# ---- char labels (interpreter/interpreter.py:547-571: CharLabel) -----------------------------------------------------
def char_label(lines, bits, n_chars, want_ids=False):
    """The (W, n_chars) one-hot labels of every line of `lines`, a flat list of (1, H, W, C) DeviceArrays whose first
    `bits` channels are the bit layers: threshold at (mean + max) / 2 of the line, decode, vote per column
    (LabelChar._func1, interpreter.py:547-571).  ONE uocr_char_label call for all lines, whatever their sizes (none for an
    empty list); labels
    have the lines' dtype.  want_ids=True: also the int32 (W,) winning class of every column, -1 where the row is zero."""
    lines = list(lines)
    _check_entries('char_label', lines)
    if not lines:
        return ([], []) if want_ids else []
    code, c = _shared_code(lines, 'char_label', 'dtype and channel count'), lines[0].shape[3]
    if any(a.shape[3] != c for a in lines):
        raise ValueError('char_label: the lines of one call share dtype and channel count, got ' +
                         ', '.join(f'{a.shape} {a.dtype}' for a in lines))
    labels = [CP.empty((a.shape[2], n_chars), a.dtype) for a in lines]
    ids = [CP.empty((a.shape[2],), np.int32) for a in lines] if want_ids else None
    _rt().call('uocr_char_label', code, len(lines), _pointers(lines), _ints([a.shape[1] for a in lines]),
               _ints([a.shape[2] for a in lines]), int(c), int(bits), int(n_chars), _pointers(labels),
               _pointers(ids) if want_ids else None)
    return (labels, ids) if want_ids else labels


# ---- text of the lines (interpreter/interpreter.py:574-614: PredToText) ------------------------------------------------
def _pred_to_text_call(lines, cls, caps):
    """ONE uocr_pred_to_text call and ONE device-to-host copy: the counts sit at the head of the buffer the ids follow
    in.  Returns (counts, [the first min(count, cap) ids of every line])."""
    n = len(lines)
    starts = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64) + 4 * n
    out = CP.empty((int(starts[-1]),), np.uint8)
    address = lambda offsets: (C.c_void_p * n)(*[out.ptr + int(o) for o in offsets])
    _rt().call('uocr_pred_to_text', _shared_code(lines, 'pred_to_text', 'a dtype'), n, _pointers(lines),
               _ints([a.shape[0] for a in lines]), int(lines[0].shape[1]), _ints(cls), address(starts[:-1]), _ints(caps),
               address(4 * np.arange(n)))
    host = out.numpy()
    counts = host[:4 * n].view(np.int32)
    return counts, [host[s:s + min(int(c), cap)] for s, c, cap in zip(starts, counts, caps)]


def pred_to_text(lines, cls):
    """PredToText._func1 (interpreter.py:596-614) up to the character table: the ids the reference's walk emits for every
    line of `lines`, a flat list of (W, n_chars) DeviceArrays (the Char net's raw output), as one list of ints per line.
    cls[id] is the index of the id's pair of similar characters, -1 for an id without one.  ONE uocr_pred_to_text call
    for all lines with room for one id per row -- exact whenever no row holds a tie -- and ONE device-to-host copy; the
    lines that emitted more (rows with ties) are repeated in ONE second call with the room their counts ask for.  No
    call for an empty list."""
    lines = list(lines)
    _check_entries('pred_to_text', lines, '(W, n_chars)')
    if not lines:
        return []
    cls = [int(v) for v in cls]
    if any(a.shape[1] != len(cls) for a in lines):
        raise ValueError(f'pred_to_text: {len(cls)} classes, but the lines are ' + ', '.join(str(a.shape) for a in lines))
    caps = [a.shape[0] for a in lines]
    counts, ids = _pred_to_text_call(lines, cls, caps)
    _repeat_longer(counts, ids, caps, lambda longer, room: _pred_to_text_call([lines[i] for i in longer], cls, room))
    return [v.tolist() for v in ids]


# ---- score of the lines: what the Char net read against the labels (no counterpart in the reference) --------------------
def text_score(preds, labels, canon, want_ids=False):
    """The edit distance between what the labels say and what the Char net read, for every line: preds and labels are flat
    lists of (W, n_chars) DeviceArrays of one dtype, preds[i] the net's raw output and labels[i] the one-hot labels of the
    same W columns.  Both are read by one rule (the first maximum of every row, none where it is 0 or the row holds a
    NaN; one id per run of equal ids, the tab ends a run) and compared at unit cost, ids x and y matching when
    canon[x] == canon[y].  Returns int32 (n, 3): distance, length of the expected reading, length of the read one; with
    want_ids=True also the two readings, (scores, read ids per line, expected ids per line) as lists of ints.  ONE
    uocr_text_score call and ONE device-to-host copy -- scores and ids share a buffer -- and no call for an empty list."""
    preds, labels = list(preds), list(labels)
    if len(preds) != len(labels):
        raise ValueError(f'text_score: {len(preds)} predictions for {len(labels)} labels')
    _check_entries('text_score', preds + labels, '(W, n_chars)')
    if not preds:
        return (np.zeros((0, 3), np.int32), [], []) if want_ids else np.zeros((0, 3), np.int32)
    canon = [int(v) for v in canon]
    for pred, label in zip(preds, labels):
        if pred.shape != label.shape or pred.shape[1] != len(canon):
            raise ValueError(f'text_score: prediction {pred.shape} and labels {label.shape} of a line have one shape, '
                             f'(W, {len(canon)}) for a table of {len(canon)} entries')
    code = _shared_code(preds + labels, 'text_score', 'a dtype')
    n, widths = len(preds), [a.shape[0] for a in preds]
    starts = 16 * n + np.concatenate([[0], np.cumsum(widths + widths)]).astype(np.int64)
    out = CP.empty((int(starts[-1]) if want_ids else 16 * n,), np.uint8)
    address = lambda offsets: (C.c_void_p * n)(*[out.ptr + int(o) for o in offsets]) if want_ids else None
    _rt().call('uocr_text_score', code, n, _pointers(preds), _pointers(labels), _ints(widths), len(canon), _ints(canon),
               address(starts[:n]), address(starts[n:2 * n]), out.ptr)
    host = out.numpy()
    table = host[:16 * n].view(np.int32).reshape(n, 4)
    scores = table[:, :3].copy()
    if not want_ids:
        return scores
    read = [host[s:s + count].tolist() for s, count in zip(starts[:n], table[:, 2])]
    expected = [host[s:s + count].tolist() for s, count in zip(starts[n:2 * n], table[:, 1])]
    return scores, read, expected


# ---- score of the masks: what a mask net found of the true components (nn/metrics.py: binary_classification_metrics is
# the pixel half; the reference has no score of components) --------------------------------------------------------------
def label_overlap(pairs, cap_a, cap_b, want_table=False):
    """The overlap counts of pairs (a, b) of int32 (H, W) label planes, a the expected labels and b the predicted ones as
    label_batch(labels=True) returns them, whatever the sizes of the pairs.  Labels above a cap, and negative ones, count
    in the overflow bucket cap + 1.  Returns (summary, rows, cols): int64 (n, 8) = tp, fp, fn, tn, expected, predicted,
    matched, overflow; int32 (n, cap_a + 2, 4) and (n, cap_b + 2, 4) = area, best, inter, other per row and per column of
    the table (include/univer_hip.h states the rules); with want_table=True also the tables, int32 (n, cap_a + 2,
    cap_b + 2), as a fourth item.  ONE uocr_label_overlap call and ONE device-to-host copy -- summary, rows and cols
    share a buffer, which the tables join only when asked for -- and no call for an empty list."""
    pairs = [(a, b) for a, b in pairs]
    cap_a, cap_b = int(cap_a), int(cap_b)
    if cap_a < 0 or cap_b < 0:
        raise ValueError(f'label_overlap: cap_a = {cap_a}, cap_b = {cap_b}')
    for a, b in pairs:
        for plane in (a, b):
            if not isinstance(plane, DeviceArray) or plane.ndim != 2 or plane.dtype != np.int32 or plane.size < 1:
                raise ValueError(f'label_overlap: expected int32 (H, W) device arrays, got '
                                 f'{getattr(plane, "shape", type(plane))} {getattr(plane, "dtype", "")}')
        if a.shape != b.shape:
            raise ValueError(f'label_overlap: the planes of a pair have one shape, got {a.shape} and {b.shape}')
    n, r, s = len(pairs), cap_a + 2, cap_b + 2
    sizes = [64 * n, 16 * n * r, 16 * n * s, 4 * n * r * s]           # summary (int64 first), rows, cols, tables
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if not pairs:
        empty = (np.zeros((0, 8), np.int64), np.zeros((0, r, 4), np.int32), np.zeros((0, s, 4), np.int32))
        return empty + (np.zeros((0, r, s), np.int32),) if want_table else empty
    out = CP.empty((int(starts[4 if want_table else 3]),), np.uint8)
    tables = None if want_table else CP.empty((n, r, s), np.int32)
    at = lambda k: C.c_void_p(out.ptr + int(starts[k]))
    _rt().call('uocr_label_overlap', n, _pointers([a for a, _ in pairs]), _pointers([b for _, b in pairs]),
               _ints([a.shape[0] for a, _ in pairs]), _ints([a.shape[1] for a, _ in pairs]), cap_a, cap_b,
               at(3) if want_table else C.c_void_p(tables.ptr), at(1), at(2), at(0))
    host = out.numpy()
    piece = lambda k, dtype, shape: host[starts[k]:starts[k + 1]].view(dtype).reshape(shape).copy()
    result = (piece(0, np.int64, (n, 8)), piece(1, np.int32, (n, r, 4)), piece(2, np.int32, (n, s, 4)))
    return result + (piece(3, np.int32, (n, r, s)),) if want_table else result


_MASK_SCORE_FIELDS = ('tp fp fn tn expected predicted matched overflow rows precision recall f1 accuracy iou '
                      'mean_matched_iou')


class MaskScore(namedtuple('MaskScore', _MASK_SCORE_FIELDS)):
    """The score of one mask: the eight ints of the summary (pixels: tp, fp, fn, tn, overflow; components: expected,
    predicted, matched), `rows` = (area, best, inter, other) of every expected component within the cap, as a tuple of
    tuples of ints, and the numbers derived from the ints on the host: precision, recall, f1 and accuracy by the
    reference's formulas (nn/metrics.py:13-17), iou = tp / (tp + fp + fn), mean_matched_iou over the matched components;
    each None where its denominator is 0."""
    __slots__ = ()


def mask_numbers(tp, fp, fn, tn):
    """precision, recall, f1, accuracy, iou of four pixel counts (ints): nn/metrics.py:13-17 with f1beta = 1, and the
    intersection over union; None where a denominator is 0"""
    ratio = lambda numerator, denominator: numerator / denominator if denominator else None
    precision, recall = ratio(tp, tp + fp), ratio(tp, tp + fn)
    f1 = None if precision is None or recall is None else ratio(2 * precision * recall, precision + recall)
    return precision, recall, f1, ratio(tp + tn, tp + tn + fp + fn), ratio(tp, tp + fp + fn)


def mask_score_of(summary, rows):
    """the MaskScore of one entry of label_overlap: its summary (8 ints) and its rows (cap + 2, 4)"""
    ints = [int(v) for v in summary]
    inner = [tuple(int(v) for v in row) for row in rows[1:-1] if row[0] > 0]
    ious = [inter / (area + other - inter) for area, best, inter, other in inner
            if best > 0 and 2 * inter > area + other - inter]
    return MaskScore(*ints, tuple(inner), *mask_numbers(*ints[:4]), sum(ious) / len(ious) if ious else None)


def mask_score(pairs, threshold, true_threshold=None, cap=64):
    """How well masks were predicted: pairs of ((pred_array, channel), (true_array, channel)), channels of (1, H, W, C)
    DeviceArrays as label_batch takes them, a prediction and the truth of one size.  Both sides are thresholded
    (`threshold` the prediction, `true_threshold` the truth, by default the same rule: 'mean', 'mean_max' or a number)
    and labelled by uocr_label_batch -- ONE call for all 2n entries where rule and dtype are the same, two otherwise --
    and the two label planes of every pair go through label_overlap with caps `cap`.  A mask with more than `cap`
    components is no error: its planes are complete, the excess counts in the overflow bucket (MaskScore.overflow).
    cap=0 compares foreground with foreground alone.  Returns one MaskScore per pair."""
    pairs = [((p, int(pc)), (t, int(tc))) for (p, pc), (t, tc) in pairs]
    cap = int(cap)
    if cap < 0:
        raise ValueError(f'mask_score: cap = {cap}')
    if not pairs:
        return []
    true_threshold = threshold if true_threshold is None else true_threshold
    sides = [[pred for pred, _ in pairs], [true for _, true in pairs]]
    for entries in sides:
        _check_entries('mask_score', [a for a, _ in entries])
        for a, channel in entries:
            if not 0 <= channel < a.shape[3] or a.shape[1] < 1 or a.shape[2] < 1:
                raise ValueError(f'mask_score: channel {channel} of an array of shape {a.shape}')
    for (pred, _), (true, _) in pairs:
        if pred.shape[1:3] != true.shape[1:3]:
            raise ValueError(f'mask_score: a prediction of {pred.shape[1:3]} for a truth of {true.shape[1:3]}')
    rules = [_threshold_args('mask_score', threshold), _threshold_args('mask_score', true_threshold)]
    planes = [[CP.empty(a.shape[1:3], np.int32) for a, _ in entries] for entries in sides]
    # the library itself, not label_batch: a count above the room for rows (one row each: none is wanted here) is no error
    codes = {a.code & 0xff for entries in sides for a, _ in entries}
    if rules[0] == rules[1] and len(codes) == 1:
        _label_batch_call(sides[0] + sides[1], *rules[0], 1, planes[0] + planes[1])
    else:
        for entries, rule, side_planes in zip(sides, rules, planes):
            _label_batch_call(entries, *rule, 1, side_planes)
    summary, rows, _ = label_overlap(zip(planes[1], planes[0]), cap, cap)
    return [mask_score_of(summary[i], rows[i]) for i in range(len(pairs))]


# ---- line crops (interpreter/interpreter.py:504-523: the gather half of LineCrop) -------------------------------------
def line_crop_shape(box_h, box_w, quarter_turns, zoomed_height=32, minimal_width=8):
    """(zoom_h, zoom_w, out_w) of a box_h x box_w box after `quarter_turns` turns of 90 degrees, ndimage.zoom by
    zf = zoomed_height / height in both directions (:512-514: output sizes are Python round(n * zf), half to even; the
    width may come out 0) and zero padding of the width up to minimal_width (:516-521).  None switches a step off, as in
    the reference."""
    h, w = (box_w, box_h) if quarter_turns % 2 else (box_h, box_w)
    if zoomed_height is not None:
        zf = zoomed_height / h
        h, w = int(round(h * zf)), int(round(w * zf))
    return h, w, w if minimal_width is None else max(w, minimal_width)


def line_crop(entries, zoomed_height=32, minimal_width=8):
    """CropRotateAndZoomLines._func2 (interpreter.py:504-523) for a flat list of entries (array, y0, x0, box_h, box_w,
    quarter_turns): the box of the (1, H, W, C) DeviceArray `array`, turned by quarter_turns * 90 degrees (0-3; the
    reference's rotation None / 90 / 180 / 270), zoomed to zoomed_height rows at order 0 and zero-padded to minimal_width
    columns.  ONE uocr_line_crop call for all entries, whatever their sizes and channel counts (none for an empty list);
    returns the (1, zoomed_height, out_w, C) DeviceArrays in the entries' order and dtype."""
    entries = [(a, int(y0), int(x0), int(bh), int(bw), int(turns)) for a, y0, x0, bh, bw, turns in entries]
    _check_entries('line_crop', [entry[0] for entry in entries])
    for a, y0, x0, bh, bw, turns in entries:
        if not (0 <= y0 and 0 <= x0 and bh >= 1 and bw >= 1 and y0 + bh <= a.shape[1] and x0 + bw <= a.shape[2]):
            raise ValueError(f'line_crop: the box [{y0}, {y0 + bh}) x [{x0}, {x0 + bw}) is empty or not inside {a.shape}')
        if not 0 <= turns <= 3:
            raise ValueError(f'line_crop: quarter_turns must be 0, 1, 2 or 3, got {turns}')
    if not entries:
        return []
    arrays, y0, x0, box_h, box_w, turns = zip(*entries)
    code = _shared_code(arrays, 'line_crop', 'a dtype')
    zoom_h, zoom_w, out_w = zip(*[line_crop_shape(bh, bw, t, zoomed_height, minimal_width) for bh, bw, t in zip(box_h, box_w, turns)])
    outs = [CP.empty((1, zh, ow, a.shape[3]), a.dtype) for a, zh, ow in zip(arrays, zoom_h, out_w)]
    _rt().call('uocr_line_crop', code, len(entries), _pointers(arrays), *(_ints([a.shape[d] for a in arrays]) for d in (1, 2, 3)),
               _ints(y0), _ints(x0), _ints(box_h), _ints(box_w), _ints(turns), _ints(zoom_h), _ints(zoom_w), _pointers(outs),
               _ints(out_w))
    return outs


# ---- the lines of a page in one strip (the Char net over all lines of a page in one pass) -------------------------------
PACK_GAP = 4             # columns between neighbouring lines: the left padding of the Char net's windows of 8 columns


def pack_layout(widths, gap=PACK_GAP, max_columns=32768):
    """Where the lines of a page, `widths` columns wide, go when they are laid side by side: a list of strips, each
    (segments, strip_w) with segments = [(line index, x0, w), ...], line `index` at columns [x0, x0 + w) of a strip of
    strip_w columns, `gap` columns between neighbours and none at the outer ends.  Host only.  Lines keep their order and
    are never split; a strip takes lines while it stays within max_columns, a line wider than that gets a strip of its
    own.  gap >= 4: the windows of the Char net (Conv2DToBatchedFixedWidthed(8)) pad 4 zero columns on their left, so a
    narrower gap lets a line's first windows see its neighbour -- the convs in front, 3 columns wide with padding 1, need
    1 each."""
    gap, max_columns = int(gap), int(max_columns)
    if gap < PACK_GAP:
        raise ValueError(f'pack_layout: gap {gap} is narrower than the left padding of the windows of 8 columns, {PACK_GAP}: '
                         f'a line would see its neighbour')
    strips = []
    for index, w in enumerate(int(w) for w in widths):
        if w < 1:
            raise ValueError(f'pack_layout: line {index} has width {w}')
        if strips and strips[-1][1] + gap + w <= max_columns:
            segments, strip_w = strips[-1]
            segments.append((index, strip_w + gap, w))
            strips[-1] = (segments, strip_w + gap + w)
        else:
            strips.append(([(index, 0, w)], w))
    return strips


def _segment_arrays(segments, strip_w, who):
    """(x0, w) of a call as C arrays, after the checks the library makes too (ascending, disjoint, inside the strip)"""
    segments = [(int(x0), int(w)) for x0, w in segments]
    end = 0
    for x0, w in segments:
        if w < 1 or x0 < end or x0 + w > strip_w:
            raise ValueError(f'{who}: the segments {segments} are not ascending, disjoint and inside [0, {strip_w})')
        end = x0 + w
    return _ints([x0 for x0, _ in segments]), _ints([w for _, w in segments])


def pack_lines(lines, strip):
    """One strip of pack_layout -- strip = (segments, strip_w), segments = [(line index, x0, w), ...] -- filled from the
    flat list `lines` of (1, H, W, C) DeviceArrays of one height, channel count and dtype: a new (1, H, strip_w, C)
    DeviceArray, lines[index] at columns [x0, x0 + w), zero everywhere else.  ONE uocr_pack_lines call."""
    segments, strip_w = strip
    chosen = [lines[index] for index, _, _ in segments]
    if not chosen:
        raise ValueError('pack_lines: a strip without lines')
    _check_entries('pack_lines', chosen)
    code, (_, h, _, c) = _shared_code(chosen, 'pack_lines', 'a dtype'), chosen[0].shape
    if any((a.shape[1], a.shape[3]) != (h, c) for a in chosen) or any(a.shape[2] != w for a, (_, _, w) in zip(chosen, segments)):
        raise ValueError(f'pack_lines: the lines {[a.shape for a in chosen]} do not fit the segments {segments} of one strip')
    x0, w = _segment_arrays([s[1:] for s in segments], int(strip_w), 'pack_lines')
    out = CP.empty((1, h, int(strip_w), c), chosen[0].dtype)
    _rt().call('uocr_pack_lines', code, len(chosen), _pointers(chosen), w, h, c, x0, out.ptr, int(strip_w))
    return out


def zero_gaps(x, segments):
    """In place on x: (1, H, W, C): every column outside the segments [(x0, w), ...] becomes +0.0, whatever it held; the
    segments are not touched.  ONE uocr_zero_gaps call that visits the gaps only (none for an empty list).  Returns x."""
    if not isinstance(x, DeviceArray) or x.ndim != 4 or x.shape[0] != 1:
        raise ValueError(f'zero_gaps: expected a (1, H, W, C) device array, got {getattr(x, "shape", type(x))}')
    x0, w = _segment_arrays(segments, x.shape[2], 'zero_gaps')
    if len(x0):
        _rt().call('uocr_zero_gaps', x.code & 0xff, x.ptr, x.shape[1], x.shape[2], x.shape[3], len(x0), x0, w)
    return x


# ---- training pages made on the device (image_generator/generate.py: add_paragraph) ---------------
PAGE_TABLES = (('paragraphs', 32, 8), ('lines', 32 * 30, 5), ('glyphs', 32 * 30 * 11, 2))    # name, rows per page, ints per row
PAGE_LAYERS = (('image', 1), ('monochrome', 1), ('paragraph', 1), ('line', 2), ('char', 9))  # name, channels


def _atlas_arrays(atlas, who):
    """(metrics, adv, offset, cells) of an atlas: int32 (F, 7), (F, 162), (F, 162) and uint8 (n,) DeviceArrays"""
    arrays = [atlas[key] for key in ('metrics', 'adv', 'offset', 'cells')]
    faces = arrays[0].shape[0] if isinstance(arrays[0], DeviceArray) and arrays[0].ndim == 2 else 0
    wanted = (((faces, 7), np.int32), ((faces, 162), np.int32), ((faces, 162), np.int32), (arrays[3].shape[:1], np.uint8))
    for a, (shape, dtype) in zip(arrays, wanted):
        if not isinstance(a, DeviceArray) or faces < 1 or a.shape != shape or a.dtype != dtype:
            raise ValueError(f'{who}: the atlas holds metrics (F, 7), adv (F, 162), offset (F, 162) int32 and cells (n,) uint8 '
                             f'device arrays, got {[(getattr(a, "shape", type(a)), getattr(a, "dtype", None)) for a in arrays]}')
    return arrays


def page_layout(atlas, seed, first_page, n_pages, height, width):
    """The tables of pages first_page .. first_page + n_pages - 1 (Python ints, taken mod 2^64 like the seed) of
    height x width pixels: {'paragraphs': (n, 32, 8), 'lines': (n, 960, 5), 'glyphs': (n, 10560, 2), 'counts': (n, 4)} int32
    DeviceArrays; rows past a page's counts hold whatever the allocation held.  ONE uocr_page_layout call (none for no
    page); nothing is read back."""
    metrics, adv, _, _ = _atlas_arrays(atlas, 'page_layout')
    n_pages, height, width = int(n_pages), int(height), int(width)
    if n_pages < 0 or height < 1 or width < 1:
        raise ValueError(f'page_layout: {n_pages} pages of {height} x {width}')
    tables = {name: CP.empty((n_pages, rows, ints), np.int32) for name, rows, ints in PAGE_TABLES}
    tables['counts'] = CP.empty((n_pages, 4), np.int32)
    if n_pages:
        _rt().call('uocr_page_layout', int(seed) % 2 ** 64, int(first_page) % 2 ** 64, n_pages, height, width, metrics.shape[0],
                   metrics.ptr, adv.ptr, *(tables[name].ptr for name in ('paragraphs', 'lines', 'glyphs', 'counts')))
    return tables


def page_render(atlas, tables, height, width, lut):
    """The five label layers of the pages in `tables` (the dict page_layout returns, or hand-built tables of the same
    shapes): {'image', 'monochrome', 'paragraph': (n, H, W, 1), 'line': (n, H, W, 2), 'char': (n, H, W, 9)} DeviceArrays in
    the dtype of `lut`, the (256,) DeviceArray of np.arange(256) / 255.  ONE uocr_page_render call (none for no page)."""
    metrics, adv, offset, cells = _atlas_arrays(atlas, 'page_render')
    height, width = int(height), int(width)
    n_pages = tables['counts'].shape[0]
    for name, rows, ints in PAGE_TABLES + (('counts', 4, None),):
        a, shape = tables[name], (n_pages, rows) + ((ints,) if ints else ())
        if not isinstance(a, DeviceArray) or a.shape != shape or a.dtype != np.int32:
            raise ValueError(f'page_render: table {name!r} must be an int32 device array of shape {shape}, got '
                             f'{getattr(a, "shape", type(a))} {getattr(a, "dtype", "")}')
    if not isinstance(lut, DeviceArray) or lut.shape != (256,) or height < 1 or width < 1:
        raise ValueError(f'page_render: lut must be a (256,) device array and the page at least 1 x 1, got '
                         f'{getattr(lut, "shape", type(lut))}, {height} x {width}')
    out = {name: CP.empty((n_pages, height, width, c), lut.dtype) for name, c in PAGE_LAYERS}
    if n_pages:
        _rt().call('uocr_page_render', lut.code & 0xff, n_pages, height, width,
                   *(tables[name].ptr for name in ('paragraphs', 'lines', 'glyphs', 'counts')), metrics.shape[0], metrics.ptr,
                   adv.ptr, offset.ptr, cells.ptr, cells.shape[0], lut.ptr, *(out[name].ptr for name, _ in PAGE_LAYERS))
    return out


class _Ops:
    add = staticmethod(add)


CP.ops = _Ops
