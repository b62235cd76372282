"""The HBM-bound kernels of elementwise.hip, loss.hip and shape_ops.hip past one grid, against the float64 oracle.

The other parity tests run these kernels at the sizes of the golden fixtures (35 to a few thousand elements): one
trip of every grid-stride loop, aligned operands, one block of partial sums.  Here every launcher's block cap is
crossed by a small margin, operands are also views that are only element-aligned, and every result is compared with
oracle/nn_oracle.py evaluated in float64 on the inputs (and hyper-parameters) rounded to the storage type, so only the
kernel's own arithmetic is judged.  What each case is for:

| op | sizes here | what they reach |
|---|---|---|
| act_fwd / act_bwd / act_bwd_from_output / add / axpy / scale / fill (`map_kernel`, `fill_kernel`) | 1, V-1, V, V+1, 255 V + 3, 2048 * 256 * V + V + 1 with V = 16 / sizeof(type); float32, float64, binary16; aligned and through views one element in | vector body and scalar tail in the first block, in a later block and behind a second trip of the grid capped at 2048 blocks; the V = 1 kernels for unaligned operands (their second trip starts at 524 288 elements) |
| has_nan | same sizes, float32 / float64 | NaN at 0, at n - 1 and at an index only the second trip reads; +-inf is not NaN |
| convert | 1, 3, 1023, 524 288 + 5, 2 097 152 + 5; all six type pairs | the scalar kernel past its 2048-block cap, bit for bit with numpy's astype (one rounding from float64 to binary16) |
| u8_to_float | 16 * 40, 8 388 608 + 48 pixels (16-pixel kernel past 2048 blocks), 524 288 + 7 (fallback past 2048 blocks), source or destination one element in | both kernels, bit for bit |
| copy_2d (concat / split) | 4100 rows x (1, 3, 5, 520) columns on the last axis, 2 x (2050, 1030) on axis 0 | more than 8192 blocks of 256 elements; narrow and wide column counts in one call sequence |
| Adam / Momentum / RMSProp | 1, 3, 4, 5, 1027, 300 001, cap + 5 | Adam's vector body (4 float32 / 2 float64) with a tail behind the 2048-block cap, the scalar kernels past theirs, unaligned views with guards |
| fused Momentum / Adam tails | 5003, 262 144 * 4 + 7 with four ranges, 1024 * 1024 + 4099 without | ranges that begin and end inside a vector, adjacent and empty ranges, L1 at weights of exactly 0, zero_grad on and off, hyper-parameters from device memory, the 256-block (ranges) and 1024-block caps with further trips, the last block's sum over 256 blocks of partials, VEC = 1 for views |
| regularize | 60, 1025, 600 001 | `reg_kernel` past its 512-block cap, `finish_sum_kernel` over 512 partials, accumulation into gradient and loss slot |
| softmax CE | (4100, 162), (8200, 100), (16400, 37); c in 1 .. 700 at m = 37 | more than 1024 blocks (the strided walk of `last_block_fold` past its first 4 rows per thread), every lane-group width and more than 4 trips of 64 lanes, rows with a large common offset |
| sigmoid CE | 525 313 elements | the 512-block cap |
| Dice / Jaccard | (1, 768, 768, 1), (1, 1024, 1100, 2), (2, 130, 130, 4), (2, 97, 101, 3), (2, 95, 97, 1), binary16 (1, 1024, 2100, 2) | the 64-chunk cap of the sums kernels, the 512-chunk cap of the vector gradient kernel, C = 4 vectors, the generic kernels over several chunks, the fallback for unaligned views |
| max-pool / upsample / fixed width | (2, 2050, 2064, 4), (3, 1800, 1804, 1), (2, 301, 403, 3); upsampling of more than 2 097 152 quads / outputs; (2, 16, 16400, 4) strips | the 8192-block cap of the vector and of the generic kernels, ties in most windows |

Every case named after a cap computes the block count the launcher will ask for (the host formula restated below) and
asserts that it exceeds the cap.  Outputs start as NaN (arrays the wrappers allocate through `CP.empty` are poisoned,
explicit outputs are pre-filled) and views sit between sentinel borders that must survive.

Entry points that had no test of their own until now: uocr_act_bwd_from_output, uocr_copy_2d beyond one block,
uocr_convert for five of its six pairs; the fused optimizer tails, Adam / Momentum / RMSProp, the regularisers and
the losses had none against the oracle at more than one block.

uocr_act_bwd_from_output takes LeakyRelu (alpha > 0) and Sigmoid only: a Relu output is -0.0 for every negative
input and for the input -0.0 alike, so the reference's `x >= 0` mask cannot be recovered from it.  The entry point
refuses Relu, and that refusal is what the Relu case asserts.

Tolerances are the project's (normalised max error): 1e-5 float32, 1e-12 float64 (test_gpu_ops.py), 1e-3 for a tensor
stored in binary16 and 2e-5 for float32 / float64 results from binary16 inputs (test_gpu_f16.py).  Ops that move or
select values are compared bit for bit.
"""
import numpy as np
import pytest

from conftest import rel_linf
from oracle import nn_oracle as O

pytestmark = pytest.mark.gpu

TOL = {'float32': 1e-5, 'float64': 1e-12, 'float16': 1e-3}
TOL_FROM16 = 2e-5                 # float32 / float64 results computed from binary16 inputs
DTYPES = ['float32', 'float64', 'float16']
MAX_GRID = 2048                   # UOCR_MAX_GRID: block cap of the elementwise launchers (uocr_common.h)
SHAPE_GRID = 4 * MAX_GRID         # block cap of the shape_ops launchers
GUARD = 64                        # sentinel elements on each side of a view
SENTINEL = -1536.0                # exact in binary16
ACT_CASES = (('relu', 0.0), ('leaky', 0.01), ('leaky', 0.3), ('sigmoid', 0.0))


# ---- host rules restated -------------------------------------------------------------------------------------
def cdiv(a, b):
    return (a + b - 1) // b


def wanted_blocks(items, per_block=256):
    """uocr_blocks_for before its cap: the grid the launcher would need to cover `items` in one trip."""
    return max(1, cdiv(items, per_block))


def vec_width(dtype):
    return 16 // np.dtype(dtype).itemsize


def map_items(n, dtype, off):
    """launch_map / uocr_fill / uocr_adam_step: one thread per 16-byte vector, per element for unaligned operands."""
    return n if off else cdiv(n, vec_width(dtype))


def map_sizes(dtype):
    v = vec_width(dtype)
    return sorted({1, max(1, v - 1), v, v + 1, 255 * v + 3, MAX_GRID * 256 * v + v + 1})


# ---- helpers ---------------------------------------------------------------------------------------------------
def rs(a, dtype):
    """what the device holds after an upload in `dtype`, as float64"""
    return np.asarray(a, dtype=np.float64).astype(dtype).astype(np.float64)


def hp(x, dtype):
    """a scalar argument after the launcher's cast to the compute type (binary16 tensors compute in float32)"""
    t = np.float64 if np.dtype(dtype) == np.float64 else np.float32
    return float(t(x))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, f'{what}: {got.dtype}{got.shape} != {ref.dtype}{ref.shape}'
    bad = np.flatnonzero(bits(got).ravel() != bits(ref).ravel())
    assert bad.size == 0, (f'{what}: {bad.size} of {ref.size} elements differ, first at flat index {bad[0]}: '
                           f'got {got.ravel()[bad[0]]!r}, expected {ref.ravel()[bad[0]]!r}')


def close(got, ref, tol, what):
    """rel_linf(got, ref) <= tol, reported as the number of elements beyond tol * max|ref| and the worst of them."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f'{what}: {got.shape} != {ref.shape}'
    if ref.size == 0:
        return
    scale = max(1e-30, float(np.max(np.abs(ref))))
    err = np.abs(got - ref)
    err[np.isnan(err)] = np.inf                      # a NaN left in an output is as wrong as it gets
    bad = err > tol * scale
    worst = int(np.argmax(err))
    print(f'{what}: rel_linf {err.ravel()[worst] / scale:.3e} (tolerance {tol:.0e}) at flat index {worst}')
    assert not bad.any(), (f'{what}: {int(bad.sum())} of {ref.size} elements off by more than {tol:.0e} * {scale:.3e}; '
                           f'worst at flat index {worst}: got {got.ravel()[worst]!r}, expected {ref.ravel()[worst]!r}')
    assert rel_linf(got, ref) <= tol, what


def loss_close(loss, ref, tol, what):
    print(f'{what}: loss {float(loss)!r}, oracle {ref!r}')
    assert abs(float(loss) - ref) <= tol * max(1.0, abs(ref)), f'{what}: loss {float(loss)!r} != {ref!r}'


class Buf:
    """`n` elements of `dtype` on the device, `off` elements past a 16-byte boundary, between sentinel borders.
    `data` None: the payload starts as NaN (an output the op must overwrite)."""

    def __init__(self, CP, n, dtype, off=0, data=None, shape=None):
        self.CP, self.n, self.lo = CP, int(n), GUARD + off
        host = np.full(self.lo + self.n + GUARD, SENTINEL, dtype=np.float64)
        host[self.lo:self.lo + self.n] = np.nan if data is None else np.asarray(data, dtype=np.float64).ravel()
        self.base = CP.copy(host, dtype)
        view = self.base.t[self.lo:self.lo + self.n]
        self.v = type(self.base)(view if shape is None else view.view(*shape))
        assert self.v.ptr % 16 == (off * np.dtype(dtype).itemsize) % 16

    def get(self, what):
        """the payload, after checking that the borders are untouched"""
        host = self.CP.asnumpy(self.base)
        assert np.all(host[:self.lo] == SENTINEL), f'{what}: wrote BEFORE the view'
        assert np.all(host[self.lo + self.n:] == SENTINEL), f'{what}: wrote PAST the view'
        return host[self.lo:self.lo + self.n].reshape(self.v.shape)


@pytest.fixture
def gpu(monkeypatch):
    """mode(dtype) -> CP in that compute type; every array the ops allocate through CP.empty starts as NaN (0xA5 for
    integer arrays).  float32 and the default gradient scale are restored afterwards."""
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    plain = CP.empty

    def poisoned(shape, dtype=None):
        out = plain(shape, dtype)
        if out.size:
            out.t.fill_(float('nan') if out.t.is_floating_point() else 0xA5)
        return out

    monkeypatch.setattr(CP, 'empty', staticmethod(poisoned))

    def mode(dtype):
        CP.set_dtype(dtype)
        CP.f16_grad_scale_log2 = None
        return CP

    yield mode
    monkeypatch.undo()
    CP.set_dtype('float32')
    CP.f16_grad_scale_log2 = None


def signed_zeros(x):
    """exact zeros and negative zeros among the values: the `>= 0` mask of the reference decides there.  Nothing else
    is closer to zero than 1e-3, so that alpha * x keeps its sign in binary16 too (the backward pass from the output
    reads the sign of the input off the output)."""
    small = np.abs(x) < 1e-3
    x[small] = np.where(x[small] < 0, -1e-3, 1e-3)
    x[0::7] = 0.0
    x[3::11] = -0.0
    return x


# ---- 1. map-style kernels --------------------------------------------------------------------------------------
class MapCalls:
    """The out-of-place map ops on Buf operands.  Aligned: through the wrappers of nn/ops.py (their outputs come from
    the poisoned CP.empty).  Offset views: the same entry points by name with a NaN-filled output view, because the
    wrappers allocate their (aligned) output themselves."""

    def __init__(self, CP, dtype, off):
        from univer_ocr_amd.nn import ops
        self.CP, self.ops, self.dtype, self.off = CP, ops, dtype, off

    def _run(self, wrapper, name, head, ins, what):
        if not self.off:
            out = self.CP.asnumpy(wrapper())
        else:
            o = Buf(self.CP, ins[0].n, self.dtype, self.off)
            self.CP.runtime().call(name, ins[0].v.code, *head, *[b.v.ptr for b in ins], o.v.ptr, ins[0].n)
            out = o.get(what)
        for b in ins:
            b.get(what + ' (input)')
        return out

    def act_fwd(self, kind, alpha, x, what):
        return self._run(lambda: self.ops.act_fwd(kind, x.v, alpha), 'uocr_act_fwd',
                         (self.ops.ACT_CODES[kind], float(alpha)), (x,), what)

    def act_bwd(self, kind, alpha, x, dy, what):
        return self._run(lambda: self.ops.act_bwd(kind, x.v, dy.v, alpha), 'uocr_act_bwd',
                         (self.ops.ACT_CODES[kind], float(alpha)), (x, dy), what)

    def act_bwd_from_output(self, kind, alpha, y, dy, what):
        return self._run(lambda: self.ops.act_bwd_from_output(kind, y.v, dy.v, alpha), 'uocr_act_bwd_from_output',
                         (self.ops.ACT_CODES[kind], float(alpha)), (y, dy), what)

    def add(self, a, b, what):
        return self._run(lambda: self.ops.add(a.v, b.v), 'uocr_add', (), (a, b), what)


def oracle_act(kind, alpha):
    if kind == 'relu':
        return O.relu_fwd, O.relu_bwd
    if kind == 'leaky':
        return (lambda a: O.leaky_relu_fwd(a, alpha)), (lambda a, g: O.leaky_relu_bwd(a, g, alpha))
    return O.sigmoid_fwd, O.sigmoid_bwd


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('dtype', DTYPES)
def test_activations_and_add_past_one_grid(dtype, off, gpu):
    """act_fwd, act_bwd, act_bwd_from_output and add at the sizes of map_sizes(): vector body, vector tail in block 0,
    in block 255 and behind the second trip of the capped grid; off = 1 runs the V = 1 kernels on views.  Relu forward
    is a selection and compared bit for bit: x * mask is -0.0 for a negative x in every type (the binary16 kernels
    returned +0.0 until map_store in elementwise.hip kept the product apart from the conversion); the sign of every
    zero that Relu / LeakyRelu produce, forward and backward, is the oracle's."""
    from univer_ocr_amd.hip import HipError
    CP = gpu(dtype)
    calls = MapCalls(CP, dtype, off)
    tol = TOL[dtype]
    for n in map_sizes(dtype):
        if n > MAX_GRID * 256 * vec_width(dtype):
            assert wanted_blocks(map_items(n, dtype, off)) > MAX_GRID
        rng = np.random.default_rng(n + off)
        xs = rs(signed_zeros(rng.standard_normal(n)), dtype)
        gs = rs(rng.standard_normal(n), dtype)
        x, dy = Buf(CP, n, dtype, off, xs), Buf(CP, n, dtype, off, gs)
        for kind, alpha in ACT_CASES:
            tag = f'{kind}({alpha}) {dtype} n={n} off={off}'
            a = hp(alpha, dtype)
            fwd, bwd = oracle_act(kind, a)
            y = calls.act_fwd(kind, alpha, x, tag + ' fwd')
            if kind == 'relu':
                same_bits(y, fwd(xs).astype(dtype), tag + ' fwd')
            else:
                close(y, fwd(xs), tol, tag + ' fwd')
            dx = calls.act_bwd(kind, alpha, x, dy, tag + ' bwd')
            close(dx, bwd(xs, gs), tol, tag + ' bwd')
            if kind != 'sigmoid':                            # x * mask keeps the sign of a zero result
                assert np.array_equal(np.signbit(y), np.signbit(fwd(xs))), tag + ' fwd: sign of zero'
                assert np.array_equal(np.signbit(dx), np.signbit(bwd(xs, gs))), tag + ' bwd: sign of zero'
            # from the STORED output: the kernel's own arithmetic against float64 on that output, and the whole
            # against the derivative at the input
            yb = Buf(CP, n, dtype, off, y)
            if kind == 'relu':
                with pytest.raises(HipError):
                    calls.act_bwd_from_output(kind, alpha, yb, dy, tag)
                continue
            dx = calls.act_bwd_from_output(kind, alpha, yb, dy, tag + ' bwd from output')
            y64 = np.asarray(y, dtype=np.float64)
            own = gs * y64 * (1 - y64) if kind == 'sigmoid' else gs * np.where(y64 >= 0, 1.0, a)
            close(dx, own, tol, tag + ' bwd from output, on the stored output')
            close(dx, bwd(xs, gs), tol, tag + ' bwd from output == act_bwd')
        close(calls.add(x, dy, f'add {dtype} n={n} off={off}'), xs + gs, tol, f'add {dtype} n={n} off={off}')


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('dtype', DTYPES)
def test_axpy_scale_fill_past_one_grid(dtype, off, gpu):
    from univer_ocr_amd.nn import ops
    CP = gpu(dtype)
    tol = TOL[dtype]
    for n in map_sizes(dtype):
        if n > MAX_GRID * 256 * vec_width(dtype):
            assert wanted_blocks(map_items(n, dtype, off)) > MAX_GRID
        rng = np.random.default_rng(100 + n + off)
        xs, ys = rs(rng.standard_normal(n), dtype), rs(rng.standard_normal(n), dtype)
        tag = f'{dtype} n={n} off={off}'
        x, y = Buf(CP, n, dtype, off, xs), Buf(CP, n, dtype, off, ys)
        ops.axpy(0.375, x.v, y.v)
        close(y.get('axpy ' + tag), ys + 0.375 * xs, tol, 'axpy ' + tag)
        same_bits(x.get('axpy x ' + tag), xs.astype(dtype), 'axpy leaves x alone ' + tag)
        ops.scale_(x.v, -1.7)
        close(x.get('scale ' + tag), hp(-1.7, dtype) * xs, tol, 'scale ' + tag)
        f = Buf(CP, n, dtype, off)
        ops.fill_(f.v, 0.1)
        same_bits(f.get('fill ' + tag), np.full(n, 0.1, dtype=dtype), 'fill ' + tag)


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_has_nan_everywhere_in_the_grid(dtype, off, gpu):
    """The kernel is scalar: its capped grid covers 2048 * 256 elements per trip."""
    from univer_ocr_amd.nn import ops
    CP = gpu(dtype)
    trip = MAX_GRID * 256
    for n in map_sizes(dtype):
        rng = np.random.default_rng(n)
        xs = rng.standard_normal(n)
        where = {0, n - 1, n // 2}
        if n > trip:
            assert wanted_blocks(n) > MAX_GRID
            where |= {trip, trip + 7, n - vec_width(dtype)}       # read in the second trip only
        x = Buf(CP, n, dtype, off, xs)
        assert not ops.has_nan(x.v), f'{dtype} n={n}: NaN reported in finite data'
        inf = xs.copy()
        inf[0], inf[n - 1], inf[n // 2] = np.inf, -np.inf, np.inf
        assert not ops.has_nan(Buf(CP, n, dtype, off, inf).v), f'{dtype} n={n}: +-inf reported as NaN'
        for i in sorted(where):
            bad = xs.copy()
            bad[i] = np.nan
            assert ops.has_nan(Buf(CP, n, dtype, off, bad).v), f'{dtype} n={n} off={off}: NaN at {i} not found'


@pytest.mark.parametrize('src,dst', [(s, d) for s in DTYPES for d in DTYPES if s != d])
def test_convert_all_pairs_bit_for_bit(src, dst, gpu):
    """One thread per element, 2048 blocks at most; values across the binary16 range, its overflow threshold, its
    subnormals and float64 values that a rounding through float32 on the way to binary16 would get wrong."""
    CP = gpu('float32')
    for n in (1, 3, 1023, MAX_GRID * 256 + 5, 4 * MAX_GRID * 256 + 5):
        if n > MAX_GRID * 256:
            assert wanted_blocks(n) > MAX_GRID
        rng = np.random.default_rng(n)
        with np.errstate(over='ignore'):
            host = (rng.standard_normal(n) * np.exp(rng.uniform(-12, 8, n))).astype(src)
        edge = np.array([0.0, -0.0, 65504.0, 65519.0, 65520.0, -70000.0, 6.0e-8, 2.9e-8, 3.1e-8, 1e-40, np.inf, -np.inf,
                         1.0 + 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -30, 1.0 + 3 * 2.0 ** -11])
        k = min(n, edge.size)
        with np.errstate(over='ignore'):
            host[:k] = edge[:k].astype(src)
        for off_s, off_d in ((0, 0), (1, 1)):
            s = Buf(CP, n, src, off_s, host)
            d = Buf(CP, n, dst, off_d)
            CP.runtime().call('uocr_convert', s.v.code, s.v.ptr, d.v.code, d.v.ptr, n)
            with np.errstate(over='ignore'):
                ref = host.astype(dst)
            same_bits(d.get(f'convert {src}->{dst} n={n}'), ref, f'convert {src}->{dst} n={n} off={off_s}')


@pytest.mark.parametrize('dtype', DTYPES)
def test_u8_feed_past_one_grid_and_off_alignment(dtype, gpu):
    """16-pixel kernel: one thread per 16 pixels, so the capped grid covers 2048 * 256 * 16 pixels per trip; the
    fallback (count % 16 != 0, or source / destination off 16-byte alignment) one pixel per thread."""
    from univer_ocr_amd.nn import ops
    CP = gpu(dtype)
    vec_trip = MAX_GRID * 256 * 16

    def ref_of(u8):
        if dtype == 'float64':
            return u8.astype(np.float64) * (1.0 / 255.0)
        return (u8.astype(np.float32) * np.float32(1.0 / 255.0)).astype(dtype)

    # (count, source offset, destination offset, vector kernel?)
    for count, so, do, vec in ((16 * 40, 0, 0, True), (vec_trip + 48, 0, 0, True), (16 * 40, 1, 0, False),
                               (16 * 40, 0, 1, False), (MAX_GRID * 256 + 16, 1, 1, False),
                               (MAX_GRID * 256 + 7, 0, 0, False)):
        if count > vec_trip:
            assert vec and wanted_blocks(count // 16) > MAX_GRID
        elif count > MAX_GRID * 256:
            assert not vec and wanted_blocks(count) > MAX_GRID
        rng = np.random.default_rng(count + so + 2 * do)
        u8 = rng.integers(0, 256, count).astype(np.uint8)
        u8[:3] = (0, 255, 1)
        base = np.full(count + 2 * GUARD + so, 0x5A, dtype=np.uint8)
        base[GUARD + so:GUARD + so + count] = u8
        dev = CP.copy(base, np.uint8)
        src = type(dev)(dev.t[GUARD + so:GUARD + so + count])
        assert (src.ptr % 16 == 0) == (so == 0) and (count % 16 == 0 and so == 0 and do == 0) == vec
        out = Buf(CP, count, dtype, do)
        ops.u8_to_float(src, 1.0 / 255.0, out=out.v)
        same_bits(out.get(f'u8 feed {dtype} count={count}'), ref_of(u8), f'u8 feed {dtype} count={count} src+{so} dst+{do}')
        assert np.array_equal(CP.asnumpy(dev), base)


# ---- 2. copy_2d ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_concat_and_split_past_the_block_cap(dtype, gpu):
    """uocr_copy_2d: one thread per element, 8192 blocks at most.  Last axis: 4100 rows of 1, 3, 5 and 520 columns
    (the wide copy needs 8329 blocks); axis 0: one row of 2 111 500 columns per part."""
    from univer_ocr_amd.nn import ops
    CP = gpu(dtype)
    rng = np.random.default_rng(5)
    lead = (2, 50, 41)
    widths = (1, 520, 3, 5)
    assert wanted_blocks(int(np.prod(lead)) * max(widths)) > SHAPE_GRID
    parts = [rng.standard_normal(lead + (c,)).astype(dtype) for c in widths]
    y = ops.concat([CP.copy(p) for p in parts], axis=-1)
    same_bits(CP.asnumpy(y), np.concatenate(parts, axis=-1), f'concat axis -1 {dtype}')
    g = rng.standard_normal(lead + (sum(widths),)).astype(dtype)
    outs = ops.split(CP.copy(g), [p.shape for p in parts], axis=-1)
    at = 0
    for o, c in zip(outs, widths):
        same_bits(CP.asnumpy(o), np.ascontiguousarray(g[..., at:at + c]), f'split axis -1 {dtype}, {c} columns')
        at += c
    rows = [rng.standard_normal((2050, 1030)).astype(dtype), rng.standard_normal((3, 1030)).astype(dtype),
            rng.standard_normal((2050, 1030)).astype(dtype)]
    assert wanted_blocks(rows[0].size) > SHAPE_GRID
    y0 = ops.concat([CP.copy(p) for p in rows], axis=0)
    same_bits(CP.asnumpy(y0), np.concatenate(rows, axis=0), f'concat axis 0 {dtype}')
    g0 = rng.standard_normal(y0.shape).astype(dtype)
    at = 0
    for o, p in zip(ops.split(CP.copy(g0), [p.shape for p in rows], axis=0), rows):
        same_bits(CP.asnumpy(o), g0[at:at + p.shape[0]], f'split axis 0 {dtype}')
        at += p.shape[0]


# ---- 3. optimizers --------------------------------------------------------------------------------------------------
def opt_state(rng, n, dtype):
    """weights, two gradients, a velocity and accumulated squares in [1e-3, 1) -- as held in `dtype`"""
    return (rs(rng.standard_normal(n), dtype), rs(rng.standard_normal(n), dtype), rs(rng.standard_normal(n), dtype),
            rs(rng.standard_normal(n) * 0.1, dtype), rs(rng.uniform(1e-3, 1.0, n), dtype))


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('opt', ['adam', 'momentum', 'rmsprop'])
def test_optimizer_steps_against_the_oracle(opt, dtype, off, gpu):
    """Two steps from a non-zero state.  Adam moves 16 bytes per thread when all four arrays are aligned, else one
    element, like Momentum and RMSProp always."""
    from univer_ocr_amd.nn import ops
    CP = gpu(dtype)
    tol = TOL[dtype]
    per_thread = vec_width(dtype) if (opt == 'adam' and not off) else 1
    cap = MAX_GRID * 256 * per_thread
    for n in (1, 3, 4, 5, 1027, 300001, cap + 5):
        if n > cap:
            assert wanted_blocks(cdiv(n, per_thread)) > MAX_GRID
        rng = np.random.default_rng(n + off)
        w0, g0, g1, v0, a0 = opt_state(rng, n, dtype)
        w, g, v, a = (Buf(CP, n, dtype, off, d) for d in (w0, g0, v0, a0))
        if opt == 'adam':
            lr, b1, b2 = hp(0.0015, dtype), hp(0.9, dtype), hp(0.999, dtype)
            ref = O.AdamState(lr, b1, b2)
            ref.state['p'] = (v0, a0)
            step = lambda: ops.adam_step(w.v, g.v, v.v, a.v, lr, b1, b2, O.EPS_OPT)          # noqa: E731
        elif opt == 'momentum':
            lr, mu = hp(0.05, dtype), hp(0.9, dtype)
            ref = O.MomentumState(lr, mu)
            ref.state['p'] = v0
            step = lambda: ops.momentum_step(w.v, g.v, v.v, lr, mu)                          # noqa: E731
        else:
            lr, rho = hp(0.01, dtype), hp(0.95, dtype)
            ref = O.RMSPropState(lr, rho)
            ref.state['p'] = a0
            step = lambda: ops.rmsprop_step(w.v, g.v, a.v, lr, rho, O.EPS_OPT)               # noqa: E731
        wr = w0
        for k, grad in enumerate((g0, g1)):
            tag = f'{opt} {dtype} n={n} off={off} step {k + 1}'
            if k:
                g = Buf(CP, n, dtype, off, grad)
            wr = ref.update('p', wr, grad)
            step()
            close(w.get(tag), wr, tol, tag + ' w')
            same_bits(g.get(tag), grad.astype(dtype), tag + ' gradient untouched')
            if opt == 'adam':
                close(v.get(tag), ref.state['p'][0], tol, tag + ' velocity')
                close(a.get(tag), ref.state['p'][1], tol, tag + ' accumulated')
            elif opt == 'momentum':
                close(v.get(tag), ref.state['p'], tol, tag + ' velocity')
            else:
                close(a.get(tag), ref.state['p'], tol, tag + ' accumulated')


# ---- 4. fused optimizer tails -------------------------------------------------------------------------------------------
def fused_ranges(n, wide):
    """Four ranges: one that starts one element into the first vector and ends one short of a vector end, its
    neighbour (three elements across a vector boundary), an empty one -- or, `wide`, one across several grid trips
    with both ends inside vectors -- and the last three elements (the scalar tail when n % 4 == 3)."""
    third = (('l2', 2.0 ** -8), 300001, 700003) if wide else (('l2', 2.0 ** -8), 2049, 2049)
    return [(('l2', 2.0 ** -7), 1, 1023), (('l1', 3 * 2.0 ** -8), 1023, 1026), third, (('l1', 2.0 ** -6), n - 3, n)]


def oracle_fused(opt, w, g, v, a, ranges, hyper):
    """O.l1_reg / O.l2_reg on each range, then the oracle optimizer; returns w, regularised g, state, loss."""
    g = g.copy()
    loss = 0.0
    for (kind, strength), lo, hi in ranges:
        part, dg = (O.l1_reg if kind == 'l1' else O.l2_reg)(w[lo:hi], strength)
        g[lo:hi] += dg
        loss += part
    if opt == 'momentum':
        ref = O.MomentumState(hyper[0], hyper[1])
        ref.state['p'] = v
        w = ref.update('p', w, g)
        return w, g, (ref.state['p'], None), loss
    ref = O.AdamState(hyper[0], hyper[1], hyper[2])
    ref.state['p'] = (v, a)
    w = ref.update('p', w, g)
    return w, g, ref.state['p'], loss


FUSED_CASES = [
    # (n, ranges?, wide third range?, grid cap the case is named after or None)
    (5003, True, False, None),
    (262144 * 4 + 7, True, True, 256),
    (1024 * 1024 + 4099, False, False, 1024),
]


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('case', range(len(FUSED_CASES)))
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('opt', ['momentum', 'adam'])
def test_fused_tails_against_the_oracle(opt, dtype, case, off, gpu):
    """Regularisers on up to four ranges + optimizer step + gradient reset in one launch, compared with the oracle
    (never with the unfused kernels).  Each (zero_grad, hyper) variant runs on fresh copies; the loss of the three
    zero_grad=True runs must be the same double (fixed summation order, arrival counter back at zero)."""
    from univer_ocr_amd.nn import ops
    CP = gpu(dtype)
    tol = TOL[dtype]
    n, with_ranges, wide, cap = FUSED_CASES[case]
    ranges = fused_ranges(n, wide) if with_ranges else []
    if cap is not None:
        assert wanted_blocks(n if off else cdiv(n, 4)) > cap
        assert cap == (256 if ranges else 1024)                   # launch_opt_fused
    rng = np.random.default_rng(n + off)
    w0, g0, _, v0, a0 = opt_state(rng, n, dtype)
    w0[5:1026:3] = 0.0                                            # sign(0) = 0 inside the L1 range and around it
    w0[n - 2] = -0.0
    scalars = (0.05, 0.9, 0.0, 0.0) if opt == 'momentum' else (0.0015, 0.9, 0.999, O.EPS_OPT)
    on_device = (0.02, 0.8, 0.0, 0.0) if opt == 'momentum' else (0.004, 0.85, 0.99, O.EPS_OPT)
    losses = []
    for zero_grad, from_device in ((True, False), (False, False), (True, True), (True, False), (False, True)):
        tag = f'{opt} {dtype} n={n} off={off} zero_grad={zero_grad} hyper={"device" if from_device else "scalars"}'
        w, g, v, a = (Buf(CP, n, dtype, off, d) for d in (w0, g0, v0, a0))
        used = tuple(hp(x, dtype) for x in (on_device if from_device else scalars))
        hyper = CP.copy(np.array(on_device), np.float64) if from_device else None
        if opt == 'momentum':
            loss = ops.momentum_step_fused(w.v, g.v, v.v, scalars[0], scalars[1], ranges, zero_grad, hyper)
        else:
            loss = ops.adam_step_fused(w.v, g.v, v.v, a.v, *scalars, ranges, zero_grad, hyper)
        wr, gr, (vr, ar), lr = oracle_fused(opt, w0, g0, v0, a0, ranges, used)
        close(w.get(tag), wr, tol, tag + ' w')
        close(v.get(tag), vr, tol, tag + ' velocity')
        if opt == 'adam':
            close(a.get(tag), ar, tol, tag + ' accumulated')
        else:
            same_bits(a.get(tag), a0.astype(dtype), tag + ' unused array untouched')
        if zero_grad:
            assert not np.any(g.get(tag)), tag + ': gradient not reset'
        else:
            close(g.get(tag), gr, tol, tag + ' regularised gradient')
        if ranges:
            loss_close(loss, lr, tol, tag + ' regularisation loss')
            losses.append(float(loss))
        else:
            assert loss == 0
    assert len(set(losses)) <= 1, f'regularisation loss differs between identical calls: {losses}'


# ---- 5. unfused regularisers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('kind', ['l1', 'l2'])
def test_regularize_past_the_partial_sum_cap(kind, dtype, gpu):
    """reg_kernel: 1024 elements per block, 512 blocks at most; finish_sum_kernel then adds 512 partials with 256
    threads.  `accumulate` adds into an existing gradient and an existing loss slot."""
    from univer_ocr_amd.nn import ops
    CP = gpu(dtype)
    tol = TOL[dtype]
    strength = 2.0 ** -6
    for n in (60, 1025, 600001):
        if n > 512 * 1024:
            assert wanted_blocks(n, 1024) > 512
        rng = np.random.default_rng(n)
        w0 = rs(rng.standard_normal(n), dtype)
        w0[::5] = 0.0
        g0 = rs(rng.standard_normal(n), dtype)
        ref_loss, ref_dg = (O.l1_reg if kind == 'l1' else O.l2_reg)(w0, strength)
        tag = f'{kind} {dtype} n={n}'
        for off in (0, 1):
            w, g = Buf(CP, n, dtype, off, w0), Buf(CP, n, dtype, off, g0)
            for _ in range(2):                                   # the workspace partials are reused: same value twice
                fresh = Buf(CP, n, dtype, off, np.zeros(n))
                loss = ops.regularize(kind, w.v, fresh.v, strength)
                loss_close(loss, ref_loss, tol, tag)
                close(fresh.get(tag), ref_dg, tol, tag + ' gradient')
            slot = CP.full((1,), 5.0, np.float64)
            ops.regularize(kind, w.v, g.v, strength, slot, accumulate=True)
            close(g.get(tag), g0 + ref_dg, tol, tag + ' accumulated gradient')
            loss_close(float(slot.numpy()[0]), 5.0 + ref_loss, tol, tag + ' accumulated')
            same_bits(w.get(tag), w0.astype(dtype), tag + ' weights untouched')


# ---- 6. cross-entropies ---------------------------------------------------------------------------------------------------
def softmax_blocks(m, c):
    """uocr_softmax_ce: 16 / 32 / 64 lanes per row, 4 waves per block"""
    lanes = 16 if c <= 64 else 32 if c <= 128 else 64
    return cdiv(m, 4 * (64 // lanes))


def loss_and_grad(CP, dtype, call, pred, gt):
    """one loss call in the current mode -> (loss, gradient as float64 with a binary16 gradient scale removed)"""
    loss, grad = call(CP.copy(pred), CP.copy(gt))
    got = CP.asnumpy(grad).astype(np.float64)
    if dtype == 'float16':
        assert grad.gscale > 0
        got = got / 2.0 ** grad.gscale
    return float(loss), got


SOFTMAX_SHAPES = [(4100, 162), (8200, 100), (16400, 37)] + [(37, c) for c in (1, 16, 17, 64, 65, 128, 129, 256, 257, 700)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SOFTMAX_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_softmax_ce_past_1024_blocks_and_across_lane_groups(shape, dtype, gpu):
    """m > 37: more than 1024 blocks, so the last block adds the block losses past its first four rows per
    thread in the strided walk of last_block_fold.  Three calls in a row: the arrival counter must be back at zero each time."""
    from univer_ocr_amd.nn import ops
    CP = gpu(dtype)
    m, c = shape
    if m > 37:
        assert softmax_blocks(m, c) > 4 * 256
    rng = np.random.default_rng(m * 1000 + c)
    pred = rs(rng.standard_normal((m, c)) * 3.0, dtype)
    gt = np.zeros((m, c))
    gt[np.arange(m), rng.integers(0, c, m)] = 1.0
    if c > 1:
        soft = rng.random((3, c))
        gt[:3] = rs(soft / soft.sum(axis=1, keepdims=True), dtype)     # a few rows of soft labels
    ref_loss, ref_grad = O.softmax_ce_loss(pred, gt)
    assert np.isfinite(ref_loss) and np.ptp(pred, axis=1).max() <= 80
    tag = f'softmax CE {dtype} {m}x{c}'
    seen = []
    for _ in range(3):
        loss, grad = loss_and_grad(CP, dtype, ops.softmax_ce, pred, gt)
        loss_close(loss, ref_loss, TOL_FROM16 if dtype == 'float16' else TOL[dtype], tag)
        close(grad, ref_grad, TOL[dtype], tag + ' gradient')
        seen.append(loss)
    assert len(set(seen)) == 1, f'{tag}: {seen}'
    loss, none = ops.softmax_ce(CP.copy(pred), CP.copy(gt), need_grad=False)
    assert none is None and float(loss) == seen[0]


@pytest.mark.parametrize('dtype,offset', [('float64', 1e4), ('float32', 60.0)])
def test_softmax_ce_subtracts_the_row_maximum(dtype, offset, gpu):
    from univer_ocr_amd.nn import ops
    CP = gpu(dtype)
    m, c = 67, 162
    rng = np.random.default_rng(11)
    sign = np.where(rng.random((m, 1)) < 0.5, -1.0, 1.0)
    pred = rs(rng.standard_normal((m, c)) * 3.0 + sign * offset, dtype)
    gt = np.zeros((m, c))
    gt[np.arange(m), rng.integers(0, c, m)] = 1.0
    ref_loss, ref_grad = O.softmax_ce_loss(pred, gt)
    loss, grad = loss_and_grad(CP, dtype, ops.softmax_ce, pred, gt)
    loss_close(loss, ref_loss, TOL[dtype], f'softmax CE {dtype} rows offset by +-{offset}')
    close(grad, ref_grad, TOL[dtype], f'softmax CE {dtype} rows offset by +-{offset}, gradient')


@pytest.mark.parametrize('dtype', DTYPES)
def test_sigmoid_ce_past_the_block_cap(dtype, gpu):
    """1024 elements per block, 512 blocks at most: 524 288 + 1025 elements need 514."""
    from univer_ocr_amd.nn import ops
    CP = gpu(dtype)
    m, c = 512 * 1024 + 1025, 1
    assert wanted_blocks(m * c, 1024) > 512
    rng = np.random.default_rng(12)
    pred = rs(np.clip(rng.standard_normal((m, c)) * 4.0, -12.0, 12.0), dtype)
    gt = (rng.random((m, c)) > 0.7).astype(np.float64)
    ref_loss, ref_grad = O.sigmoid_ce_loss(pred, gt)
    assert np.isfinite(ref_loss)
    seen = []
    for _ in range(3):
        loss, grad = loss_and_grad(CP, dtype, ops.sigmoid_ce, pred, gt)
        loss_close(loss, ref_loss, TOL_FROM16 if dtype == 'float16' else TOL[dtype], f'sigmoid CE {dtype}')
        close(grad, ref_grad, TOL[dtype], f'sigmoid CE {dtype} gradient')
        seen.append(loss)
    assert len(set(seen)) == 1, seen


# ---- 7. Dice / Jaccard -------------------------------------------------------------------------------------------------
def seg_plan(shape, dtype, aligned=True):
    """uocr_seg_loss: (vector kernels?, chunks the sums kernels want before the 64 cap, chunks the vector gradient
    kernel wants before the 512 cap)"""
    n, h, w, c = shape
    hw, elem = h * w, np.dtype(dtype).itemsize
    vec = elem <= 4 and c in (1, 2, 4) and (hw * c * elem) % 16 == 0 and aligned
    return vec, cdiv(hw, 8192), cdiv(hw * c * elem // 16, 1024) if vec else None


SEG_CASES = [
    # (shape, dtype, vector kernels?, cap the case is named after)
    ((1, 768, 768, 1), 'float32', True, 'sums64'),
    ((1, 1024, 1100, 2), 'float32', True, 'grad512'),
    ((2, 130, 130, 4), 'float32', True, None),
    ((2, 97, 101, 3), 'float32', False, None),
    ((2, 95, 97, 1), 'float32', False, None),
    ((1, 768, 768, 1), 'float16', True, 'sums64'),
    ((1, 1024, 2100, 2), 'float16', True, 'grad512'),
    ((2, 130, 130, 4), 'float16', True, None),
    ((2, 97, 101, 3), 'float64', False, None),
    ((1, 768, 768, 1), 'float64', False, 'sums64'),
]


def seg_inputs(rng, shape, dtype):
    pred = rs(rng.random(shape) * 0.98 + 0.01, dtype)
    gt = (rng.random(shape) > 0.6).astype(np.float64)
    if shape[0] > 1:
        gt[0] = 0.0                                    # an image without a single label pixel next to one with
    return pred, gt


def check_seg(CP, ops, dtype, pred, gt, dev_pred, dev_gt, tag):
    for kind, fn in (('dice', O.dice_loss), ('jaccard', O.jaccard_loss)):
        ref_loss, ref_grad = fn(pred, gt)
        for out_act in (None, 'sigmoid'):
            what = f'{kind} {tag} out_act={out_act}'
            loss, grad = ops.seg_loss(kind, dev_pred, dev_gt, True, out_act=out_act)
            got = CP.asnumpy(grad).astype(np.float64)
            if dtype == 'float16':
                assert grad.gscale == ops.f16_grad_scale_log2('seg', pred.shape[1] * pred.shape[2]) > 0
                got = got / 2.0 ** grad.gscale
            loss_close(loss, ref_loss, TOL_FROM16 if dtype == 'float16' else TOL[dtype], what)
            close(got, ref_grad * pred * (1 - pred) if out_act else ref_grad, TOL[dtype], what + ' gradient')
            loss2, none = ops.seg_loss(kind, dev_pred, dev_gt, need_grad=False, out_act=out_act)
            assert none is None and float(loss2) == float(loss), what + ': need_grad=False gives another loss'


@pytest.mark.parametrize('case', range(len(SEG_CASES)), ids=lambda i: f'{SEG_CASES[i][1]}-{"x".join(map(str, SEG_CASES[i][0]))}')
def test_seg_losses_past_their_chunk_caps(case, gpu):
    from univer_ocr_amd.nn import ops
    shape, dtype, vec, cap = SEG_CASES[case]
    CP = gpu(dtype)
    is_vec, sum_chunks, grad_chunks = seg_plan(shape, dtype)
    assert is_vec == vec
    if cap == 'sums64':
        assert sum_chunks > 64
    elif cap == 'grad512':
        assert grad_chunks > 512
    else:
        assert sum_chunks > 1 and (grad_chunks is None or grad_chunks > 1)     # several chunks per image
    rng = np.random.default_rng(case)
    pred, gt = seg_inputs(rng, shape, dtype)
    check_seg(CP, ops, dtype, pred, gt, CP.copy(pred), CP.copy(gt), f'{dtype} {shape}')


@pytest.mark.parametrize('dtype', ['float32', 'float16'])
def test_seg_losses_fall_back_for_unaligned_views(dtype, gpu):
    """A shape the vector kernels would take, through views one element past a 16-byte boundary."""
    from univer_ocr_amd.nn import ops
    CP = gpu(dtype)
    shape = (2, 130, 136, 1)
    assert seg_plan(shape, dtype)[0] and not seg_plan(shape, dtype, aligned=False)[0]
    rng = np.random.default_rng(21)
    pred, gt = seg_inputs(rng, shape, dtype)
    n = pred.size
    p, g = Buf(CP, n, dtype, 1, pred, shape), Buf(CP, n, dtype, 1, gt, shape)
    check_seg(CP, ops, dtype, pred, gt, p.v, g.v, f'{dtype} {shape} views')
    same_bits(p.get('pred'), pred.astype(dtype), 'prediction untouched')
    same_bits(g.get('gt'), gt.astype(dtype), 'labels untouched')


# ---- 8. max-pool, upsample, fixed width ---------------------------------------------------------------------------------------
def quarters(rng, shape, dtype):
    """-0.25, 0 or 0.25: the maximum of most windows is shared (55 % of the 2 x 2 ones), the values are exact in every
    type, and 0 also ties with the zero padding"""
    return (rng.integers(-1, 2, shape) * 0.25).astype(dtype)


POOL_CASES = [
    # (shape, dtype, ks, stride, padding, ceil_mode, what must exceed the 8192-block cap)
    ((2, 2050, 2064, 4), 'float32', (2, 2), (2, 2), (0, 0), False, 'vector'),
    ((3, 1800, 1804, 1), 'float32', (2, 2), (2, 2), (0, 0), False, 'generic'),
    ((2, 301, 403, 3), 'float32', (3, 3), (2, 2), (1, 1), True, None),
    ((3, 1800, 1804, 1), 'float64', (2, 2), (2, 2), (0, 0), False, 'generic'),
    ((3, 1800, 1804, 1), 'float16', (2, 2), (2, 2), (0, 0), False, 'generic'),
    ((2, 301, 403, 3), 'float64', (3, 3), (2, 2), (1, 1), True, None),
]


@pytest.mark.parametrize('case', range(len(POOL_CASES)), ids=lambda i: f'{POOL_CASES[i][1]}-{"x".join(map(str, POOL_CASES[i][0]))}')
def test_maxpool_past_the_block_cap_with_ties(case, gpu):
    from univer_ocr_amd.nn import ops
    shape, dtype, ks, st, pd, ceil, cap = POOL_CASES[case]
    CP = gpu(dtype)
    n, h, w, c = shape
    oh, ow = O.maxpool2d_out_hw(h, w, ks, st, pd, ceil)
    vec = dtype == 'float32' and ks == (2, 2) and st == (2, 2) and pd == (0, 0) and h == 2 * oh and w == 2 * ow and c % 4 == 0
    assert vec == (cap == 'vector')
    if cap == 'vector':
        assert wanted_blocks(n * oh * ow * c // 4) > SHAPE_GRID                # forward and backward: one thread per window quad
    elif cap == 'generic':
        assert wanted_blocks(n * oh * ow * c) > SHAPE_GRID and wanted_blocks(n * h * w * c) > SHAPE_GRID
    rng = np.random.default_rng(case)
    X = quarters(rng, shape, dtype)
    ref_y, ref_mask = O.maxpool2d_fwd(X.astype(np.float64), ks, st, pd, ceil)
    assert np.mean(ref_mask.reshape(n, oh, ks[0], ow, ks[1], c).sum(axis=(2, 4)) > 1) > 0.5     # most windows have ties
    tag = f'maxpool {dtype} {shape} k{ks} s{st} p{pd}'
    y, mask = ops.maxpool2d_fwd(CP.copy(X), ks, st, pd, ceil)
    same_bits(CP.asnumpy(y), ref_y.astype(dtype), tag + ' y')
    same_bits(CP.asnumpy(mask), ref_mask.astype(np.uint8), tag + ' mask')
    g = rs(rng.standard_normal(ref_y.shape), dtype)
    ref_dx = O.maxpool2d_bwd(g, ref_mask, shape, ks, st, pd)
    dx = ops.maxpool2d_bwd(CP.copy(g), mask, shape, ks, st, pd)
    close(CP.asnumpy(dx), ref_dx, TOL[dtype], tag + ' dx')


UPSAMPLE_CASES = [
    # (shape, dtype, scale, vector kernels?)
    ((2, 2050, 2052, 1), 'float32', (2, 2), True),
    ((1, 1025, 2052, 4), 'float32', (2, 2), True),
    ((1, 840, 840, 3), 'float32', (2, 2), False),
    ((1, 730, 730, 4), 'float32', (3, 2), False),
    ((1, 730, 730, 4), 'float64', (3, 2), False),
    ((1, 840, 840, 3), 'float16', (2, 2), False),
]


@pytest.mark.parametrize('case', range(len(UPSAMPLE_CASES)),
                         ids=lambda i: f'{UPSAMPLE_CASES[i][1]}-{"x".join(map(str, UPSAMPLE_CASES[i][0]))}')
def test_upsample_past_the_block_cap(case, gpu):
    from univer_ocr_amd.nn import ops
    shape, dtype, scale, vec = UPSAMPLE_CASES[case]
    CP = gpu(dtype)
    n, h, w, c = shape
    assert vec == (dtype == 'float32' and scale == (2, 2) and c in (1, 4) and (w * c) % 4 == 0)
    # vector kernels: one thread per 16 bytes of the LOW-resolution tensor in both passes; generic: one per output
    # element of the pass (forward: the high-resolution tensor, backward: the low-resolution one)
    assert wanted_blocks(n * h * w * c // 4 if vec else n * h * w * c) > SHAPE_GRID
    rng = np.random.default_rng(case)
    X = rng.standard_normal(shape).astype(dtype)
    tag = f'upsample {dtype} {shape} x{scale}'
    y = ops.upsample2d_fwd(CP.copy(X), scale)
    same_bits(CP.asnumpy(y), O.upsample2d_fwd(X, scale), tag + ' y')
    g = rng.standard_normal((n, h * scale[0], w * scale[1], c)).astype(dtype)
    dx = ops.upsample2d_bwd(CP.copy(g), shape, scale)
    close(CP.asnumpy(dx), O.upsample2d_bwd(g.astype(np.float64), scale), TOL[dtype], tag + ' dx')


@pytest.mark.parametrize('shape,dtype,widths', [((2, 3, 4000, 4), 'float32', (2, 3, 8)),
                                                ((2, 16, 16400, 4), 'float32', (2, 3, 8)),
                                                ((2, 16, 16400, 4), 'float64', (3,)),
                                                ((2, 16, 16400, 4), 'float16', (3,))])
def test_fixed_width_on_long_strips(shape, dtype, widths, gpu):
    """The second shape needs more than 8192 blocks in both passes at every width."""
    from univer_ocr_amd.nn import ops
    CP = gpu(dtype)
    rng = np.random.default_rng(31)
    X = rng.standard_normal(shape).astype(dtype)
    Xd = CP.copy(X)
    for width in widths:
        if shape[1] > 3:
            assert wanted_blocks(X.size) > SHAPE_GRID
        tag = f'fixed width {width} {dtype} {shape}'
        y = ops.fixed_width_fwd(Xd, width)
        same_bits(CP.asnumpy(y), O.fixed_width_fwd(X.astype(np.float64), width).astype(dtype), tag + ' y')
        g = rng.standard_normal(y.shape).astype(dtype)
        dx = ops.fixed_width_bwd(CP.copy(g), shape, width)
        close(CP.asnumpy(dx), O.fixed_width_bwd(g.astype(np.float64), shape, width), TOL[dtype], tag + ' dx')
