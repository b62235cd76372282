"""NaN and Inf reach the weights through every training kernel: the rules of nonfinite_rules.py on the GPU.

Trainer.train defends a run against divergence with Model.nan_weights() alone, so a non-finite value that appears anywhere
in a step must arrive in the weights as NaN, kernel by kernel.  Every other GPU test uses NaN and Inf only as a pre-fill that
finds unwritten outputs, as data for has_nan / convert / zero_gaps, or as a marker for wrong results; here one NaN or Inf is
planted into an OPERAND of each training kernel and the output is judged against the float64 oracle on the same operands by
the four rules (R1 nothing swallowed, R2 nothing crosses images, R3 agreement where both are finite, R4 spread counted;
nonfinite_rules.py states them, test_nonfinite_host.py shows on the CPU that they hold for a float32 restatement and reject
three wrong kernels).  With finite data, state carried from a neighbouring tile or image by the persistent kernels shows as
a small numeric error; with one NaN it is there or it is not.

Kernel level -- the case tables and launch builders of test_gpu_elementwise.py, operands planted in a copy:
  conv, upconv, pair, dense, windows   elementwise_bound.CASES (pages 3 x 37 x 141, max_blocks 0 and 3, `last_conv` asserted):
                                       forward plain and LeakyReLU (x, the centre tap of each weight, a bias), backward-data
                                       plain and masked (dy, a weight); SIGMOID_CASES: the Sigmoid epilogue (x, weight, bias)
  weight gradients                     elementwise_wgrad.WCASES (3 x 20 x 32 and 1 x 13 x 141; `last_conv` / `last_gemm`
                                       asserted): x and dy, overwriting and accumulating, own finish and the deferred group;
                                       one NaN in the value an accumulating call starts from stays NaN, alone
  elementwise and shape kernels        nonfinite_rules.MAP_CASES, float32 and binary16, bad(K) == bad(R) exactly: act_fwd /
                                       act_bwd / act_bwd_from_output, upsample2d, fixed_width, copy_2d (concat, split),
                                       convert, maxpool2d forward and backward with the NaN at each position of a window
  losses                               seg_loss Dice / Jaccard at c = 1, 2, 4 (vector and generic kernels) and 3, float32 and
                                       binary16, with and without out_act='sigmoid', planted in pred and in gt: the loss is
                                       NaN, the planted (image, channel) pair all NaN, every other pair finite and within
                                       tolerance; softmax_ce and sigmoid_ce with one planted row
  regularisers, optimizers             l1_reg / l2_reg; momentum_step, adam_step, rmsprop_step and the two fused steps with
                                       regulariser ranges: NaN in g at the first index, past the first grid trip and at the
                                       last index makes w NaN exactly there, every other element of w and of the state keeps
                                       the bits of a clean run, has_nan(w) is True.  (No gradient scale reaches an optimizer:
                                       the weight-gradient kernels divide it out, which the binary16 WCASES cover.)
Step level -- PageTrainer on 2 x 64 x 128 pages, float32 (four nets, char_width 64) and binary16 (the three page nets; binary16
dense is refused), fused (graph-level fusions, fused optimizer tail) and unfused (every layer its own kernel, regularise +
update + clear one by one), eager and graphs=True: clean steps first (with graphs until the step is captured: the planted
step is a replay), then one step with a NaN in the layers of one run of nonfinite_rules.STEP_RUNS -- an input pixel, a
label, a weight.  Every net the run reaches has nan_weights() True and EVERY parameter NaN everywhere (what the oracle
says: test_nonfinite_host.py); the nets it does not reach stay finite.

Findings.
  * On the parent of the commit that added this file grad_store<_Float16> (loss.hip) stored fminf(fmaxf(NaN, -65504), 65504)
    = -65504: all 28 binary16 seg_loss cases and both binary16 cross-entropy cases failed R1 (every gradient element of the
    planted pair or row -65504 for the oracle's NaN), and 12 of the 16 binary16 step cases ended with finite weights (up to
    6e4) and nan_weights() False (the four that passed: the unfused 'inputs' and 'weights'
    runs).  Fixed there: a NaN is stored as NaN.
  * maxpool2d backward selected (mask ? share : 0) where the reference multiplies share * mask: a non-finite dy reached one
    position of its window instead of four, and a window whose maximum is NaN (no mask bit, count 0) gave 0 for the oracle's
    NaN.  Fixed in shape_ops.hip (both kernels take the product); no net uses the layer.
  * upconv_inf and border_dy below: kept as strict expected failures (18 cases), each with its reason.
  * Nothing crossed an image, a row or an (image, channel) pair in any kernel, at max_blocks 0 or 3; no elementwise, shape,
    regulariser or optimizer kernel spread (R4: 0 everywhere).
Spread (R4; printed per case with -s; summed over a case's plants, outputs and both max_blocks):
    float32 forward / backward-data: 0 for every table kernel, the MFMA conv, the generic conv, both upconvs, the pair, dense and
    windows, but 768 each for table6 / table7 under the default dispatch (the tiled and t32 Toeplitz kernels);
    binary16: 0 with h16 = 0; the conv_h16 MFMA kernels 992 .. 1760 (table3 .. table7), up4 464, their Sigmoid forms 144 .. 652,
    the pair with a Sigmoid 4; all inside the planted image.
    weight gradients (other taps and channels of dw; summed over the launch forms too): 20 .. 440 per case, 0 for dense,
    windows, the MFMA and generic conv and table0 / table8; db never.

Measured on MI355X: the whole file runs in 25 s (332 cases: 314 pass, 18 expected failures); its longest case takes 1.4 s
(32-pair), the step-level cases 0.1 .. 0.3 s each.
"""
import collections
import contextlib

import numpy as np
import pytest

import elementwise_bound as B
import elementwise_wgrad as W
import nonfinite_rules as N
import test_f16_training_host as H16
import test_f32_training_host as H32
from test_gpu_conv_padding import DEFAULTS, KERNELS, KID, ctx  # noqa: F401  (ctx: the NaN-filling fixture)
from test_gpu_elementwise import CAPS, launches, wgrad_call
from test_gpu_gemm_configs import GEMM_DEFAULTS, WS_HALF, expect_gemm

pytestmark = pytest.mark.gpu

MINUS = N.minus_cases(B.CASES + B.SIGMOID_CASES)
WMINUS = N.minus_cases(W.WCASES)
_PLANTED = collections.OrderedDict()


def replanted(p, plant):
    """nonfinite_rules.replanted, remembered for the neighbouring cases that run the same problem under other options (the
    planted copy keeps its oracle outputs and sums)"""
    key = (id(p), plant.id)
    if key not in _PLANTED:
        _PLANTED[key] = N.replanted(p, plant.changes)
        while len(_PLANTED) > 40:
            _PLANTED.popitem(last=False)
    return _PLANTED[key]


def upconv_inf(c, plant):
    """FINDING (conv_up.hip, both types, every upconv case): +-Inf in x or dy comes out as +-Inf where the oracle has NaN.
    The kernels work on the low-resolution tensor with the taps that fall on one low-resolution pixel summed beforehand
    (up_phase.h): Inf * (w_a + w_b) is +-Inf, the oracle's Inf * w_a + Inf * w_b with weights of opposite sign is NaN -- and
    behind a Sigmoid epilogue the kernel's v = +-Inf gives a finite 0 or 1.  Keeping the NaN would mean multiplying every
    tap by itself, which is the kernel this one replaces.  A NaN in x or dy, and NaN or Inf in a weight or bias, pass."""
    p = c.problem.base if isinstance(c.problem, B.SigmoidProblem) else c.problem
    return isinstance(p, B.UpProblem) and any(k in ('x', 'g') and np.isinf(v) for k, (_, v) in plant.changes.items())


UP_CASES = [i for i, c in enumerate(B.CASES) if isinstance(c.problem, B.UpProblem)]
UP_SIGMOID_CASES = [i for i, c in enumerate(B.SIGMOID_CASES) if isinstance(c.problem.base, B.UpProblem)]


def planted_outputs(CP, c, findings=False):
    """every plant of case `c` (elementwise_bound) x every judged output x max_blocks 0 and 3 -> the misses; findings: only
    the plants of the known finding (upconv_inf) instead of all the others"""
    rt = CP.runtime()
    p = c.problem
    for key, value in DEFAULTS:
        rt.set_option(key, c.opts.get(key, value))
    CP.set_dtype(p.dtype)
    failures, spread = [], {}
    for plant in N.plants(p, c.id in MINUS):
        names = [n for n in c.outputs if plant.outputs is None or n in plant.outputs]
        if not names or upconv_inf(c, plant) != findings:
            continue
        pp = replanted(p, plant)
        run = launches(CP, c._replace(problem=pp))
        ref, tols = N.reference(pp), N.tolerances(pp, c.operand16)
        for name in names:
            launch, entry = run[name]
            for cap in CAPS:
                rt.set_option('max_blocks', cap)
                try:
                    got = launch()
                    noted = rt.last_conv()
                finally:
                    rt.set_option('max_blocks', 0)
                what = f'{c.id} {plant.id} {name} max_blocks={cap}'
                if entry is not None and noted != (entry, KID[c.kernels[name]]):
                    failures.append(f'{what}: last_conv {noted} ({KERNELS[noted[1]]}) != {c.kernels[name]}')
                host = CP.asnumpy(got)
                assert host.dtype == B.STORE[p.dtype], (what, host.dtype)
                verdict = N.judge(what, host, ref[name], tols[name], plant.image, N.image_ids(pp, name), judged=pp.judged(name))
                failures += verdict.failures
                spread[name] = spread.get(name, 0) + verdict.spread
    print(f'{c.id}: spread (non-finite where the oracle is finite, summed over the plants) ' +
          ', '.join(f'{k} {v}' for k, v in spread.items()))
    return failures


@pytest.mark.parametrize('index', range(len(B.CASES)), ids=B.CASE_IDS)
def test_planted_forward_and_backward_data(index, ctx):
    failures = planted_outputs(ctx, B.CASES[index])
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('index', range(len(B.SIGMOID_CASES)), ids=B.SIGMOID_IDS)
def test_planted_sigmoid_epilogue(index, ctx):
    failures = planted_outputs(ctx, B.SIGMOID_CASES[index])
    assert not failures, '\n'.join(failures)


@pytest.mark.xfail(strict=True, reason='upconv: Inf * (sum of the taps of a phase) is Inf where the oracle has NaN (upconv_inf)')
@pytest.mark.parametrize('index', UP_CASES, ids=[B.CASE_IDS[i] for i in UP_CASES])
def test_finding_upconv_turns_an_inf_into_inf_not_nan(index, ctx):
    failures = planted_outputs(ctx, B.CASES[index], findings=True)
    assert not failures, '\n'.join(failures)


@pytest.mark.xfail(strict=True, reason='upconv + Sigmoid: v = +-Inf gives 0 or 1 where the oracle has NaN (upconv_inf)')
@pytest.mark.parametrize('index', UP_SIGMOID_CASES, ids=[B.SIGMOID_IDS[i] for i in UP_SIGMOID_CASES])
def test_finding_upconv_sigmoid_turns_an_inf_into_a_number(index, ctx):
    failures = planted_outputs(ctx, B.SIGMOID_CASES[index], findings=True)
    assert not failures, '\n'.join(failures)


# ---- weight gradients ------------------------------------------------------------------------------------------------------
FORMS = ((0, False, False), (3, False, False), (0, True, False), (3, True, False), (0, True, True))   # max_blocks, accumulate, deferred


def border_dy(c, plant):
    """FINDING (conv_c16_wgrad of conv_fast.hip -- float32 3x3 16 -> 1 at a zero padding value -- and dw2 of the float32
    conv_pair_bwd, the same conv inside the pair): a NaN or Inf in dy at a BORDER pixel reaches only the taps whose x lies
    inside the image.  The oracle's dw sums over the padded x, so the taps that fall into the padding get 0 * NaN = NaN
    as well; these kernels are x-stationary, walk the pixels of the image alone and never form that product (every other
    weight-gradient kernel clamps and selects, and does).  dw always holds NaN at the taps inside (the centre tap at
    least), so has_nan still sees the step; making the kernels agree would mean walking the padded border too."""
    affected = isinstance(c.problem, W.PairWgradProblem) or (c.kernel is not None and c.kernel[1] == 'c16_wgrad')
    return affected and plant.id.startswith(('g[first]', 'g[last]'))


BORDER_CASES = [i for i, c in enumerate(W.WCASES)
                if isinstance(c.problem, W.PairWgradProblem) or (c.kernel is not None and c.kernel[1] == 'c16_wgrad')]


def planted_weight_gradients(CP, c, findings=False):
    rt = CP.runtime()
    p = c.problem
    options = dict(DEFAULTS)
    options.update(GEMM_DEFAULTS)
    options.update(c.opts)
    for key, value in options.items():
        rt.set_option(key, value)
    CP.set_dtype(p.dtype)
    cu = rt.device_info()['cu_count']
    failures, spread = [], {}

    def run(pp, what, forms, start):
        call = wgrad_call(CP, c._replace(problem=pp))
        ref = N.reference(pp)
        for cap, accumulate, deferred in forms:
            tols = N.tolerances(start, accumulate=accumulate) if pp is p else N.tolerances(pp, accumulate=accumulate)
            buffers = {k: CP.copy(start.init[k], np.float32) if accumulate else CP.empty(ref[k].shape, np.float32) for k in p.outputs}
            rt.set_option('max_blocks', cap)
            try:
                with rt.defer_wgrad() if deferred else contextlib.nullcontext():
                    call(buffers, accumulate)
                    noted = rt.last_conv()
            finally:
                rt.set_option('max_blocks', 0)
            form = f'{what} max_blocks={cap} accumulate={accumulate}' + (' deferred' if deferred else '')
            if c.kernel is not None and noted != (c.kernel[0], KID[c.kernel[1]]):
                failures.append(f'{form}: last_conv {noted} ({KERNELS[noted[1]]}) != {c.kernel}')
            if c.gemm is not None and not deferred:
                want = expect_gemm(*c.gemm, True, cu, WS_HALF, options)
                if rt.last_gemm() != want or want[3] < 2:
                    failures.append(f'{form}: last_gemm {rt.last_gemm()} != host rule {want} with two or more slabs')
            for name in p.outputs:
                with np.errstate(all='ignore'):
                    want = ref[name] + start.init[name] if accumulate else ref[name]
                verdict = N.judge(f'{form} {name}', CP.asnumpy(buffers[name]), want, tols[name])
                failures.extend(verdict.failures)
                spread[name] = spread.get(name, 0) + verdict.spread

    try:
        for plant in N.wgrad_plants(p, c.id in WMINUS):
            if border_dy(c, plant) == findings:
                run(replanted(p, plant), f'{c.id} {plant.id}', FORMS, p)
        if not findings:
            # one NaN in the value an accumulating call starts from stays NaN, and nothing else becomes one
            before = dict(spread)
            run(p, f'{c.id} init[centre]=nan', [f for f in FORMS if f[1]], N.with_planted_init(p))
            if spread != before:
                failures.append(f'{c.id}: a NaN in the accumulated value spread: {spread} after {before}')
    finally:
        for key, value in GEMM_DEFAULTS:
            rt.set_option(key, value)
    print(f'{c.id}: spread to other channels and taps (summed over the plants and launch forms) ' +
          ', '.join(f'{k} {v}' for k, v in spread.items()))
    return failures


@pytest.mark.parametrize('index', range(len(W.WCASES)), ids=W.WCASE_IDS)
def test_planted_weight_gradients(index, ctx):
    failures = planted_weight_gradients(ctx, W.WCASES[index])
    assert not failures, '\n'.join(failures)


@pytest.mark.xfail(strict=True, reason='x-stationary 16 -> 1 weight gradient: dy at a border pixel never meets the zero padding (border_dy)')
@pytest.mark.parametrize('index', BORDER_CASES, ids=[W.WCASE_IDS[i] for i in BORDER_CASES])
def test_finding_border_dy_skips_the_taps_in_the_padding(index, ctx):
    failures = planted_weight_gradients(ctx, W.WCASES[index], findings=True)
    assert not failures, '\n'.join(failures)


# ---- elementwise and shape kernels -----------------------------------------------------------------------------------------
def map_launch(CP, case_id, d, dtype):
    """{output: DeviceArray} of MapCase `case_id` on the device operands `d`"""
    from univer_ocr_amd.nn import ops
    op, _, kind = case_id.partition('-')
    if op == 'act_fwd':
        return dict(y=ops.act_fwd(kind, d['x'], N.ALPHA))
    if op == 'act_bwd':
        return dict(dx=ops.act_bwd(kind, d['x'], d['dy'], N.ALPHA))
    if op == 'act_bwd_from_output':
        return dict(dx=ops.act_bwd_from_output(kind, d['y'], d['dy'], N.ALPHA))
    if op == 'upsample2d':
        return dict(y=ops.upsample2d_fwd(d['x'], (2, 2)), dx=ops.upsample2d_bwd(d['g'], d['x'].shape, (2, 2)))
    if op == 'fixed_width':
        return dict(y=ops.fixed_width_fwd(d['x'], 8), dx=ops.fixed_width_bwd(d['g'], d['x'].shape, 8))
    if op == 'copy_2d':
        cat = ops.concat([d['a'], d['b']])
        part_a, part_b = ops.split(cat, [d['a'].shape, d['b'].shape])
        return dict(cat=cat, part_a=part_a, part_b=part_b)
    if op == 'convert':
        out = CP.empty(d['x'].shape, np.float16 if dtype == 'float32' else np.float32)
        CP.runtime().call('uocr_convert', d['x'].code, d['x'].ptr, out.code, out.ptr, out.size)
        return dict(y=out)
    assert op == 'maxpool2d'
    y, mask = ops.maxpool2d_fwd(d['x'], (2, 2), (2, 2), (0, 0))
    return dict(y=y, mask=mask, dx=ops.maxpool2d_bwd(d['g'], mask, d['x'].shape, (2, 2), (2, 2), (0, 0)))


@pytest.mark.parametrize('dtype', ['float32', 'float16'])
@pytest.mark.parametrize('index', range(len(N.MAP_CASES)), ids=N.MAP_IDS)
def test_planted_elementwise_and_shape_kernels(index, dtype, ctx):
    """bad(K) == bad(R) exactly; a copy keeps the bits, everything else the tolerance of test_gpu_streaming_ops"""
    CP = ctx
    CP.set_dtype(dtype)
    c = N.MAP_CASES[index]
    q = c.operands(dtype)
    failures, spread = [], 0
    for plant in c.plants(q):
        qq = c.changed(q, plant)
        ref = c.reference(qq)
        got = map_launch(CP, c.id, {k: CP.copy(v) for k, v in qq.items()}, dtype)
        for name in c.outputs:
            K = CP.asnumpy(got[name])
            with np.errstate(over='ignore'):
                R = ref[name] if c.outputs[name] == 'close' else ref[name].astype(K.dtype).astype(np.float64)
            verdict = N.judge(f'{c.id} {dtype} {plant.id} {name}', K, R, c.tolerance(name, R, dtype),
                              plant.image if c.per_image else None, c.images(name, R), exact=True)
            failures += verdict.failures
            spread += verdict.spread
    print(f'{c.id} {dtype}: spread {spread}')
    assert not failures, '\n'.join(failures)


# ---- losses ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('index', range(len(N.SEG_CASES)), ids=N.SEG_IDS)
def test_planted_seg_loss(index, ctx):
    from univer_ocr_amd.nn import ops
    CP = ctx
    c = N.SEG_CASES[index]
    p = c.problem
    CP.set_dtype(p.dtype)
    pairs = N.seg_pairs(p.q['y'].shape)
    failures, spread = [], 0
    for plant in N.seg_plants(p.q, minus=index % 14 == 0):
        q = dict(p.q)
        for key, (at, value) in plant.changes.items():
            q[key] = N.put(q[key], at, value)
        ref_loss, R = N.seg_reference(c, q)
        what = f'{c.id} {plant.id}'
        loss, grad = ops.seg_loss(c.kind, CP.copy(q['y']), CP.copy(q['gt']), True, c.out_act)
        assert getattr(grad, 'gscale', 0) == p.gscale, (what, grad.gscale, p.gscale)
        if not np.isnan(float(loss)):
            failures.append(f'{what}: the loss is {float(loss)!r}, the oracle\'s {ref_loss!r}')
        K = CP.asnumpy(grad)
        planted = np.broadcast_to(pairs == plant.image, K.shape)
        if not np.isnan(K[planted]).all():
            failures.append(f'{what}: {int((~np.isnan(K[planted])).sum())} of {int(planted.sum())} gradient elements of the planted '
                            f'(image, channel) pair are not NaN, first {K[planted][~np.isnan(K[planted])][0]!r}')
        verdict = N.judge(what, K, R, N.seg_tolerance(c, q, R), plant.image, pairs, saturating=p.half)
        failures += verdict.failures
        spread += verdict.spread
        loss_only, none = ops.seg_loss(c.kind, CP.copy(q['y']), CP.copy(q['gt']), False, c.out_act)
        if none is not None or not np.isnan(float(loss_only)):
            failures.append(f'{what}: need_grad=False gives the loss {float(loss_only)!r}')
    print(f'{c.id}: spread {spread}')
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dtype', ['float32', 'float16'])
@pytest.mark.parametrize('kind', ['softmax', 'sigmoid'])
def test_planted_cross_entropy(kind, dtype, ctx):
    """one planted row: the loss is non-finite as the oracle's, the other rows of the gradient are finite and right"""
    from univer_ocr_amd.nn import ops
    CP = ctx
    CP.set_dtype(dtype)
    call = ops.softmax_ce if kind == 'softmax' else ops.sigmoid_ce
    failures, spread = [], 0
    for shape in N.CE_SHAPES:
        q = N.ce_operands(shape, dtype, kind == 'softmax')
        rows = np.arange(shape[0])[:, None]
        for where, at in N.positions(shape).items():
            for value in N.CE_VALUES[kind]:
                qq = dict(q, pred=N.put(q['pred'], at, value))
                ref_loss, R = N.ce_reference(kind, qq)
                what = f'{kind}_ce {dtype} {shape} pred[{where}]={N.describe(value)}'
                loss, grad = call(CP.copy(qq['pred']), CP.copy(qq['gt']))
                R = R * 2.0 ** getattr(grad, 'gscale', 0)
                tol = N.TOL[dtype] * np.abs(R[np.isfinite(R)]).max()
                failures += N.judge(what + ' loss', float(loss), ref_loss, 0.0).failures
                verdict = N.judge(what, CP.asnumpy(grad), R, tol, at[0], rows, saturating=dtype == 'float16')
                failures += verdict.failures
                spread += verdict.spread
    print(f'{kind}_ce {dtype}: spread {spread}')
    assert not failures, '\n'.join(failures)


# ---- regularisers and optimizers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['l1', 'l2'])
def test_planted_regularisers(kind, ctx):
    from univer_ocr_amd.nn import ops
    CP = ctx
    rng = np.random.default_rng(3)
    w, g0 = (rng.standard_normal(5003).astype(np.float32).astype(np.float64) for _ in range(2))
    failures = []
    for where, at in N.positions(w.shape).items():
        for value in N.ALL_VALUES:
            ref_loss, R = N.reg_reference(kind, N.put(w, at, value), g0, 2.0 ** -6)
            wd, gd = CP.copy(N.put(w, at, value), np.float32), CP.copy(g0, np.float32)
            loss = ops.regularize(kind, wd, gd, 2.0 ** -6)
            what = f'{kind}_reg w[{where}]={N.describe(value)}'
            failures += N.judge(what + ' loss', float(loss), ref_loss, 0.0).failures
            failures += N.judge(what, CP.asnumpy(gd), R, N.TOL['float32'] * np.abs(R[np.isfinite(R)]).max(), exact=True).failures
    assert not failures, '\n'.join(failures)


OPT_TRIP = 2048 * 256 * 4          # elements of the first grid trip of the widest launcher (uocr_adam_step: 2048 blocks of
OPT_N = OPT_TRIP + 4101            # 256 threads, 16 bytes each); the others cover fewer


@pytest.mark.parametrize('opt', N.OPTIMIZERS)
def test_planted_optimizer_steps(opt, ctx):
    """NaN in g at the first index, past the first grid trip and at the last index: w is NaN exactly there, every other element
    of w and of the state keeps the bits of a clean run (which agrees with the oracle where test_gpu_streaming_ops.py
    says), has_nan(w) is True and, for the clean run, False."""
    from univer_ocr_amd.nn import ops
    CP = ctx
    n = OPT_N
    rng = np.random.default_rng(5)
    w0, g0, v0 = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    a0 = rng.uniform(1e-3, 1.0, n).astype(np.float32)
    spots = list(N.opt_spots(n, OPT_TRIP))
    assert spots[1] > OPT_TRIP
    base = opt.split('_')[0]
    hyper = N.OPT_HYPER[base]

    def step(g_host):
        w, g, v, a = (CP.copy(x, np.float32) for x in (w0, g_host, v0, a0))
        if opt == 'momentum':
            ops.momentum_step(w, g, v, *hyper)
        elif opt == 'adam':
            ops.adam_step(w, g, v, a, *hyper, 1e-8)
        elif opt == 'rmsprop':
            ops.rmsprop_step(w, g, a, *hyper, 1e-8)
        elif opt == 'momentum_fused':
            ops.momentum_step_fused(w, g, v, *hyper, N.OPT_RANGES(n))
        else:
            ops.adam_step_fused(w, g, v, a, *hyper, 1e-8, N.OPT_RANGES(n))
        return ops.has_nan(w), [CP.asnumpy(x) for x in (w, v, a)]

    clean_flag, clean = step(g0)
    gp = g0.copy()
    gp[spots] = np.nan
    flag, planted = step(gp)
    assert not clean_flag and all(np.isfinite(x).all() for x in clean)
    assert flag, f'{opt}: has_nan(w) is False after a step with NaN in the gradient'
    assert np.array_equal(np.flatnonzero(np.isnan(planted[0])), spots), \
        f'{opt}: w is NaN at {np.flatnonzero(np.isnan(planted[0]))[:8]}, planted {spots}'
    keep = np.ones(n, bool)
    keep[spots] = False
    for name, got, want in zip(('w', 'velocity', 'accumulated'), planted, clean):
        assert np.array_equal(got[keep].view(np.uint32), want[keep].view(np.uint32)), f'{opt}: {name} differs from the clean run'
        assert not np.isinf(got).any(), f'{opt}: {name} holds an Inf'
    # the oracle: what it keeps NaN in the state, the kernel keeps NaN
    ref = N.opt_reference(opt, *(x.astype(np.float64) for x in (w0, gp, v0, a0)))
    for name, got, want in zip(('w', 'velocity', 'accumulated'), planted, ref):
        assert np.array_equal(np.isnan(got), np.isnan(want)), f'{opt}: {name} is NaN elsewhere than the oracle\'s'


# ---- step level ------------------------------------------------------------------------------------------------------------------
def nest(flat):
    out = {}
    for key, value in flat.items():
        layer, pname = key.rsplit('/', 1)
        out.setdefault(layer, {})[pname] = value.tolist()
    return out


@pytest.fixture
def modes():
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    lazy = CP.lazy_losses
    yield CP
    CP.set_dtype('float32')
    CP.f16_grad_scale_log2 = None
    CP.lazy_losses = lazy


@pytest.mark.parametrize('run', list(N.STEP_RUNS))
@pytest.mark.parametrize('graphs', [False, True], ids=['eager', 'graphs'])
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'unfused'])
@pytest.mark.parametrize('dtype', ['float32', 'float16'])
def test_one_nan_in_a_step_reaches_every_weight(dtype, fused, graphs, run, modes, monkeypatch):
    import torch
    from univer_ocr_amd.my_model.trainer import PageTrainer
    from univer_ocr_amd.nn.models import Model
    CP = modes
    CP.set_dtype(dtype)
    CP.lazy_losses = True
    half = dtype == 'float16'
    host = H16 if half else H32
    nets = H16.PAGE_NETS if half else H32.ALL_NETS
    if not fused:                                        # regularise, update and clear one by one
        monkeypatch.setattr(Model, '_fused_tail_plan', lambda self: None)
    trainer = PageTrainer(*host.PAGE, optimizer='sgd', lr=host.LR, seed=3, nets=nets, graphs=graphs, fuse=fused)
    assert trainer.lanes is not None and trainer.graphs == graphs
    for name, model in trainer.models.items():
        model.set_weights(nest(H16.analytic_net(name).params))
        assert model.has_fused_tail() == fused
    batch = host.page_batch(1)
    for _ in range(3 if graphs else 1):                  # clean steps: eager, eager, capture
        trainer.step(trainer.make_context(batch))
    trainer.join()
    assert (trainer._captured is not None) == graphs
    for name, model in trainer.models.items():
        assert not model.nan_weights(), f'{name}: NaN weights after the clean steps'
    layers, hit, spared = N.STEP_RUNS[run]
    if run == 'weights':
        torch.cuda.synchronize()
        for name, model in trainer.models.items():
            model.params()[N.first_weight(model.params())].value.t.view(-1)[0] = float('nan')
        torch.cuda.synchronize()
    context = trainer.make_context(N.planted_batch(batch, [k for k in layers if k in batch]))
    trainer.step(context)                                # with graphs: a replay
    trainer.join()
    torch.cuda.synchronize()
    failures = []
    for name, model in trainer.models.items():
        values = {pn: p.value.numpy() for pn, p in model.params().items()}
        if name in hit:
            if not model.nan_weights():
                failures.append(f'{name}: nan_weights() is False after the planted step')
            for pn, v in values.items():
                if not np.isnan(v).all():
                    failures.append(f'{name} {pn}: {int((~np.isnan(v)).sum())} of {v.size} elements are not NaN, largest finite '
                                    f'{np.nanmax(np.abs(np.where(np.isfinite(v), v, np.nan))):.3e}')
        else:
            assert name in spared
            if model.nan_weights() or not all(np.isfinite(v).all() for v in values.values()):
                failures.append(f'{name}: not planted in this run, but its weights are not finite')
    assert not failures, '\n'.join(failures)
