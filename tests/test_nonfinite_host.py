"""The rules of nonfinite_rules.py on the CPU: for every kernel case that test_gpu_nonfinite.py plants a NaN or an Inf into,
the float64 oracle gives the rules something to judge, a float32 NumPy restatement of the oracle passes all four, and three
wrong kernels do not:
  (a) the non-finite elements clipped to +-65504 with NaN mapped to -65504 -- what grad_store<_Float16> of loss.hip did:
      R1 must fail;
  (b) one NaN copied into another image: R2 must fail;
  (c) for an exact-set kernel, one NaN more: R4 must fail.
Per case and plant it also asserts that the oracle's non-finite set is not empty (nonfinite_rules.ORACLE_ABSORBS lists the
plants the oracle itself absorbs, and why), that it leaves every other image finite where the output is per image, and
that the case's tolerance, evaluated on the planted operands, is non-finite only where the oracle is.

Step level: for every net and every plant of nonfinite_rules.STEP_RUNS, one NaN makes EVERY element of EVERY parameter
gradient of O.make_net(...).data_grads NaN -- NaN, not merely non-finite: has_nan does not count +-Inf -- at the analytic
weights on the 2 x 64 x 128 page batches (float32: test_f32_training_host.page_case, char_width 64; binary16:
test_f16_training_host.page_case on the rounded input), and the nets a run does not plant stay finite.  A plant for which
the oracle does not give NaN everywhere is not used at step level: a NaN in ONE channel of a Line label or ONE class of a
Char label leaves the other columns of the last layer's weight gradient finite, so labels are planted in every channel of
one position (nonfinite_rules.LABEL_LAYERS).
"""
import numpy as np
import pytest

import elementwise_bound as B
import elementwise_wgrad as W
import nonfinite_rules as N
import test_f16_training_host as H16
import test_f32_training_host as H32
from oracle import nn_oracle as O


def distinct(cases):
    """the cases of a table with distinct (problem, rounded operands, outputs): the option sets of one problem share them"""
    seen, out = set(), []
    for c in cases:
        key = (id(c.problem), getattr(c, 'operand16', ()), getattr(c, 'outputs', ()))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def check(what, restated, R, tol, images, image, exact=False, saturating=False, judged=None, absorbed=False):
    """the assertions of the module docstring for one output of one plant"""
    assert absorbed or N.bad(R).any(), f'{what}: the oracle stays finite'
    if images is not None and image is not None:
        assert not (N.bad(R) & np.broadcast_to(images != image, R.shape)).any(), f'{what}: the oracle leaves image {image}'
    assert N.tolerance_is_sound(tol, R), f'{what}: the tolerance is non-finite where the oracle is finite'
    kw = dict(image=image, images=images, exact=exact, saturating=saturating, judged=judged)
    verdict = N.judge(what, restated, R, tol, **kw)
    assert not verdict.failures, verdict.failures
    if N.bad(R).any():
        mutant = np.where(N.bad(restated), N.clamped(restated), restated)
        assert any(' R1 ' in f for f in N.judge(what, mutant, R, tol, **kw).failures), f'{what}: the clamp passes R1'
    if images is not None and image is not None and np.asarray(images).max() > 0:
        assert any(' R2 ' in f for f in N.judge(what, N.leaked(restated, images, image), R, tol, **kw).failures), \
            f'{what}: a NaN in another image passes R2'
    if exact:
        assert any(' R4 ' in f for f in N.judge(what, N.one_more(restated), R, tol, **kw).failures), f'{what}: one NaN more passes R4'
    return verdict.spread


CONV = distinct(B.CASES + B.SIGMOID_CASES)
MINUS = N.minus_cases(B.CASES + B.SIGMOID_CASES)


@pytest.mark.parametrize('index', range(len(CONV)), ids=[c.id for c in CONV])
def test_conv_cases_on_the_host(index):
    c = CONV[index]
    p = c.problem
    for plant in N.plants(p, c.id in MINUS):
        pp = N.replanted(p, plant.changes)
        ref, tol, low = N.reference(pp), N.tolerances(pp, c.operand16), N.restated(pp)
        for name in c.outputs:
            if plant.outputs is not None and name not in plant.outputs:
                continue
            # +-Inf into a Sigmoid is legitimately 1 or 0: one infinite term makes v infinite, not NaN
            sigmoid_of_inf = isinstance(p, B.SigmoidProblem) and any(np.isinf(v) for _, v in plant.changes.values())
            check(f'{c.id} {plant.id} {name}', low[name], ref[name], tol[name], N.image_ids(pp, name), plant.image,
                  judged=pp.judged(name), absorbed=sigmoid_of_inf)


WGRAD = distinct(W.WCASES)
WMINUS = N.minus_cases(W.WCASES)


@pytest.mark.parametrize('index', range(len(WGRAD)), ids=[c.id for c in WGRAD])
def test_weight_gradient_cases_on_the_host(index):
    c = WGRAD[index]
    p = c.problem
    for plant in N.wgrad_plants(p, c.id in WMINUS):
        pp = N.replanted(p, plant.changes)
        ref, low = N.reference(pp), N.restated(pp)
        # (x does not reach db, and nothing reaches a switched-off bias: some output must be non-finite, not each)
        unused = plant.id.startswith('x[last]') and isinstance(p, W.ConvWgradProblem) and N.last_pixel_unused(p.d)
        assert any(N.bad(ref[name]).any() for name in p.outputs) != unused, f'{c.id} {plant.id}: the oracle stays finite'
        for accumulate in (False, True):
            tol = N.tolerances(pp, accumulate=accumulate)
            for name in p.outputs:
                with np.errstate(all='ignore'):
                    want = pp.expected(name, accumulate)
                    got = low[name] + pp.init[name] if accumulate else low[name]
                check(f'{c.id} {plant.id} {name} accumulate={accumulate}', got, want, tol[name], None, None, absorbed=True)
    # one NaN in the value an accumulating call starts from stays NaN, and only there
    pi = N.with_planted_init(p)
    for name in p.outputs:
        want = pi.expected(name, True)
        assert np.array_equal(N.bad(want), N.bad(pi.init[name])) and N.bad(want).sum() == 1
        check(f'{c.id} init {name}', p.restated()[name] + pi.init[name], want, pi.tolerances(True)[name], None, None)


@pytest.mark.parametrize('dtype', ['float32', 'float16'])
@pytest.mark.parametrize('index', range(len(N.MAP_CASES)), ids=N.MAP_IDS)
def test_elementwise_and_shape_cases_on_the_host(index, dtype):
    c = N.MAP_CASES[index]
    q = c.operands(dtype)
    for plant in c.plants(q):
        qq = c.changed(q, plant)
        ref, low = c.reference(qq), c.restated(qq, dtype)
        reached = False
        for name in c.outputs:
            R = ref[name]
            reached |= bool(N.bad(R).any())
            check(f'{c.id} {dtype} {plant.id} {name}', low[name], R, c.tolerance(name, R, dtype), c.images(name, R),
                  plant.image if c.per_image else None, exact=c.exact and N.bad(R).any(), absorbed=True)
        assert reached != N.absorbed(c.id, plant), f'{c.id} {plant.id}: the oracle is {"non-" if reached else ""}finite'


@pytest.mark.parametrize('index', range(len(N.SEG_CASES)), ids=N.SEG_IDS)
def test_seg_loss_cases_on_the_host(index):
    """Every plant makes the loss NaN and every gradient element of the planted (image, channel) pair NaN; the restatement
    is the float32 one of elementwise_bound.FromOutputProblem (coefficients rounded to float32)."""
    c = N.SEG_CASES[index]
    p = c.problem
    pairs = N.seg_pairs(p.q['y'].shape)
    for plant in N.seg_plants(p.q, minus=index % 14 == 0):
        q = dict(p.q)
        for key, (at, value) in plant.changes.items():
            q[key] = N.put(q[key], at, value)
        loss, R = N.seg_reference(c, q)
        assert np.isnan(loss), (c.id, plant.id, loss)
        assert np.isnan(R[np.broadcast_to(pairs == plant.image, R.shape)]).all(), (c.id, plant.id)
        with np.errstate(all='ignore'):
            ca, cb = p.coefficients(q, np.float32)
            low = (ca * q['gt'].astype(np.float32) + cb).astype(np.float64)
            if c.out_act:
                y = q['y'].astype(np.float32)
                low = (low.astype(np.float32) * (y * (np.float32(1) - y))).astype(np.float64)
            if p.half:
                low = low.astype(np.float16).astype(np.float64)
        check(f'{c.id} {plant.id}', low, R, N.seg_tolerance(c, q, R), pairs, plant.image, saturating=p.half)


@pytest.mark.parametrize('kind', ['softmax', 'sigmoid'])
def test_cross_entropy_cases_on_the_host(kind):
    """One planted row: the oracle's loss is non-finite, its gradient leaves every other row finite."""
    for shape in N.CE_SHAPES:
        q = N.ce_operands(shape, 'float32', kind == 'softmax')
        rows = np.arange(shape[0])[:, None]
        for where, at in N.positions(shape).items():
            for value in N.CE_VALUES[kind]:
                qq = dict(q, pred=N.put(q['pred'], at, value))
                loss, R = N.ce_reference(kind, qq)
                assert not np.isfinite(loss), (kind, where, value, loss)
                assert not (N.bad(R) & (rows != at[0])).any()
                low = N.ce_reference(kind, {k: v.astype(np.float32) for k, v in qq.items()})[1].astype(np.float64)
                tol = N.TOL['float32'] * np.abs(R[np.isfinite(R)]).max()
                check(f'{kind} {shape} {where} {value}', low, R, tol, rows, at[0], absorbed=True)


@pytest.mark.parametrize('kind', ['l1', 'l2'])
def test_regulariser_cases_on_the_host(kind):
    rng = np.random.default_rng(3)
    w, g0 = (rng.standard_normal(5003).astype(np.float32).astype(np.float64) for _ in range(2))
    for where, at in N.positions(w.shape).items():
        for value in N.ALL_VALUES:
            loss, R = N.reg_reference(kind, N.put(w, at, value), g0, 2.0 ** -6)
            assert not np.isfinite(loss)
            # sign(+-Inf) is +-1: the L1 gradient of an infinite weight is finite in the oracle
            assert N.bad(R).sum() == (0 if kind == 'l1' and np.isinf(value) else 1)


@pytest.mark.parametrize('opt', N.OPTIMIZERS)
def test_optimizer_cases_on_the_host(opt):
    """NaN in g at three indices: the oracle's w is NaN exactly there, every other element equals the clean step's."""
    n = 5003
    rng = np.random.default_rng(5)
    w, g, v = (rng.standard_normal(n) for _ in range(3))
    a = rng.uniform(1e-3, 1.0, n)
    spots = list(N.opt_spots(n, 2048))
    clean = N.opt_reference(opt, w, g, v, a)
    gp = g.copy()
    gp[spots] = np.nan
    planted = N.opt_reference(opt, w, gp, v, a)
    assert np.array_equal(np.flatnonzero(np.isnan(planted[0])), spots)
    keep = np.ones(n, bool)
    keep[spots] = False
    for got, want in zip(planted, clean):
        assert np.array_equal(got[keep], want[keep])


def step_case(name, half):
    X, y = (H16 if half else H32).page_case(name, 1)
    return (O.round16(X) if half else X), y


@pytest.mark.parametrize('half', [False, True], ids=['float32', 'float16'])
@pytest.mark.parametrize('run', list(N.STEP_RUNS))
def test_one_nan_reaches_every_parameter_gradient(run, half):
    layers, hit, spared = N.STEP_RUNS[run]
    nets = H16.PAGE_NETS if half else H32.ALL_NETS
    host = H16 if half else H32
    batch = host.page_batch(1)
    planted = N.planted_batch(batch, [k for k in layers if k in batch])
    for name in nets:
        tag_x, tag_y = host.TAGS[name]
        if not half and name == 'Char' and 'char_lines' not in batch:
            continue
        net = H16.analytic_net(name)
        if run == 'weights':
            pn = N.first_weight(net.params)
            net.params[pn] = N.put(net.params[pn], (0,) * net.params[pn].ndim, N.NAN)
        X, y = planted[tag_x], planted[tag_y]
        if half:
            X = O.round16(X)
        else:
            X, y = H32.f32(X), H32.f32(y)
        with np.errstate(all='ignore'):
            pred, loss, grads = net.data_grads(X, y)
        if name in hit:
            assert np.isnan(loss), (run, name, loss)
            for pn, g in grads.items():
                assert np.isnan(g).all(), f'{run} {name} {pn}: {int((~np.isnan(g)).sum())} of {g.size} elements are not NaN'
        else:
            assert name in spared and np.isfinite(loss)
            assert all(np.isfinite(g).all() for g in grads.values()), (run, name)


def test_a_label_planted_in_one_channel_is_not_a_step_case():
    """Why labels are planted in every channel: one NaN in channel 0 of a Line label leaves the oracle's gradient of the
    last layer's weights towards channel 1 finite."""
    X, y = H32.page_case('Line', 1)
    y = N.put(y, (0, y.shape[1] // 2, y.shape[2] // 2, 0), N.NAN)
    with np.errstate(all='ignore'):
        _, loss, grads = H16.analytic_net('Line').data_grads(X, y)
    g = grads['Line/end/conv_1/w']
    assert np.isnan(loss) and np.isnan(g[..., 0]).all() and np.isfinite(g[..., 1]).all()
