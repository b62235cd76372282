"""Host checks of the elementwise bound (elementwise_bound.py) for every case of the GPU table: no GPU needed.

  * a correct implementation has room: the float32 NumPy restatement of the oracle stays at or below HALF the bound
    on every judged element.  A binary16 store alone uses its term up: round-to-nearest misses a value just above a
    power of two by 2^-11 of it, so even the float64 reference rounded once to binary16 reaches 0.99 of the
    bound wherever the kernel has no operand term (printed below as `exact, stored`).  For binary16 outputs the half therefore applies
    to what the store leaves: the unrounded float32 restatement stays within half of tol - (2^-11 |ref| + 2^-25),
    and, rounded once to binary16, within the whole bound;
  * the case tests something new: at least half of the elements have a tolerance below 1/16 of what the suite's
    rel_linf allowance (1e-5 float32, 1e-3 binary16) grants them;
  * three wrong implementations are rejected by the bound -- a constant of a tenth of the rel_linf allowance times
    max |ref| added everywhere (a leak), the residue of a 5-wide float32 sliding sum that adds the entering element
    and subtracts the leaving one, and weights rounded to binary16 judged with operand_u = 0 -- and rel_linf accepts
    the first two.  The sliding residue is 2^-24 of the largest value the sum has met, and a binary16 store hides it
    unless |ref| (with an operand term: S) is some 2^-13 of that value: the binary16 inputs therefore give the strips
    all of the exponent range the normal range leaves (elementwise_bound.fit16: 2^16 between strips), the walk starts
    at the end where the large strip lies, and the mutant is judged AFTER its store, under the full tolerance of the
    GPU test, as every other mutant is;
  * binary16: every stored input and every S lies in the normal range;
  * conv pair backward: at most 1 % of the dx pixels are left unjudged for an undecided LeakyReLU slope.

The Sigmoid cases, the Sigmoid derivative taken from a stored output and the pair's dx with every pixel judged have
tests of their own below: what their inputs must offer, the float32 restatement within the bound (its largest err /
tol is printed), and the wrong implementations each bound must reject -- a Sigmoid by tanh with a binary16 argument,
expf clamped at |v| = 16, y (1 - y) from a y rounded once more to binary16, and for the pair's dx a dropped tap at a
strip border, a flipped decided slope, d_a1 rounded twice and the mask read one row off.  Where rel_linf accepts a
mutant that the bound rejects the output says so.

The weight gradients (elementwise_wgrad.py) have theirs at the end: the case table reaches every kernel family of the
weight-gradient ladder with n <= 2048 at both pages; the float32 restatement keeps to HALF of gamma(n + 8) S on every
element of dw and db; 2^-17 of the neighbouring channel added to every element exceeds the tolerance while its rel_linf
stays below the 2e-5 the other tests allow; the binary16 inputs with their gradient scale are normal; a contested slope
of the pair dominates at most 5 % of dw1 / db1.

The binary16 pair at its kernels' own roundings (elementwise_bound.Pair16Steps) comes last: the pages reach every launch
form of both backward kernels; the float32 restatement has room, the widening dominates at most 5 % of any output, and
five mutants are rejected: the 2^-17 channel leak (inside the 2e-4 rel_linf of test_gpu_pair_forms.py), a halo column
and a band's overlap row summed twice, the wave kernel with the strip kernel's slope-and-product rule and with alpha
unrounded in d_a1.
"""
import numpy as np
import pytest

import elementwise_bound as B
import elementwise_wgrad as W
from conftest import rel_linf
from test_gpu_conv_padding import WGRAD, expect_kernel
from test_gpu_gemm_configs import expect_gemm, expect_group
from test_gpu_pair_forms import TOL_SUM16, expect_pair


def test_gamma_and_tolerance_terms():
    assert B.gamma(1) == pytest.approx(2.0 ** -24, rel=1e-6) and B.gamma(100) > 100 * 2.0 ** -24
    ref, s = np.array([2.0, -4.0]), np.array([8.0, 16.0])
    assert np.array_equal(B.tolerance(ref, s, 25), B.gamma(33) * s)
    assert np.array_equal(B.tolerance(ref, s, 25, store16=True), 2.0 ** -11 * np.abs(ref) + B.gamma(33) * s + 2.0 ** -25)
    assert np.array_equal(B.tolerance(ref, s, 25, operand16=True), (2.0 ** -11 + B.gamma(33)) * s)


def test_inputs_are_representable_and_vary_by_region():
    rng = np.random.default_rng(1)
    for dtype, store in B.STORE.items():
        x = B.scaled_input(rng, (3, 37, 141, 4), dtype)
        assert np.array_equal(x.astype(store).astype(np.float64), x) and np.all(x != 0)
        limit = sum(B.EXPONENTS[dtype].values())
        assert 0.25 * 2.0 ** -limit <= np.abs(x).min() and np.abs(x).max() <= 2.0 ** limit
        e = B.region_exponents(np.random.default_rng(2), (3, 37, 141, 4), B.EXPONENTS[dtype])
        for axis, size in ((1, B.BAND), (2, B.STRIP)):      # constant inside a band / strip, the ends of the range occur
            moved = np.moveaxis(np.broadcast_to(e, (3, 37, 141, 4)), axis, 0)
            assert all(np.array_equal(moved[i], moved[i - i % size]) for i in range(moved.shape[0]))
        assert np.ptp(e) >= limit
    assert 16 % B.BAND or 16 % B.STRIP                      # (8 divides 16: band borders on tile borders; 24 does not)
    assert all(t % B.STRIP for t in (16, 32, 64))


def test_the_table_holds_every_family():
    ids = set(B.CASE_IDS)
    assert len(ids) == len(B.CASES)
    kernels = {(c.problem.dtype, k) for c in B.CASES for k in c.kernels.values()}
    want32 = {'t32', 'tiled', 'c16_expand', 'c16_reduce', 'dgrad_s2', 'dgrad_c64s2', 'table_px', 'table_fast', 'mfma',
              'generic'}
    assert want32 <= {k for d, k in kernels if d == 'float32'}, kernels
    assert {'h16', 'table_px', 'table_fast', 'tiled', 'dgrad_s2'} <= {k for d, k in kernels if d == 'float16'}, kernels
    for i in range(len(B.TABLE)):
        assert {f'32-table{i}', f'32-table{i}-t32_0-tiled0', f'16-table{i}', f'16-table{i}-h16_0'} <= ids
    assert {'32-up4', '32-up1', '32-pair', '32-dense', '32-windows', '16-up4', '16-up1', '16-pair'} <= ids
    # the options that take the shadowing kernels away leave table kernels only
    for c in B.CASES:
        if c.id.endswith('-t32_0-tiled0'):
            assert not {'t32', 'tiled'} & set(c.kernels.values()), c
        if c.id.endswith('-h16_0'):
            assert 'h16' not in c.kernels.values() and not c.operand16, c


def test_sigmoid_tolerance_terms():
    u, k = 2.0 ** -24, B.SIGMOID_K
    v, e = np.array([0.0, -30.0, 30.0, -100.0, 3.0]), np.array([0.0, 0.0, 0.0, 0.0, 1.0])
    s = 1.0 / (1.0 + np.exp(-v))
    want = s * ((1.0 - s) * k * u + 2 * u) + 2.0 ** -126
    want[4] += 1.0 * (1.0 / (1.0 + np.exp(-2.0))) * (1.0 - 1.0 / (1.0 + np.exp(-2.0)))      # E sigma'(|v| - E)
    assert np.allclose(B.sigmoid_tolerance(v, e), want, rtol=1e-12, atol=0.0)
    assert B.sigmoid_tolerance(v, e)[3] == pytest.approx(2.0 ** -126, rel=1e-3)              # sigma(-100) = 4e-44
    assert np.allclose(B.sigmoid_tolerance(v, e, store16=True), want + 2.0 ** -11 * s + 2.0 ** -25, rtol=1e-12, atol=0.0)
    assert B.sigmoid_tolerance(np.array([0.5]), np.array([2.0]))[0] > 2.0 * 0.25                # the interval holds 0
    # the float64 Sigmoid keeps its relative accuracy on both sides
    assert B.sigmoid(np.array([-700.0]))[0] == pytest.approx(np.exp(-700.0), rel=1e-15)
    assert 1.0 - B.sigmoid(np.array([40.0]))[0] == 0.0 and B.sigmoid(np.array([-40.0]))[0] == pytest.approx(np.exp(-40.0))
    # the float32 restatement overflows where the kernels' expf does
    assert B.sigmoid(np.array([-88.73, -88.0], np.float32), np.float32)[0] == 0.0
    assert B.sigmoid(np.array([-88.73, -88.0], np.float32), np.float32)[1] > 0.0


def test_the_sigmoid_table_holds_every_family():
    ids = set(B.SIGMOID_IDS)
    assert len(ids) == len(B.SIGMOID_CASES)
    linear = {c.id for c in B.CASES if not isinstance(c.problem, B.WindowsProblem)}
    assert ids == {i + '-sigmoid' for i in linear}
    assert {'32-up4-sigmoid', '32-up1-sigmoid', '32-pair-sigmoid', '16-pair-sigmoid', '32-dense-sigmoid',
            '32-mfma-mfma2-sigmoid', '32-generic-sigmoid', '16-up4-h16_0-sigmoid'} <= ids
    by_id = {c.id: c for c in B.CASES}
    for c in B.SIGMOID_CASES:
        base = by_id[c.id[:-len('-sigmoid')]]
        assert c.opts == base.opts and c.outputs == ('y_sigmoid',) and c.problem.base is base.problem
        assert c.kernels.get('y_sigmoid') == base.kernels.get('y')
        assert bool(c.operand16) == ('y' in base.operand16)


@pytest.mark.parametrize('index', range(len(B.SIGMOID_CASES)), ids=B.SIGMOID_IDS)
def test_sigmoid_case_inputs_room_and_mutations(index):
    """The inputs offer what a test of the Sigmoid needs (SigmoidProblem.check_inputs: >= 30 % of the outputs with
    |v| <= 4, >= 5 % each with v >= 20 and v <= -20, float32: some v < -88.72, binary16: some Sigmoid below the
    subnormals, regions of order one and saturated ones); the float32 restatement 1 / (1 + exp(-v)) of the float32
    linear restatement keeps to the bound; the tanh form with a binary16 argument and expf clamped at |v| = 16 do not."""
    c = B.SIGMOID_CASES[index]
    p = c.problem
    p.check_ranges()
    info = p.check_inputs()
    name = 'y_sigmoid'
    ref, tol = p.ref[name], p.tolerances(c.operand16)[name]
    assert tol.shape == ref.shape and np.all(tol > 0) and np.all((ref >= 0) & (ref <= 1))
    room = B.worst_ratio(p.restated(store=False)[name], ref, p.tolerances(c.operand16, store=False)[name])
    stored = B.worst_ratio(p.restated()[name], ref, tol)
    allow = B.ALLOW[p.dtype]
    fine = float(np.mean(tol < allow * np.abs(ref).max() / 16))
    print(f'{c.id}: w x 2^{info["shift"]}, |v| <= 4 on {info["mid"]:.1%}, v >= 20 on {info["high"]:.1%}, v <= -20 on '
          f'{info["low"]:.1%}, v in [{info["vmin"]:.3g}, {info["vmax"]:.3g}], region medians of |v| {info["median_min"]:.2g} .. '
          f'{info["median_max"]:.2g}; restatement / tol {room:.3f} (stored {stored:.3f}), tol < allowance / 16 on {fine:.1%}')
    failures = []
    if not room <= 1.0:
        failures.append(f'the float32 restatement reaches {room:.3f} of the bound')
    if not stored <= 1.0:
        failures.append(f'the float32 restatement, stored, reaches {stored:.3f} of the bound')
    exact32 = p.v.astype(np.float32)
    for what, act in (('tanh form with a binary16 argument', B.sigmoid_by_tanh16), ('expf clamped at |v| = 16', B.sigmoid_clamped)):
        ratio = B.worst_ratio(p.restated(act=act)[name], ref, tol)
        own = act(exact32, np.float32).astype(np.float64)       # the mutant on the oracle's v: its own error alone
        lin = rel_linf(B.r16(own) if p.half else own, ref)
        print(f'    {what}: {ratio:.3g} of the bound; rel_linf of the mutant alone {lin:.1e}')
        assert ratio > 1.0, f'{c.id}: the mutation "{what}" passes the bound ({ratio:.3g})' + \
            (f' -- and rel_linf = {lin:.1e} accepts it' if lin <= allow else '')
        if lin <= allow:
            print(f'    rel_linf <= {allow:g} accepts this mutant; the bound rejects it')
    assert not failures, '\n'.join(failures)


def test_the_pair_dx_table():
    ids = set(B.PAIR_DX_IDS)
    assert len(ids) == len(B.PAIR_DX_CASES)
    seen = {(c.problem.dtype, c.problem.q['x'].shape[1:3], c.problem.pad1, c.problem.sig) for c in B.PAIR_DX_CASES}
    for sig in (False, True):
        assert ('float32', (37, 141), 0.25, sig) in seen                  # the module's float32 pair problem
        for pad1 in (0.0, 0.25):
            assert ('float16', (37, 141), pad1, sig) in seen              # the module's shape
        assert ('float16', (21, 128), 0.0, sig) in seen                   # whole waves, pad1 = 0: MODE 0 of the kernel
    assert ('float16', (19, 71), 0.25, False) in seen and 71 % 16 and 141 % 16
    assert B.r16(0.25) == 0.25


@pytest.mark.parametrize('index', range(len(B.PAIR_DX_CASES)), ids=B.PAIR_DX_IDS)
def test_pair_dx_case_widens_little_has_room_and_rejects_the_mutations(index):
    """dx of the conv pair with every pixel judged: the widened pixels (a slope the kernel may take otherwise than the
    oracle reaches them) are at most 5 % and their tolerance stays below 1/16 of the rel_linf allowance; the kernel's
    rounding points restated in float32 keep to the bound; four wrong kernels do not."""
    c = B.PAIR_DX_CASES[index]
    p = c.problem
    p.check_ranges()
    ref, tol, t = p.ref['dx'], p.tolerances()['dx'], p.parts
    assert tol.shape == ref.shape and np.all(tol > 0)
    allow = B.ALLOW[p.dtype] * np.abs(ref).max()
    widened = p.widened
    share = float(widened.mean())
    worst = float((tol[widened] / allow).max()) if widened.any() else 0.0
    fine = float(np.mean(tol < allow / 16))
    room = B.worst_ratio(p.restated(store=False)['dx'], ref, p.tolerances(store=False)['dx'])
    stored = B.worst_ratio(p.restated()['dx'], ref, tol)
    exact = B.worst_ratio(p.kernel_steps(p.q, np.float64)[3], ref, p.tolerances(store=False)['dx'])
    print(f'{c.id}: {int((~t["decided"]).sum())} undecided and {int(t["flip"].sum())} contested slopes of {t["flip"].size}, '
          f'widened pixels {share:.2%}, their largest tolerance {worst:.2g} of the rel_linf allowance; tol < allowance / 16 on '
          f'{fine:.1%}; restatement / tol {room:.3f} (stored {stored:.3f}; rounding points in exact arithmetic {exact:.3f})')
    assert share <= 0.05, f'{share:.2%} of the dx pixels widened (> 5 %)'
    assert worst < 1 / 16, f'a widened pixel has {worst:.3g} of the rel_linf allowance (>= 1/16)'
    if p.half:
        assert widened.any(), 'no contested slope: the rule is not exercised'
    assert room <= 1.0 and stored <= 1.0 and exact <= 1.0, (room, stored, exact)
    failures = []
    for what, mutate in B.pair_dx_mutants(p).items():
        got = p.restated(mutate=mutate)['dx']
        ratio, lin = B.worst_ratio(got, ref, tol), rel_linf(got, ref)
        accepted = lin <= B.ALLOW[p.dtype]
        print(f'    {what}: {ratio:.3g} of the bound, rel_linf {lin:.1e}' +
              (f' <= {B.ALLOW[p.dtype]:g}: rel_linf accepts this mutant, the bound rejects it' if accepted else ''))
        if not ratio > 1.0:
            failures.append(f'{what} passes the bound ({ratio:.3g})' + (f' -- and rel_linf = {lin:.1e} accepts it' if accepted else ''))
    assert not failures, '\n'.join(failures)


def test_the_from_output_table():
    ids = set(B.FROM_OUTPUT_IDS)
    assert len(ids) == len(B.FROM_OUTPUT_CASES)
    vec = {}
    for c in B.FROM_OUTPUT_CASES:
        p = c.problem
        if p.kind != 'act':
            vec.setdefault((p.dtype, p.kind, p.shape[3]), set()).add(p.check_inputs())
    for dtype in B.STORE:
        assert f'{dtype[5:]}-act-37x141x1' in ids
        for kind in ('dice', 'jaccard'):
            # 16 | hw c elem on one shape and not on the other, where the element size leaves the choice (c elem < 16)
            assert vec[dtype, kind, 1] == vec[dtype, kind, 2] == {True, False}
            assert vec[dtype, kind, 4] == ({True} if dtype == 'float32' else {True, False})
            assert vec[dtype, kind, 3] == {False}


@pytest.mark.parametrize('index', range(len(B.FROM_OUTPUT_CASES)), ids=B.FROM_OUTPUT_IDS)
def test_from_output_case_has_room_and_rejects_the_mutation(index):
    """y (1 - y) of a stored y: the float32 restatement keeps to 3 u |ref| (+ the coefficient terms of seg_loss); the
    same from a y rounded once more to binary16 does not, and rel_linf accepts it."""
    c = B.FROM_OUTPUT_CASES[index]
    p = c.problem
    p.check_inputs()
    ref, tol = p.ref['dx'], p.tolerances()['dx']
    assert tol.shape == ref.shape and np.all(tol > 0)
    zero = (p.q['y'] == 0) | (p.q['y'] == 1)
    assert zero.any() and np.all(ref[zero] == 0) and np.all(ref[~zero] != 0)
    room = B.worst_ratio(p.restated(store=False)['dx'], ref, p.tolerances(store=False)['dx'])
    stored = B.worst_ratio(p.restated()['dx'], ref, tol)
    mutant = p.mutated()
    ratio, lin, allow = B.worst_ratio(mutant, ref, tol), rel_linf(mutant, ref), B.ALLOW[p.dtype]
    print(f'{c.id}: restatement / tol {room:.3f} (stored {stored:.3f}); y rounded to binary16: {ratio:.3g} of the bound, '
          f'rel_linf {lin:.1e}' + (f' <= {allow:g}: rel_linf accepts this mutant, the bound rejects it' if lin <= allow else ''))
    assert room <= 1.0 and stored <= 1.0, (room, stored)
    assert ratio > 1.0, f'{c.id}: y (1 - y) from a binary16 y passes the bound ({ratio:.3g})' + \
        (f' -- and rel_linf = {lin:.1e} accepts it' if lin <= allow else '')


@pytest.mark.parametrize('index', range(len(B.CASES)), ids=B.CASE_IDS)
def test_case_has_room_is_new_and_rejects_the_mutations(index):
    c = B.CASES[index]
    p = c.problem
    p.check_ranges()
    tols, strict = p.tolerances(c.operand16), p.tolerances(())
    low, unstored, rounded = p.restated(), p.restated(store=False), p.with_rounded_weights()
    allow = B.ALLOW[p.dtype]
    failures = []
    for name in c.outputs:
        ref, tol, judged = p.ref[name], tols[name], p.judged(name)
        assert tol.shape == ref.shape and np.all(tol > 0)
        unjudged = 1.0 - judged.mean()
        room = B.worst_ratio(unstored[name], ref, tol - p.store_part(name), judged)
        stored = B.worst_ratio(low[name], ref, tol, judged)
        exact = B.worst_ratio(B.r16(ref), ref, tol, judged) if p.half else 0.0
        fine = float(np.mean(tol < allow * np.abs(ref).max() / 16))
        leak = B.constant_leak(low[name], ref, p.dtype)
        slide = unstored[name] + B.sliding_residue(unstored[name], B.sliding_axis(p, name))
        if p.half:                              # the drift is on the float32 value; the test sees what the store keeps
            slide = B.r16(slide)
        r_leak, r_slide = (B.worst_ratio(a, ref, tol, judged) for a in (leak, slide))
        r_w16 = B.worst_ratio(rounded[name], ref, strict[name], judged)
        l_leak, l_slide = rel_linf(leak, ref), rel_linf(slide, ref)
        print(f'{c.id} {name}: restatement / tol {room:.3f} (stored {stored:.3f}; exact, stored {exact:.3f}), tol < allowance / 16 on {fine:.1%}, unjudged {unjudged:.2%}; '
              f'leak {r_leak:.3g} (rel_linf {l_leak:.1e}), sliding {r_slide:.3g} (rel_linf {l_slide:.1e}), '
              f'binary16 weights {r_w16:.3g}')
        if not room <= 0.5:
            failures.append(f'{name}: the float32 restatement reaches {room:.3f} of the bound (> 0.5)')
        if not stored <= 1.0:
            failures.append(f'{name}: the float32 restatement, stored, reaches {stored:.3f} of the bound (> 1)')
        if not fine >= 0.5:
            failures.append(f'{name}: only {fine:.1%} of the tolerances lie below 1/16 of the rel_linf allowance')
        if not unjudged <= 0.01:
            failures.append(f'{name}: {unjudged:.2%} of the pixels unjudged (> 1 %)')
        for what, ratio in (('constant leak', r_leak), ('sliding sum', r_slide), ('binary16 weights', r_w16)):
            if not ratio > 1.0:
                failures.append(f'{name}: the {what} mutation passes the bound ({ratio:.3g})')
        for what, err in (('constant leak', l_leak), ('sliding sum', l_slide)):
            if not err <= allow:
                failures.append(f'{name}: rel_linf rejects the {what} mutation too ({err:.2e}): nothing new shown')
    assert not failures, '\n'.join(failures)


# ---- weight gradients (elementwise_wgrad.py) ------------------------------------------------------------------------------
def test_the_weight_gradient_table():
    """Every kernel family of the weight-gradient ladder runs; every case sums at most 2048 terms; each configuration has
    the w % 4 == 0 page and the ragged one."""
    ids = set(W.WCASE_IDS)
    assert len(ids) == len(W.WCASES)
    seen = {c.kernel[1] for c in W.WCASES if c.kernel is not None and c.kernel[0] == WGRAD}
    want = {'table_fast', 'c16_wgrad', 'wgrad_t542', 'wgrad_s2_tiled', 'h16_wgrad', 'h16_wgrad_s2', 'mfma', 'generic'}
    assert want <= seen, sorted(want - seen)
    for c in W.WCASES:
        p = c.problem
        assert p.terms() <= W.MAX_TERMS, (c.id, p.terms())
        if isinstance(p, W.ConvWgradProblem):
            assert c.kernel == (WGRAD, expect_kernel(WGRAD, p.dtype, p.d, p.pad_value, c.opts)), c.id
    assert W.SHAPES[0][2] % 4 == 0 and W.SHAPES[1][2] % 4 != 0 and W.SHAPES[1][2] > 2 * 64 and W.SHAPES[1][2] % 64
    # bands of four output rows: whole ones and, at stride 2, a short last one; short last ones at either stride
    assert W.SHAPES[0][0] > 1 and W.SHAPES[0][1] % 4 == 0 and (W.SHAPES[0][1] // 2) % 4 and W.SHAPES[1][1] % 4
    assert all(2 * a[2] == b[2] or 2 * a[2] == b[2] + 1 for a, b in zip(W.LOW_SHAPES, W.SHAPES))
    pages = {}
    for c in W.WCASES:
        p = c.problem
        if isinstance(p, (W.ConvWgradProblem, W.UpWgradProblem, W.PairWgradProblem)):
            key = c.id.replace(p.name, type(p).__name__ + p.name.split('-')[0])
            pages.setdefault(key, set()).add(p.q['x'].shape[:3])
    assert all(len(v) == 2 for v in pages.values()), pages
    for i in range(len(B.TABLE)):
        for shape in W.SHAPES:
            tag = f'{shape[0]}x{shape[1]}x{shape[2]}'
            assert {f'32-table{i}-{tag}-dw', f'32-table{i}-{tag}-dw-t32_0-tiled0', f'16-table{i}-{tag}-dw',
                    f'16-table{i}-{tag}-dw-h16_0'} <= ids
    assert {'32-mfma-3x20x32-dw-mfma2', '32-generic-1x13x141-dw', '32-up4-3x10x16-dw', '16-up1-1x6x71-dw', '32-dense-dw',
            '32-dense-dw-mfma2', f'32-dense{W.SLAB_ROWS}-dw', '32-windows-dw', '32-pair-3x20x32-dw',
            '32-pair-1x13x141-dw-sigmoid'} <= ids
    # the dense case that must split its depth: two or more slabs under the host rule, alone and as two of a group
    (c,) = [c for c in W.WCASES if c.gemm is not None]
    assert 1000 <= c.gemm[2] <= 2040 and c.problem.rows == c.gemm[2]
    for cu in (64, 256, 304):
        assert expect_gemm(*c.gemm, True, cu, 128 << 20, c.opts)[3] >= 2
        assert min(expect_group([c.gemm] * 2, cu, 128 << 20, 0, c.opts['split_blocks'], c.opts['split_min'])) >= 2


def test_weight_gradient_tolerance_terms():
    p = W.wproblem('table', 'float32', 7, 0)
    s, n = p.sums['dw']
    assert n == 3 * 20 * 32 and np.array_equal(p.tolerances()['dw'], B.gamma(n + 8) * s)
    acc = p.tolerances(True)['dw']
    assert np.array_equal(acc, B.gamma(n + 8) * s + 2.0 ** -24 * np.abs(p.init['dw'] + p.ref['dw']))
    r = p.init['dw'] / p.ref['dw']
    assert np.all((np.abs(r) > 0.2499) & (np.abs(r) < 1.0001)) and (r > 0).any() and (r < 0).any()
    assert np.array_equal(p.init['dw'].astype(np.float32).astype(np.float64), p.init['dw'])
    off = W.wproblem('table', 'float32', 0, 0)                      # no bias: ref 0, tolerance 0, only the exact value passes
    assert not off.bias and np.all(off.ref['db'] == 0) and np.all(off.tolerances()['db'] == 0) and np.all(off.init['db'] != 0)
    assert W.ratio(np.zeros(16), off.ref['db'], off.tolerances()['db']).max() == 0
    assert W.ratio(np.full(16, 1e-30), off.ref['db'], off.tolerances()['db']).max() == np.inf
    assert W.ratio(np.full(16, np.nan), off.ref['db'], off.tolerances()['db']).max() == np.inf


@pytest.mark.parametrize('index', range(len(W.WCASES)), ids=W.WCASE_IDS)
def test_weight_gradient_case_has_room_and_rejects_the_leak(index):
    """Room: the float32 NumPy restatement (the pair: through the kernel's rounding points) stays within HALF of the
    tolerance on every element of every output.  The leak mutant: 2^-17 of the neighbouring channel's value added to every
    element of dw (db) exceeds the tolerance somewhere, and rel_linf < 2e-5 accepts it.  binary16: x and 2^k dy lie in the
    normal range, k > 0.  The pair: a contested slope dominates the tolerance of at most 5 % of dw1 / db1."""
    c = W.WCASES[index]
    p = c.problem
    p.check_ranges()
    tols, acc, low = p.tolerances(), p.tolerances(True), p.restated()
    leaks, asserted = W.leak_ratios(p), W.leak_asserted(p)
    failures = []
    for name in p.outputs:
        ref, tol = p.ref[name], tols[name]
        assert tol.shape == ref.shape == acc[name].shape and np.all(tol >= 0) and np.all(acc[name] > 0)
        assert np.all((tol > 0) | (ref == 0))
        room = float(W.ratio(low[name], ref, tol).max())
        with np.errstate(divide='ignore', invalid='ignore'):
            loose = float(np.nanmax(np.where(ref != 0, tol / np.abs(ref), 0.0)))
        line = f'{c.id} {name}: n = {p.terms()}, k = {p.gscale}, restatement / tol {room:.4f}, largest tol / |ref| {loose:.3g}'
        if not room <= 0.5:
            failures.append(f'{name}: the float32 restatement reaches {room:.3f} of the bound (> 0.5)')
        if name in leaks:
            lin = rel_linf(p.leaked(name), ref)
            line += f'; leak {leaks[name]:.3g} of the bound, rel_linf {lin:.2e}' + ('' if name in asserted else ' (not asserted)')
            if name in asserted and not leaks[name] > 1.0:
                failures.append(f'{name}: the leak mutant passes the bound ({leaks[name]:.3g})')
            if not lin < W.ALLOW_W:
                failures.append(f'{name}: rel_linf rejects the leak mutant too ({lin:.2e}): nothing new shown')
        else:
            line += '; no leak mutant (a single channel, or a switched-off bias)'
        if isinstance(p, W.PairWgradProblem) and name in ('dw1', 'db1'):
            share = p.widened_share(name)
            line += f'; widening above the arithmetic part on {share:.2%}, contested slopes {int(p.dx.parts["flip"].sum())}'
            if not share <= W.WIDEN_CAP:
                failures.append(f'{name}: a contested slope dominates {share:.2%} of the elements (> 5 %)')
        print(line)
    multi = any(p.leak_axis(k) is not None for k in p.outputs)
    assert bool(asserted) == multi, (c.id, asserted)     # every case with a neighbouring channel has an asserted mutant
    assert not failures, '\n'.join(failures)


# ---- the binary16 pair at its own roundings (elementwise_bound.Pair16Steps) -------------------------------------------------
HOST_CU = 256                                   # compute units the launch rules are evaluated with here


def test_the_binary16_pair_table():
    """The pages are the smallest at which each launch form of the two binary16 backward kernels still runs: the
    cooperative kernel (4) at several images, a ragged width with and without a padding value (MODE 1) and two whole
    waves at pad1 0 (MODE 0); the wave kernel (5) at 600 columns -- ten strips, three blocks with two live strips in the
    last, a ragged last strip -- at 560 -- nine strips, the last ends on the page -- and at three images of one row; at
    three rows pair_band 2 gives two bands, the second with one row.  Every page sums at most 2048 terms."""
    assert len(set(W.PAIR16_IDS)) == len(W.PAIR16_KEYS) == 2 * len(W.PAIR16_PAGES)
    pages = {(k, s, pad) for k, s, pad in W.PAIR16_PAGES}
    assert {('strip', (3, 20, 32), 0.25), ('strip', (1, 13, 141), 0.0), ('strip', (1, 13, 141), 0.25), ('strip', (2, 8, 128), 0.0),
            ('wave', (1, 3, 600), 0.0), ('wave', (1, 3, 600), 0.25), ('wave', (1, 3, 560), 0.0), ('wave', (3, 1, 560), 0.25)} == pages
    for kernel, (n, h, w), pad1 in W.PAIR16_PAGES:
        assert n * h * w <= W.MAX_TERMS
        for g in (4, 2):
            form, det = expect_pair('bwd', 'float16', n, h, w, pad1, {'pair_g': g}, HOST_CU)
            assert form[0] == (5 if kernel == 'wave' else 4), (kernel, w, form)
            assert form[1] == (g if kernel == 'wave' else 4)
            if kernel == 'strip':
                assert form[2] == (0 if (w, pad1) == (128, 0.0) else 1), (w, pad1, form)
    assert expect_pair('bwd', 'float16', 1, 3, 600, 0.0, {}, HOST_CU)[1] == dict(nstrips=10, last_live=2, last_band=3)
    assert expect_pair('bwd', 'float16', 1, 3, 560, 0.0, {}, HOST_CU)[1]['nstrips'] == 9 and 8 * 62 + 64 == 560 < 9 * 62 + 64
    assert 9 * 62 + 64 > 600                                                 # the tenth strip is ragged
    form, det = expect_pair('bwd', 'float16', 1, 3, 600, 0.0, {'pair_band': 2}, HOST_CU)
    assert form[6:] == (2, 2) and det['last_band'] == 1
    assert expect_pair('bwd', 'float16', 3, 20, 32, 0.25, {'pair_band': 2}, HOST_CU)[0][6] > 1
    assert {(s, pad) for s, pad, _ in B.PAIR_WAVE_DX_KEYS} == {((2, 11, 600), 0.25), ((1, 3, 560), 0.0)}
    assert expect_pair('bwd', 'float16', 2, 11, 600, 0.25, {}, HOST_CU)[0][0] == 5
    assert B.A16 != B.A32 and abs(B.A16 / B.ALPHA - 1) < 2.0 ** -11 and B.r16(0.25) == 0.25


def test_the_two_kernels_rounding_rules():
    """The restated activation of either kernel on hand-picked values: the wave kernel rounds first and reads the sign bit
    (a z that rounds to -0 takes alpha), multiplies by alpha16; the strip kernel compares the float32 z with 0 (-0 takes
    1), multiplies by the float32 alpha and rounds once.  An interval's endpoints enclose its nominal value."""
    z = np.array([-1e-9, 1e-9, -0.0, -1.0, 3.0, -1.0 - 2.0 ** -12])
    s = np.array([2.0, 2.0, 2.0, 1.0 + 2.0 ** -10, 5.0, 1.0 + 2.0 ** -10 + 2.0 ** -13])
    a, neg = B.pair16_leaky('wave', z, np.float64)
    assert list(neg) == [True, False, True, True, False, True] and a[0] == 0 and a[3] == -B.A16 and a[4] == 3.0
    d = B.pair16_masked('wave', s, neg, np.float64)
    assert d[0] == B.r16(2.0 * B.A16) and d[1] == 2.0 and d[3] == B.r16((1.0 + 2.0 ** -10) * B.A16)
    assert d[5] == d[3] and a[5] == a[3]                              # rounded FIRST: the bits below binary16 are gone
    a, neg = B.pair16_leaky('strip', z, np.float64)
    assert list(neg) == [True, False, False, True, False, True] and a[3] == B.r16(-B.A32) and a[5] == B.r16((-1.0 - 2.0 ** -12) * B.A32)
    d = B.pair16_masked('strip', s, neg, np.float64)
    assert d[2] == 2.0 and d[5] == B.r16(s[5] * B.A32) and d[3] == B.r16(s[3] * B.A32)
    assert B.r16(B.A16) == B.A16 and B.r16(B.A32) == B.A16 and B.A32 != B.ALPHA
    t = B.Interval(np.array([1.0, -3.0]), np.array([1.5, -2.0]), np.array([2.0, 1.0]))
    assert list(t.width) == [1.0, 4.0] and list(t.mag) == [2.0, 3.0]


def _judge_pair16(st, outputs, what):
    """room, caps and mutants of one Pair16Steps over `outputs`; returns the failures"""
    st.check_ranges()
    assert st.gscale > 0
    sh = st.shares()
    print(f'{what}: seed {st.base.seed}, k = {st.gscale}, n = {st.terms}; contested a1 {sh["a1"]:.2%}, d_a1 {sh["d_a1"]:.2%}, '
          f'g {sh["g"]:.2%}, slopes {sh["slopes"]:.2%}')
    failures = []
    low, unstored = st.restated(), st.restated(store=False)
    for name in outputs:
        ref, (arith, widen) = st.ref[name], st.parts[name]
        tol = st.tolerances()[name]
        assert tol.shape == ref.shape and np.all(tol >= 0) and np.all((tol > 0) | (ref == 0))
        if name == 'dx':
            arith = arith + B.U16 * np.abs(ref) + B.FLOOR16      # the store is part of what every pixel is allowed
            plain, room = st.room(unstored[name], name, store=True)
            stored = st.room(low[name], name, store=True)[0]
        else:
            plain, room = st.room(low[name], name)
            stored = plain
        share = st.widened_share(name)
        with np.errstate(divide='ignore', invalid='ignore'):
            rel = np.where(ref != 0, tol / np.abs(ref), np.nan)
            most = float(np.nanmax(np.where(arith > 0, widen / arith, 0.0)))
        print(f'    {name}: restatement / tol {plain:.4f} (beyond the widening {room:.4f}; stored {stored:.3f}), widening above the '
              f'arithmetic part on {share:.2%} (largest widening / arithmetic {most:.2f}), median tol / |ref| {np.nanmedian(rel):.1e}')
        if name != 'dx' and not plain <= 0.5:
            failures.append(f'{name}: the float32 restatement reaches {plain:.3f} of the bound (> 0.5)')
        if not room <= 0.5:
            failures.append(f'{name}: beyond its widening the float32 restatement reaches {room:.3f} of the bound (> 0.5)')
        if not stored <= 1.0:
            failures.append(f'{name}: the float32 restatement, stored, reaches {stored:.3f} of the bound (> 1)')
        if not share <= W.WIDEN_CAP:
            failures.append(f'{name}: the widening exceeds the arithmetic part on {share:.2%} of the elements (> 5 %)')
    mutants = (('halo', 'row') if 'dw1' in outputs else ()) + (B.WAVE_RULE_MUTANTS if st.kernel == 'wave' else ())
    for m in mutants:
        if m == 'row' and st.overlap_row() is None:
            print('    row: the page has one row, no band overlaps another')
            continue
        r = {k: v for k, v in B.pair16_mutant_ratios(st, m).items() if k in outputs or k == 'dx'}
        print(f'    {m}: ' + ', '.join(f'{k} {v:.3g}' for k, v in r.items()) + ' of the bound')
        if not max(r.values()) > 1.0:
            failures.append(f'the mutant "{m}" passes the bound ({max(r.values()):.3g})')
    return failures


@pytest.mark.parametrize('index', range(len(W.PAIR16_KEYS)), ids=W.PAIR16_IDS)
def test_binary16_pair_case_has_room_and_rejects_the_mutants(index):
    """dw1, db1, dw2, db2 (and the dx of the same launch) of the binary16 pair at the kernel's own roundings, shapes (3,
    20, 32), (1, 13, 141), (2, 8, 128) for the cooperative kernel and (1, 3, 600), (1, 3, 560), (3, 1, 560) for the wave
    kernel: the float32 restatement stays within room <= 0.5 of the tolerance; the elements whose widening exceeds the
    arithmetic part stay within WIDEN_CAP (5 %); k > 0 and every rounded quantity is in range.  Mutants: the 2^-17
    neighbouring-channel leak reaches VISIBLE tolerances on dw1 and dw2 while its rel_linf stays inside the 2e-4 that
    test_gpu_pair_forms.py allows (the gap this closes; db1 is printed, no seed shows it reliably); one halo column summed
    twice into all four outputs; the overlap row between two bands summed twice; and for the wave kernel its restatement
    fed the strip kernel's slope-and-product rule, and alpha unrounded in d_a1 -- these two show on dx (elementwise_bound,
    "Seeds", says why no weight gradient can show them)."""
    p = W.pair16_problem(*W.PAIR16_KEYS[index])
    assert '16-' + p.name == W.PAIR16_IDS[index] and p.terms() <= W.MAX_TERMS
    failures = _judge_pair16(p.steps, p.outputs + ('dx',), W.PAIR16_IDS[index])
    low = p.restated()
    acc = p.tolerances(True)
    leaks = W.leak_ratios(p)
    assert set(leaks) == {'dw1', 'db1', 'dw2'} and W.leak_asserted(p) == ('dw1', 'dw2')
    for name in p.outputs:
        assert np.array_equal(low[name], p.steps.restated()[name]) and np.all(acc[name] >= p.tolerances()[name])
        if name in leaks:
            lin = rel_linf(p.leaked(name), p.ref[name])
            print(f'    leak {name}: {leaks[name]:.3g} of the bound, rel_linf {lin:.2e}' + ('' if name != 'db1' else ' (not asserted)'))
            if name != 'db1' and not leaks[name] >= W.VISIBLE:
                failures.append(f'{name}: the leak mutant reaches {leaks[name]:.3g} tolerances (< {W.VISIBLE})')
            if not lin < TOL_SUM16:
                failures.append(f'{name}: rel_linf rejects the leak mutant too ({lin:.2e}): nothing new shown')
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('index', range(len(B.PAIR_WAVE_DX_KEYS)), ids=B.PAIR_WAVE_DX_IDS)
def test_pair_wave_dx_case_has_room_and_rejects_the_mutants(index):
    """dx of pair_wave_bwd_h_kernel at (2, 11, 600) and (1, 3, 560), every pixel judged at the kernel's own roundings:
    beyond what its contested roundings explain the float32 restatement uses at most half of the tolerance, stored it
    keeps to the whole; at most 5 % of the pixels have a widening above their arithmetic and store terms; the strip
    kernel's slope-and-product rule and an unrounded alpha each exceed the tolerance."""
    c = B.pair_wave_dx_case(index)
    failures = _judge_pair16(c.problem.steps, ('dx',), c.id)
    p = c.problem
    assert np.array_equal(p.ref['dx'], p.steps.ref['dx']) and np.array_equal(p.tolerances()['dx'], p.steps.tolerances()['dx'])
    assert p.device('g').max() <= B.F16_MAX and np.array_equal(p.device('g'), p.q['g'] * 2.0 ** p.gscale)
    assert not failures, '\n'.join(failures)
