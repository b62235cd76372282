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
"""
import numpy as np
import pytest

import elementwise_bound as B
from conftest import rel_linf


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
