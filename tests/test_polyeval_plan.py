"""hehub_amd/polyeval.py: the plan builder on the CPU.  Plan.evaluate_plain interprets a plan on exact rationals (the roundings of the
rescales ignored), so what it returns differs from p(x) only by the constants the builder rounded to integers, and is held to
numpy's polyval / chebval:

    |evaluate_plain(x) - p(x)| <= 64 * (number of rounded constants) / Delta

Each rounding moves a constant of size about Delta |c| by at most 1/2, and the recurrence can amplify that; a wrong scale anywhere
gives an error of 2^-20 or more and fails by orders of magnitude.  The measured worst case over everything below is printed by
test_worst_case_over_all_cases (DESIGN 4.7j records it).  Then the structure: the output scale is the target scale as a Fraction, the
limb count follows the documented formula, every reference points backwards at an element with enough limbs, and `switches` counts
the steps with a product."""
import math
from fractions import Fraction

import numpy as np
import pytest
from numpy.polynomial import chebyshev as Ch

import params as P
from hehub_amd.polyeval import BASES, build_plan, leaf_coefficients

DELTA = 1 << 40
L = 9
Q = P.P40[:L]
XS = (1.0, -1.0, 0.0, 0.73, -0.73, 0.001)
SHAPES = ((2, 2), (4, 2), (4, 4), (8, 4))


def coefficients(seed, degree, odd=False):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, degree + 1)
    if odd:
        c[0::2] = 0.0
    return [float(v) for v in c]


def reference(coefs, basis, x):
    return float(np.polyval(coefs[::-1], x)) if basis == "power" else float(Ch.chebval(x, coefs))


def cases():
    for basis in BASES:
        for n1, n2 in SHAPES:
            yield basis, n1, n1 * n2 - 1, False     # every leaf full
        yield basis, 4, 5, False                    # the last leaf is not filled
        yield basis, 4, 15, True                    # an odd polynomial: half the terms absent
        yield basis, 4, 3, False                    # n2 == 1: a single leaf step


CASES = list(cases())


def plan_of(basis, n1, degree, odd):
    coefs = coefficients(1000 + 10 * degree + n1 + (5 if odd else 0), degree, odd)
    return coefs, build_plan(coefs, basis, Q, DELTA, DELTA, n1=n1)


def worst_error(coefs, basis, plan):
    return max(abs(plan.evaluate_plain(x) - reference(coefs, basis, x)) for x in XS)


@pytest.mark.parametrize("basis,n1,degree,odd", CASES)
def test_evaluate_plain_matches_numpy(basis, n1, degree, odd):
    coefs, plan = plan_of(basis, n1, degree, odd)
    err, bound = worst_error(coefs, basis, plan), 64 * plan.rounded_constants / DELTA
    print(f"{basis} n1 {n1} degree {degree}: error {err:.3e}, bound {bound:.3e}, {plan.rounded_constants} rounded constants, "
          f"largest {plan.largest_constant_bits} bits")
    assert plan.rounded_constants > 0 and err <= bound


def test_worst_case_over_all_cases():
    worst = max(worst_error(c, b, p) for b, n1, d, o in CASES for c, p in [plan_of(b, n1, d, o)])
    print(f"worst |evaluate_plain - p| over {len(CASES)} plans and {len(XS)} points: {worst:.3e}")
    assert worst < 2.0 ** -30


@pytest.mark.parametrize("basis,n1,degree,odd", CASES)
def test_structure(basis, n1, degree, odd):
    _, plan = plan_of(basis, n1, degree, odd)
    n2 = degree // n1 + 1
    clog2 = lambda v: 0 if v <= 1 else math.ceil(math.log2(v))
    used = clog2(n1 - 1) + 1 if n2 == 1 else 1 + max(clog2(n1 - 1) + 1, clog2(n1 * (n2 - 1)))
    assert plan.in_limbs == L and plan.out_limbs == L - used
    assert isinstance(plan.out_scale, Fraction) and plan.out_scale == Fraction(DELTA)
    assert plan.switches == sum(1 for s in plan.steps if s.products)
    limbs = [L]
    for idx, s in enumerate(plan.steps):
        assert 2 <= s.level <= L
        forms = [f for xy in s.products for f in xy] + [s.z]
        for f in forms:
            for e, c in f.terms:
                assert 0 <= e <= idx and limbs[e] >= s.level      # backwards, and at a level the operand still has
                assert c is None or isinstance(c, int)
            assert f.cst is None or isinstance(f.cst, int)
        assert all(f.terms for xy in s.products for f in xy)
        assert s.products or s.z.terms
        limbs.append(s.level - 1)
    assert limbs == plan.limbs
    last = plan.steps[-1]
    if n2 > 1:   # the flat recombination: every product in ONE step, every other switch is a power
        assert all(len(s.products) <= 1 for s in plan.steps[:-1])
        assert len(last.products) == sum(1 for s in plan.steps[:-1] if not s.products)   # one per leaf step


def test_zero_coefficients_and_unused_powers_cost_nothing():
    """x^8 + x (n1 = 4): leaf_2 is the constant 1 -- a term of Z, no leaf step --, leaf_1 is empty, B_3 is never needed"""
    coefs = [0.0, 1.0] + [0.0] * 6 + [1.0]
    plan = build_plan(coefs, "power", Q, DELTA, DELTA, n1=4)
    assert [len(s.products) for s in plan.steps] == [1, 1, 1, 0]   # B_2, B_4, B_8, then the sum: no product left
    assert plan.switches == 3 and abs(plan.evaluate_plain(0.73) - (0.73 ** 8 + 0.73)) < 1e-9


def test_chebyshev_leaves_are_exact():
    """sum_g leaf_g T_{g n1} expanded back with T_i T_m = (T_{m+i} + T_{|m-i|}) / 2 gives the coefficients, as Fractions"""
    c = [Fraction(v) for v in coefficients(7, 15)]
    a = leaf_coefficients(c, "chebyshev", 4)
    back = [Fraction(0)] * 16
    for g, row in enumerate(a):
        for i, v in enumerate(row):
            if g == 0 or i == 0:
                back[g * 4 + i] += v
            else:
                back[g * 4 + i] += v / 2
                back[g * 4 - i] += v / 2
    assert back == c


def test_refusals():
    with pytest.raises(ValueError):
        build_plan([1.0, 2.0], "legendre", Q, DELTA, DELTA)
    with pytest.raises(ValueError):
        build_plan([1.0] * 8, "power", Q, DELTA, DELTA, n1=3)
    with pytest.raises(ValueError):
        build_plan([1.0] * 32, "power", Q[:3], DELTA, DELTA, n1=8)   # not enough moduli
    with pytest.raises(ValueError):
        build_plan([0.0, 0.0], "power", Q, DELTA, DELTA)
