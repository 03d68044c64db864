"""Plans for hp_dev_ckks_eval_plan_hks (include/hehub_amd.h): a polynomial in the power or the Chebyshev basis as a straight-line
program of steps  E_{s+1} = rescale(relin(sum_t X_t (x) Y_t) + Z)  over linear forms with integer constants.

The engine is exact integer arithmetic; what a ciphertext's integers MEAN -- its scale -- is tracked here, as fractions.Fraction,
and every constant the plan hands the engine is an integer rounded once from an exact rational.  No float arithmetic decides an
integer: a given coefficient becomes Fraction(float), exactly, and everything after that is rational.

Shape (baby-step giant-step, flat recombination), with B_j = x^j or T_j(x), n1 a power of two and n2 = deg // n1 + 1:
  babies   B_2 .. B_{n1-1} and B_{n1}; B_j = B_a B_b (power) or 2 T_a T_b - T_{a-b} (Chebyshev), j = a + b split at its top power
           of two (a = b = j / 2 for a power of two), so B_j sits ceil(log2 j) levels below the input;
  giants   G_g = B_{g n1}, g < n2, by the same rule (their indices stay multiples of n1);
  leaves   p = sum_g leaf_g(x) G_g with leaf_g in B_0 .. B_{n1-1}; each leaf_g, g >= 1, is its own step WITHOUT a product (a linear
           form, rescaled) at the babies' level l* = L - ceil(log2(n1 - 1)), at the scale target q_{lf-1} / S(G_g) -- lf the level
           of the final step -- so that every product of the final step has the scale target q_{lf-1} exactly;
  final    ONE step holding all the products leaf_g (x) G_g, g >= 1 -- one key switch -- with leaf_0 as its Z form.
The output scale is target_scale exactly; the levels consumed are 1 + max(ceil(log2(n1 - 1)) + 1, ceil(log2(n1 (n2 - 1)))) for
n2 >= 2, and ceil(log2(n1 - 1)) + 1 for the single leaf step of n2 == 1.  Zero coefficients produce no term; a leaf without a term
and a power nobody uses are not computed.

Chebyshev coefficients are split by T_i T_{g n1} = (T_{g n1 + i} + T_{g n1 - i}) / 2: the products have distinct top degrees, so the
system is triangular -- from the top coefficient down, leaf coefficient 2 c with c subtracted at index g n1 - i (no factor for i = 0
or g = 0).  In the recurrence the subtrahend is kappa T_{a-b} with kappa = round(S_a S_b / S_{a-b}), about one modulus: the scales
are matched BEFORE the rescale, where the integers are large enough for a relative 2^-40.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from fractions import Fraction
from typing import List, Optional, Sequence, Tuple

from . import capi

BASES = ("power", "chebyshev")


@dataclass
class Form:
    """sum_j coef_j * E_{elem_j} + cst: coef an integer (None: 1), cst an integer (None: 0)"""
    terms: List[Tuple[int, Optional[int]]] = field(default_factory=list)
    cst: Optional[int] = None


@dataclass
class Step:
    level: int
    products: List[Tuple[Form, Form]]
    z: Form


def _round(v: Fraction) -> int:
    """nearest integer, halves away from zero (exact)"""
    n, d = v.numerator, v.denominator
    return (2 * n + d) // (2 * d) if n >= 0 else -((-2 * n + d) // (2 * d))


def _clog2(v: int) -> int:
    return 0 if v <= 1 else (v - 1).bit_length()


def _split(j: int) -> Tuple[int, int]:
    top = 1 << (j.bit_length() - 1)
    return (j // 2, j // 2) if top == j else (top, j - top)


def leaf_coefficients(coefs: Sequence[Fraction], basis: str, n1: int):
    """a[g][i]: p = sum_g (sum_{i < n1} a[g][i] B_i) B_{g n1}, exactly"""
    d = len(coefs) - 1
    n2 = d // n1 + 1
    a = [[Fraction(0)] * n1 for _ in range(n2)]
    w = list(coefs)
    for kk in range(d, -1, -1):
        g, i = divmod(kk, n1)
        if basis == "power" or g == 0 or i == 0:
            a[g][i] = w[kk]
        else:
            a[g][i] = 2 * w[kk]
            w[g * n1 - i] -= w[kk]
    return a


class Plan:
    """.steps, .in_limbs, .out_limbs, .out_scale, .switches (steps with a key switch), .final_drops (0), .rounded_constants (how
    many constants were rounded from a rational), .largest_constant_bits; evaluate_plain(x); marshal() for the C call"""

    def __init__(self, moduli, input_scale):
        self.moduli = [int(q) for q in moduli]
        self.in_limbs = len(self.moduli)
        self.steps: List[Step] = []
        self.limbs = [self.in_limbs]            # per element
        self.scales = [Fraction(input_scale)]   # per element
        self.final_drops = 0
        self.rounded_constants = 0
        self.largest_constant_bits = 0

    # -- building ------------------------------------------------------------------------------------------------------------------
    def constant(self, v: Fraction) -> int:
        c = _round(v)
        self.rounded_constants += 1
        self.largest_constant_bits = max(self.largest_constant_bits, abs(c).bit_length())
        return c

    def add(self, level: int, products, z: Form, scale: Fraction) -> int:
        """appends a step; scale: of (sum of products + Z) BEFORE the rescale.  Returns the new element's index."""
        for f in [f for xy in products for f in xy] + [z]:
            assert all(0 <= e < len(self.limbs) and self.limbs[e] >= level for e, _ in f.terms)
        assert 2 <= level <= self.in_limbs
        self.steps.append(Step(level, list(products), z))
        self.limbs.append(level - 1)
        self.scales.append(Fraction(scale) / self.moduli[level - 1])
        return len(self.limbs) - 1

    @property
    def out_limbs(self) -> int:
        return self.limbs[-1] - self.final_drops

    @property
    def out_scale(self) -> Fraction:
        return self.scales[-1]

    @property
    def switches(self) -> int:
        return sum(1 for s in self.steps if s.products)

    # -- the plan on exact rationals, roundings of the rescales ignored -------------------------------------------------------------
    def evaluate_plain(self, x) -> float:
        val = [Fraction(x) * self.scales[0]]   # every element as value * scale

        def form(f: Form) -> Fraction:
            return sum((val[e] * (1 if c is None else c) for e, c in f.terms), Fraction(0 if f.cst is None else f.cst))

        for s in self.steps:
            acc = form(s.z)
            for fx, fy in s.products:
                acc += form(fx) * form(fy)
            val.append(acc / self.moduli[s.level - 1])
        return float(val[-1] / self.out_scale)

    # -- the C structs ---------------------------------------------------------------------------------------------------------------
    def marshal(self):
        """(array of capi.EvalStep, what must stay alive while it is used)"""
        keep = []

        def residues(c: Optional[int], level: int):
            if c is None:
                return None
            arr = (capi.u64 * level)(*[c % q for q in self.moduli[:level]])
            keep.append(arr)
            return C.cast(arr, C.POINTER(capi.u64))

        def form(f: Form, level: int) -> capi.EvalForm:
            out = capi.EvalForm()
            out.terms = len(f.terms)
            if f.terms:
                terms = (capi.EvalTerm * len(f.terms))()
                for t, (e, c) in zip(terms, f.terms):
                    t.elem = e
                    r = residues(c, level)
                    if r is not None:
                        t.coef = r
                keep.append(terms)
                out.term = C.cast(terms, C.POINTER(capi.EvalTerm))
            r = residues(f.cst, level)
            if r is not None:
                out.cst = r
            return out

        steps = (capi.EvalStep * len(self.steps))()
        for dst, s in zip(steps, self.steps):
            dst.level = s.level
            dst.products = len(s.products)
            if s.products:
                xs = (capi.EvalForm * len(s.products))(*[form(fx, s.level) for fx, _ in s.products])
                ys = (capi.EvalForm * len(s.products))(*[form(fy, s.level) for _, fy in s.products])
                keep += [xs, ys]
                dst.x = C.cast(xs, C.POINTER(capi.EvalForm))
                dst.y = C.cast(ys, C.POINTER(capi.EvalForm))
            dst.z = form(s.z, s.level)
        return steps, keep


def build_plan(coefs, basis: str, moduli, input_scale, target_scale, n1: Optional[int] = None) -> Plan:
    """coefs[j]: the coefficient of x^j (basis "power") or T_j (basis "chebyshev", x in [-1, 1]) as floats (taken exactly) or
    Fractions; moduli: q_0 .. q_{L-1} of the input ciphertext; input_scale, target_scale: exact (int or Fraction)."""
    if basis not in BASES:
        raise ValueError(f"basis must be one of {BASES}")
    c = [Fraction(v) for v in coefs]
    while len(c) > 1 and c[-1] == 0:
        c.pop()
    if len(c) < 2:
        raise ValueError("a constant polynomial needs no plan")
    d = len(c) - 1
    if n1 is None:
        n1 = 2
        while n1 * n1 < d + 1:
            n1 *= 2
    if n1 < 2 or n1 & (n1 - 1):
        raise ValueError("n1 must be a power of two, at least 2")
    n2 = d // n1 + 1
    L = len(moduli)
    target = Fraction(target_scale)
    plan = Plan(moduli, input_scale)
    q = plan.moduli
    a = leaf_coefficients(c, basis, n1)
    cheb = basis == "chebyshev"
    l_star = L - _clog2(n1 - 1)                                                            # the babies' level
    lf = l_star if n2 == 1 else L - max(_clog2(n1 - 1) + 1, _clog2(n1 * (n2 - 1)))         # the last step's
    if lf < 2:
        raise ValueError("not enough moduli for this polynomial")

    # which powers are computed: the babies the leaves use, the giants with a leaf, and what those are made of
    need = set()

    def want(j):
        if j <= 1 or j in need:
            return
        need.add(j)
        ja, jb = _split(j)
        want(ja), want(jb)
        if cheb:
            want(ja - jb)

    for g in range(n2):
        used = [i for i in range(1, n1) if a[g][i] != 0]
        for i in used:
            want(i)
        if g >= 1 and (used or a[g][0] != 0):
            want(g * n1)

    elem = {1: 0}   # power index -> element
    for j in sorted(need):
        ja, jb = _split(j)
        ea, eb = elem[ja], elem[jb]
        level = min(plan.limbs[ea], plan.limbs[eb])
        s2 = plan.scales[ea] * plan.scales[eb]
        if not cheb:
            elem[j] = plan.add(level, [(Form([(ea, None)]), Form([(eb, None)]))], Form(), s2)
        else:
            z = Form()
            if ja == jb:
                z.cst = -plan.constant(s2)                                                 # T_0 = 1 at the products' scale
            else:
                z.terms.append((elem[ja - jb], -plan.constant(s2 / plan.scales[elem[ja - jb]])))   # kappa
            elem[j] = plan.add(level, [(Form([(ea, 2)]), Form([(eb, None)]))], z, s2)

    def leaf(g: int, scale: Fraction) -> Form:
        """leaf_g as a linear form at `scale` (before a rescale)"""
        f = Form()
        for i in range(1, n1):
            if a[g][i] != 0:
                f.terms.append((elem[i], plan.constant(a[g][i] * scale / plan.scales[elem[i]])))
        if a[g][0] != 0:
            f.cst = plan.constant(a[g][0] * scale)
        return f

    if n2 == 1:
        plan.add(l_star, [], leaf(0, target * q[l_star - 1]), target * q[l_star - 1])
        return plan
    top = target * q[lf - 1]   # the scale of everything the final step sums
    products, z = [], None
    extra = []                 # leaves that are a constant alone: c * G_g, a term of Z
    for g in range(1, n2):
        if all(v == 0 for v in a[g]):
            continue
        eg = elem[g * n1]
        if all(a[g][i] == 0 for i in range(1, n1)):
            extra.append((eg, plan.constant(a[g][0] * top / plan.scales[eg])))
            continue
        sigma = top / plan.scales[eg]
        e_leaf = plan.add(l_star, [], leaf(g, sigma * q[l_star - 1]), sigma * q[l_star - 1])
        products.append((Form([(e_leaf, None)]), Form([(eg, None)])))
    z = leaf(0, top)
    z.terms += extra
    plan.add(lf, products, z, top)
    assert plan.out_scale == target
    return plan
