"""CKKS bootstrapping as a plan over the engine's calls: ModRaise -> CoeffToSlot -> EvalMod -> SlotToCoeff.

The engine is exact integer arithmetic; what a ciphertext's integers MEAN -- its scale -- is tracked here as fractions.Fraction, as
in hehub_amd/polyeval.py, and every integer the plan hands the engine (a diagonal's coefficients, a constant of EvalMod) is rounded
once from a float or a rational.  Full packing only: n = N / 2 slots.

Slots.  With zeta = exp(2 pi i / 2N), slot j of a polynomial t is t(zeta^(G^j)) with G = 3: the engine's cycle(step) is hehub's, the
automorphism of the Galois generator 3, so with THIS numbering cycle(step) is the plain rotation out[j] = in[j - step] for every
step (tests/test_bootstrap_plan.py pins it).  With the customary 5^j numbering only the even steps are rotations -- an odd power of 3
is minus a power of 5, a rotation composed with the conjugation, which no single entry of the hybrid calls expresses.  encode /
decode are host-only (the engine has no encoder).

Matrices are dicts {rotation r: complex vector d of length n} meaning y[j] = sum_r d_r[j] x[(j + r) mod n]; the product follows
(A B)_{r+s}[j] += A_r[j] B_s[(j + r) mod n].  No dense n x n array is built above n = 64 (dense() is for the tests).

The special FFT.  E0[j][k] = zeta^(G^j k), k < n; E0 = S_n ... S_4 S_2 R with R the bit reversal and S_len the
radix-2 stage on blocks of len slots,
    y[i + j] = x[i + j] + a_j x[i + j + len/2],   y[i + j + len/2] = x[i + j] + b_j x[i + j + len/2],     j < len/2,
    a_j = exp(2 pi i G^j / 4 len),  b_j = exp(2 pi i G^(j + len/2) / 4 len)        (b_j = -a_j from len = 4 on),
three diagonals (0, +-len/2) each.  A real polynomial t = t_lo + X^n t_hi has slots E0 t_lo + i Sigma E0 t_hi, Sigma = diag((-1)^j)
(zeta^(G^j n) = i^(3^j)); Sigma commutes with every stage but S_2.  R is dropped on both sides: EvalMod is slot-wise, so the
coefficients sit in the slots in bit-reversed order between CoeffToSlot and SlotToCoeff and the permutation cancels.

  CoeffToSlot  u = (1 / 2n) S^H w through `factors` matrices (groups of stages, the adjoints in reverse order), each ONE
               hp_dev_ckks_lintrans_bsgs_hks_at + hp_dev_ckks_rescale.  The LAST factor runs twice, with its diagonals A and
               A (-i Sigma): the two halves as one batch of 2 B.  t_lo = u + conj(u) (and t_hi alike) takes ONE
               hp_dev_ckks_conjugate_hks_at on that batch and one hp_dev_ckks_lincomb -- the conjugation does not go through
               baby_conj, where an entry is a conjugation OR a rotation.
  EvalMod      ONE hp_dev_ckks_eval_plan_hks on the batch of 2 B: the Chebyshev plan of cos(2 pi (K x - 1/4) / 2^r) on [-1, 1]
               (polyeval.build_plan), x = t / (K q_0), then r double-angle steps 2 E (x) E - 1 (Plan.add): sin(2 pi t / q_0),
               which is 2 pi m / q_0 up to the cube of that for t = m + q_0 I.
  SlotToCoeff  w = S (y_lo + i Sigma y_hi): the FIRST factor runs on both halves (diagonals G_1 and i Sigma G_1), summed by
               hp_dev_ckks_lincomb before the one rescale; the other factors as above.
The normalisations -- 1 / (2n), 1 / (K q_0) (the raised ciphertext is simply READ at the scale K q_0), q_0 / (2 pi Delta) -- are
folded into the diagonals, spread evenly over the factors of their side; no level is spent on them.

Out of scope: sparse packing / SubSum; a single C entry for the pipeline (a C caller chains the same calls); the node, sharded and
C++ host layers; a device encoder; sparse-secret encapsulation; the arcsine correction; iterated bootstrapping; hoisting across
factors."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from fractions import Fraction
from typing import Dict, List, Optional, Tuple

import numpy as np

from .polyeval import Form, Plan, build_plan

GEN = 3   # the Galois generator of the engine's cycle(step) (hehub's), and so of the slot numbering

Matrix = Dict[int, np.ndarray]


# ---- encoder (host only) ---------------------------------------------------------------------------------------------------------------
def slot_exponents(N: int) -> List[int]:
    return [pow(GEN, j, 2 * N) for j in range(N // 2)]


_ROOTS: Dict[int, np.ndarray] = {}


def _roots(N: int) -> np.ndarray:
    """F[j][k] = zeta^(G^j k), [n][N] (kept per N: 32 MiB at N = 2048; the encoder is a host tool for tests and small rings)"""
    if N not in _ROOTS:
        _ROOTS[N] = _roots_build(N)
    return _ROOTS[N]


def _roots_build(N: int) -> np.ndarray:
    e = np.array(slot_exponents(N), dtype=np.int64)[:, None] * np.arange(N, dtype=np.int64)[None, :] % (2 * N)
    return np.exp(2j * np.pi * e / (2 * N))


def encode(z, scale, N: int) -> List[int]:
    """n = N / 2 complex slot values -> the N integer coefficients of the real polynomial t with t(zeta^(G^j)) ~ scale * z[j]:
    t = (1/n) Re(F^H (scale z)), each coefficient rounded once"""
    z = np.asarray(z, dtype=np.complex128)
    assert z.shape == (N // 2,)
    t = (np.conj(_roots(N)).T @ (z * float(scale))).real / (N // 2)
    return [int(v) for v in np.rint(t)]


def decode(t, scale, N: int) -> np.ndarray:
    """integer coefficients -> slot values t(zeta^(G^j)) / scale"""
    return _roots(N) @ np.array([float(v) for v in t]) / float(scale)


# ---- matrices in diagonal form ---------------------------------------------------------------------------------------------------------
def mat_mul(A: Matrix, B: Matrix, n: int) -> Matrix:
    out: Matrix = {}
    for r, a in A.items():
        for s, b in B.items():
            k = (r + s) % n
            out[k] = out.get(k, 0) + a * np.roll(b, -r)
    return {r: d for r, d in out.items() if np.any(d != 0)}


def mat_adjoint(A: Matrix, n: int) -> Matrix:
    return {(-r) % n: np.conj(np.roll(d, r)) for r, d in A.items()}


def mat_scale(A: Matrix, c) -> Matrix:
    return {r: d * c for r, d in A.items()}


def mat_right_diag(A: Matrix, v: np.ndarray) -> Matrix:
    """A diag(v)"""
    return {r: d * np.roll(v, -r) for r, d in A.items()}


def mat_apply(A: Matrix, x: np.ndarray) -> np.ndarray:
    return sum(d * np.roll(x, -r) for r, d in A.items())


def dense(A: Matrix, n: int) -> np.ndarray:
    assert n <= 64
    M = np.zeros((n, n), dtype=np.complex128)
    for r, d in A.items():
        for j in range(n):
            M[j, (j + r) % n] += d[j]
    return M


def stage(n: int, ln: int) -> Matrix:
    """S_len of the head comment"""
    h, M = ln // 2, 4 * ln
    a = np.zeros(n, dtype=np.complex128)
    b = np.zeros(n, dtype=np.complex128)
    one_lo = np.zeros(n)
    for i in range(0, n, ln):
        for j in range(h):
            a[i + j] = np.exp(2j * np.pi * pow(GEN, j, M) / M)
            b[i + j + h] = np.exp(2j * np.pi * pow(GEN, j + h, M) / M)
            one_lo[i + j] = 1
    out: Matrix = {0: one_lo + b}
    for r, d in ((h % n, a), ((-h) % n, 1 - one_lo)):
        out[r] = out.get(r, 0) + d
    return out


def bit_reverse(n: int) -> np.ndarray:
    bits = n.bit_length() - 1
    return np.array([int(format(j, f"0{bits}b")[::-1], 2) if bits else 0 for j in range(n)])


def sigma(n: int) -> np.ndarray:
    return np.array([(-1.0) ** j for j in range(n)])


def stc_factors(n: int, factors: int) -> List[Matrix]:
    """S = G_f ... G_1 as `factors` matrices in the order they are applied (G_1 holds S_2), the stages split as evenly as possible"""
    stages = [stage(n, 2 << s) for s in range(n.bit_length() - 1)]
    assert 1 <= factors <= len(stages)
    base, extra = divmod(len(stages), factors)
    out, at = [], 0
    for f in range(factors):
        cnt = base + (1 if f < extra else 0)
        G = stages[at]
        for s in stages[at + 1:at + cnt]:
            G = mat_mul(s, G, n)
        out.append(G)
        at += cnt
    return out


def cts_factors(n: int, factors: int) -> List[Matrix]:
    """S^H = G_1^H ... G_f^H in the order they are applied (G_f^H first; the last one holds S_2^H)"""
    return [mat_adjoint(G, n) for G in reversed(stc_factors(n, factors))]


# ---- baby-step giant-step split -------------------------------------------------------------------------------------------------------
@dataclass
class Bsgs:
    """rotations r = g + i (signed, mod n) over the babies i and giants g that occur; diags[g][i] = rot_g^-1(diag_{g+i}) or None"""
    babies: List[int]
    giants: List[int]
    diags: List[List[Optional[np.ndarray]]]


def bsgs_split(A: Matrix, n: int) -> Bsgs:
    signed = {(r if r < n // 2 else r - n): d for r, d in A.items()}
    st = 0
    for r in signed:
        st = math.gcd(st, abs(r))
    st = st or 1
    idx = sorted(r // st for r in signed)
    span = idx[-1] - idx[0] + 1
    b1 = 1
    while b1 * b1 < span:
        b1 *= 2
    babies = sorted({(v % b1) * st for v in idx})
    giants = sorted({(v - v % b1) * st for v in idx})
    diags = [[None] * len(babies) for _ in giants]
    for r, d in signed.items():
        v = r // st
        i, g = (v % b1) * st, (v - v % b1) * st
        diags[giants.index(g)][babies.index(i)] = np.roll(d, g)
    return Bsgs(babies, giants, diags)


def bsgs_apply(s: Bsgs, x: np.ndarray) -> np.ndarray:
    """the float twin of hp_dev_ckks_lintrans_bsgs_hks: sum_g rot_g(sum_i diag_{g,i} rot_i(x))"""
    out = 0
    for g, row in zip(s.giants, s.diags):
        inner = sum(d * np.roll(x, -i) for i, d in zip(s.babies, row) if d is not None)
        out = out + np.roll(inner, -g)
    return out


def step_of(r: int, n: int) -> int:
    """the engine's cycle step of the rotation y[j] = x[j + r]"""
    return (-r) % n


# ---- EvalMod --------------------------------------------------------------------------------------------------------------------------
def cheb_coefficients(f, degree: int) -> List[float]:
    """Chebyshev interpolation of f on [-1, 1] at the degree + 1 Chebyshev nodes"""
    m = degree + 1
    theta = np.pi * (np.arange(m) + 0.5) / m
    y = f(np.cos(theta))
    c = [2.0 / m * float(np.sum(y * np.cos(j * theta))) for j in range(m)]
    c[0] /= 2
    return c


def cheb_eval(c, x):
    return np.polynomial.chebyshev.chebval(x, c)


def chebyshev_levels(degree: int) -> int:
    """the levels polyeval.build_plan spends on a Chebyshev polynomial of this degree (its default n1)"""
    n1 = 2
    while n1 * n1 < degree + 1:
        n1 *= 2
    n2 = degree // n1 + 1
    clog2 = lambda v: 0 if v <= 1 else (v - 1).bit_length()
    return clog2(n1 - 1) + 1 if n2 == 1 else 1 + max(clog2(n1 - 1) + 1, clog2(n1 * (n2 - 1)))


def evalmod_parameters(K: int, precision_bits: int) -> Tuple[int, int]:
    """(degree, r) for the scaled cosine cos(2 pi (K x - 1/4) / 2^r) on [-1, 1] followed by r double-angle steps: each step costs a
    level and multiplies an error by at most 4.  For every r in 0 .. 6 the smallest degree whose interpolation error, times 4^r, stays
    below 2^-precision_bits; of those the pair with the fewest levels, then the smallest degree (the fewest key switches)"""
    xs = np.linspace(-1, 1, 4001)
    best = None
    for r in range(0, 7):
        f = lambda x: np.cos(2 * np.pi * (K * x - 0.25) / (1 << r))
        for degree in range(3, 128):
            err = float(np.max(np.abs(cheb_eval(cheb_coefficients(f, degree), xs) - f(xs))))
            if err * 4 ** r < 2.0 ** -precision_bits:
                cost = (chebyshev_levels(degree) + r, degree)
                if best is None or cost < best[0]:
                    best = (cost, degree, r)
                break
    if best is None:
        raise ValueError("no scaled-cosine approximation reaches this precision")
    return best[1], best[2]


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
@dataclass
class MatrixCall:
    """one hp_dev_ckks_lintrans_bsgs_hks_at: its split, and the diagonals as integer polynomials (N coefficients each, or None)"""
    split: Bsgs
    polys: List[List[Optional[List[int]]]]
    half: Optional[int] = None    # SlotToCoeff's first factor: the half of the batch this call reads (None: the whole batch)

    def marshal(self, n: int):
        """the call's host arguments: (baby_steps, giant_steps, identity flags of both -- a step-0 entry takes no key --, and the
        diagonals [giants][babies] as integer polynomials or None), the steps as the engine's cycle counts them"""
        return ([step_of(r, n) for r in self.split.babies], [step_of(r, n) for r in self.split.giants],
                [r % n == 0 for r in self.split.babies], [r % n == 0 for r in self.split.giants], self.polys)


@dataclass
class MatrixStage:
    side: str                     # "cts" or "stc"
    level: int                    # limbs of the input; the output has level - 1
    in_scale: Fraction
    diag_scale: Fraction
    out_scale: Fraction
    matrices: List[Matrix]        # the float matrices (normalisation folded in), one per call
    calls: List[MatrixCall] = field(default_factory=list)


class BootstrapPlan:
    """.stages (CoeffToSlot), .evalmod (a polyeval.Plan), .stages_out (SlotToCoeff); .rotations_needed as (step, conj) pairs for
    hp_dev_hks_keygen_rot*; .levels, .in_limbs, .out_limbs, the exact .out_scale; evaluate_plain(z), a float simulation of the same
    matrices and the same polynomial; upload(engine) / run(engine, d_ct, keys)."""

    def __init__(self, logn: int, moduli_ext, k: int, delta, K: int, factors: int = 2, precision_bits: int = 20, work_scale=None,
                 delta_out=None):
        self.logn, self.N, self.n, self.k = logn, 1 << logn, 1 << (logn - 1), k
        self.mext = [int(q) for q in moduli_ext]
        self.q = self.mext[:-k]
        self.in_limbs = self.key_L0 = L = len(self.q)
        self.K, self.factors = int(K), factors
        self.delta = Fraction(delta)
        self.delta_out = Fraction(delta if delta_out is None else delta_out)
        q0, n = self.q[0], self.n
        W = Fraction(work_scale) if work_scale is not None else Fraction(1 << (self.q[1].bit_length() if self.q[1] & (self.q[1] - 1) else self.q[1].bit_length() - 1))
        self.work_scale = W
        self.rounded_constants = 0
        scale, level = Fraction(self.K * q0), L
        self.in_scale = scale
        # CoeffToSlot
        self.stages: List[MatrixStage] = []
        c = (1.0 / (2 * n)) ** (1.0 / factors)
        mats = cts_factors(n, factors)
        for j, A in enumerate(mats):
            A = mat_scale(A, c)
            both = [A, mat_right_diag(A, -1j * sigma(n))] if j == factors - 1 else [A]
            scale, level = self._matrix_stage(self.stages, "cts", level, scale, W, both)
        # EvalMod
        self.degree, self.r = evalmod_parameters(self.K, precision_bits)
        self.cheb = cheb_coefficients(self._cosine, self.degree)
        if level < 2:
            raise ValueError("not enough moduli for CoeffToSlot")
        plan = build_plan(self.cheb, "chebyshev", self.q[:level], scale, W)
        for _ in range(self.r):
            e = len(plan.limbs) - 1
            s2 = plan.scales[e] * plan.scales[e]
            if plan.limbs[e] < 2:
                raise ValueError("not enough moduli for EvalMod")
            plan.add(plan.limbs[e], [(Form([(e, 2)]), Form([(e, None)]))], Form(cst=-plan.constant(s2)), s2)
        self.evalmod: Plan = plan
        self.evalmod_level = level
        scale, level = plan.out_scale, plan.out_limbs
        # SlotToCoeff
        self.stages_out: List[MatrixStage] = []
        c2 = (q0 / (2 * math.pi * float(self.delta))) ** (1.0 / factors)
        for j, G in enumerate(stc_factors(n, factors)):
            G = mat_scale(G, c2)
            both = [G, {r: 1j * sigma(n) * d for r, d in G.items()}] if j == 0 else [G]
            target = self.delta_out if j == factors - 1 else W
            scale, level = self._matrix_stage(self.stages_out, "stc", level, scale, target, both)
            if j == 0:
                for h, call in enumerate(self.stages_out[-1].calls):
                    call.half = h
        self.out_limbs, self.out_scale = level, scale
        self.levels = L - level
        if level < 1:
            raise ValueError("not enough moduli for this bootstrap")

    def _cosine(self, x):
        return np.cos(2 * np.pi * (self.K * x - 0.25) / (1 << self.r))

    def _matrix_stage(self, where, side, level, scale, target, matrices):
        if level < 2:
            raise ValueError("not enough moduli for the matrix stages")
        D = Fraction(target) * self.q[level - 1] / scale
        st = MatrixStage(side, level, scale, D, Fraction(target), matrices)
        for M in matrices:
            sp = bsgs_split(M, self.n)
            if len(sp.babies) > 32 or len(sp.giants) > 32 or len(sp.babies) * len(sp.giants) > 256:
                raise ValueError("a factor has more diagonals than one baby-step giant-step call takes: use more factors")
            polys = [[None if d is None else self._diagonal(d, D) for d in row] for row in sp.diags]
            st.calls.append(MatrixCall(sp, polys))
        where.append(st)
        return Fraction(target), level - 1

    def _diagonal(self, d, D):
        self.rounded_constants += self.N
        return encode(d, D.numerator / D.denominator, self.N)

    # -- what a caller has to generate ---------------------------------------------------------------------------------------------------
    @property
    def all_stages(self) -> List[MatrixStage]:
        return self.stages + self.stages_out

    @property
    def rotations_needed(self) -> List[Tuple[int, bool]]:
        steps = set()
        for st in self.all_stages:
            for call in st.calls:
                steps |= {step_of(r, self.n) for r in call.split.babies + call.split.giants if r % self.n}
        return [(s, False) for s in sorted(steps)] + [(0, True)]

    def level_chain(self, level: int) -> List[int]:
        return self.q[:level] + self.mext[self.key_L0:]

    # -- a float simulation: the same matrices through the same split, the same Chebyshev coefficients and double angles -----------------
    def evaluate_plain(self, z, I=None) -> np.ndarray:
        m = encode(z, self.delta, self.N)
        t = np.array([float(v) for v in m]) + (0 if I is None else float(self.q[0]) * np.asarray(I, dtype=np.float64))
        x = decode(t, self.in_scale, self.N)
        for st in self.stages[:-1]:
            x = bsgs_apply(st.calls[0].split, x)
        u = [bsgs_apply(call.split, x) for call in self.stages[-1].calls]
        halves = [2 * v.real for v in u]                                  # u + conj(u)
        y = []
        for v in halves:
            e = cheb_eval(self.cheb, v)
            for _ in range(self.r):
                e = 2 * e * e - 1
            y.append(e)
        first = self.stages_out[0].calls
        x = bsgs_apply(first[0].split, y[0].astype(np.complex128)) + bsgs_apply(first[1].split, y[1].astype(np.complex128))
        for st in self.stages_out[1:]:
            x = bsgs_apply(st.calls[0].split, x)
        return x

    # -- the device ---------------------------------------------------------------------------------------------------------------------
    def upload(self, eng):
        """the diagonals as device tensors [key_L0 + k][N], canonical NTT words over the top chain: {id(call): [[tensor or None]]}"""
        import torch

        out = {}
        for st in self.all_stages:
            for call in st.calls:
                flat = [p for row in call.polys for p in row if p is not None]
                coeffs = torch.tensor(np.array(flat, dtype=np.int64), device=f"cuda:{eng.device}")
                rows = eng.poly_reduce_strict_(self.mext, eng.poly_from_signed(self.mext, coeffs))
                it = iter(range(len(flat)))
                out[id(call)] = [[None if p is None else rows[next(it)] for p in row] for row in call.polys]
        return out

    def _bsgs(self, eng, level, call, diags, x, keys):
        bs, gs, b_id, g_id, _ = call.marshal(self.n)
        rot = keys["rot"]
        bk = [None if same else rot[s] for s, same in zip(bs, b_id)]
        gk = [None if same else rot[s] for s, same in zip(gs, g_id)]
        return eng.ckks_lintrans_bsgs_hks(self.level_chain(level), self.k, keys["alpha"], x, bk, bs, gk, gs, diags[id(call)],
                                          key_L0=self.key_L0)

    def run(self, eng, d_ct, keys, diags=None, trace=None):
        """d_ct [B][2][in][N] at its last limb (row 0 is read) -> [B][2][out_limbs][N] at out_scale.  keys: {"alpha": alpha, "rot":
        {step: hybrid key}, "conj": key, "relin": key}, device tensors generated for key_L0 = in_limbs moduli; diags: upload()'s.
        trace: a list that receives (name, device tensor) after every call"""
        import torch

        diags = self.upload(eng) if diags is None else diags
        alpha, B = keys["alpha"], d_ct.shape[0]
        note = (lambda name, t: trace.append((name, t))) if trace is not None else (lambda name, t: None)
        x = eng.ckks_mod_raise(self.q, d_ct)
        note("raise", x)
        for j, st in enumerate(self.stages):
            outs = [self._bsgs(eng, st.level, call, diags, x, keys) for call in st.calls]
            x = outs[0] if len(outs) == 1 else torch.cat(outs).contiguous()
            note(f"cts{j}", x)
            x = eng.ckks_rescale(self.q[:st.level], x)
            note(f"cts{j}_rescaled", x)
        lvl = self.evalmod_level
        xb = eng.ckks_conjugate_hks(self.level_chain(lvl), self.k, alpha, x, keys["conj"], key_L0=self.key_L0)
        note("conj", xb)
        x = eng.ckks_lincomb(self.q[:lvl], [x, xb])
        note("real", x)
        x = eng.ckks_poly_eval_hks(self.level_chain(lvl), self.k, alpha, x, keys["relin"], self.evalmod, key_L0=self.key_L0)
        note("evalmod", x)
        for j, st in enumerate(self.stages_out):
            if j == 0:
                halves = [x[:B].contiguous(), x[B:].contiguous()]
                outs = [self._bsgs(eng, st.level, call, diags, halves[call.half], keys) for call in st.calls]
                x = eng.ckks_lincomb(self.q[:st.level], outs)
            else:
                x = self._bsgs(eng, st.level, st.calls[0], diags, x, keys)
            note(f"stc{j}", x)
            x = eng.ckks_rescale(self.q[:st.level], x)
            note(f"stc{j}_rescaled", x)
        return x
