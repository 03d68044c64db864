"""Shapes, moduli and inputs that carry the BFV calls (hp_bfv.hip: k_bfv_lift<K>, k_bfv_scale<K>, k_bfv_decrypt_round<K>) to every Garner
width, to rows of more than one chunk and to moduli of unequal width.  bfv_model.GPU_SHAPES runs the widths 1..5 and 8 (and 16 with
nine moduli); here are 5, 6, 7 (compiled with the fences, like 8) and the guarded width 16 with 9, 10, 12, 13 and 16 moduli.

No test, no fixture: tests/test_bfv_edges.py holds every condition of these tables on the CPU (primes, the base-size rule, no fold
wrap, the planted classes, the coverage of the widths); tests/test_gpu_bfv_widths.py runs them on the device."""
from typing import NamedTuple

import numpy as np

import hks_model as H
import moduli as MD
import params as P

U = np.uint64
BATCH = 2
T0, M31 = 65537, 2147483647

P40W = P.ntt_primes(32, 5, 40)             # the width shapes: 40-bit primes = 1 (mod 64), ring degrees 16 and 32
P50W = P.ntt_primes(16, 5, 50)
P36W = P.ntt_primes(16, 5, 36)
P59 = P.ntt_primes(16, 15, 59)             # = 1 (mod 2^16); P59[0] = moduli.Q59
P20, P30 = P.ntt_primes(2, 4, 20), P.ntt_primes(2, 4, 30)   # just below 2^20 and 2^30


class Shape(NamedTuple):
    """one (Q, B) of lift, scale_round and mult_low_level, and the plain moduli it runs with"""
    name: str
    logn: int
    q: list
    b: list
    ts: tuple

    @property
    def L(self):
        return len(self.q)

    @property
    def M(self):
        return len(self.b)

    @property
    def n(self):
        return 1 << self.logn

    @property
    def qb(self):
        return list(self.q) + list(self.b)

    def __str__(self):
        return self.name


def _width(name, logn, L, M, ts):
    return Shape(name, logn, P40W[:L], P40W[L:L + M], ts)


# k_bfv_scale / k_bfv_decrypt_round run at width L; k_bfv_lift at L (Q -> B) and at M (B -> Q)
WIDTH_SHAPES = [
    _width("w5", 4, 5, 6, (T0, 1 << 19, M31)),
    _width("w6", 4, 6, 7, (T0, 2)),
    _width("w7", 4, 7, 8, (T0, M31)),
    _width("w9", 4, 9, 10, (T0,)),
    _width("w12", 4, 12, 13, (T0, 2)),
    # the guarded width full on both sides; L + M = 32 is the engine's limit.  logn 5: lift_planted plants 5 + 2 M = 37 values
    Shape("w16", 5, P40W[:16], P50W, (T0, min(P40W[:16] + P50W) - 1)),
    # 59-bit digits composed into 36-bit moduli (the scaling's way back) and 36-bit digits into 59-bit moduli (the lift)
    Shape("w16x59", 5, P36W, P59, (T0, min(P36W + P59) - 1)),
]
MIX_SHAPES = [
    Shape("b59", 4, P.P40[:3], P59[:3], (T0, min(P.P40[:3]) - 1)),
    Shape("q59", 4, P59[:3], P59[3:7], (T0, M31)),
    # B exceeds 4 t N Q by less than one bit at t = 65537: close to the base-size rule
    Shape("w59q", 4, [MD.Q59] + P.P40[:5], MD.PACKEDGE[1:7], (2, T0)),
    # 20-, 30- and 59-bit moduli in one base, every one just below its power of two (no "above" prime of moduli.NARROW: hehub's fold
    # wraps for them); B = every limb 2^k + small
    Shape("narrow", 4, P20 + P30 + [MD.Q59], list(MD.ABOVE), (T0, 1 << 19, min(P20) - 1)),
]
# rows of two chunks (ELEM_CHUNK = 2048 words) in a batch of two: row > 0 and chunk > 0 together; the tiled transforms, so level A too
CHUNK_SHAPES = [Shape("chunks12", 12, P.P40[:2], P.P40[2:5], (T0,))]
SHAPES = WIDTH_SHAPES + MIX_SHAPES + CHUNK_SHAPES
MULT_SHAPES = [s for s in SHAPES if s.name in ("w5", "w6", "w7", "w12", "w16", "q59")]


class DecryptSet(NamedTuple):
    """one Q of decrypt_round alone (no transform: any odd pairwise coprime moduli, any n)"""
    name: str
    n: int
    q: list
    ts: tuple
    prime: bool = True

    def __str__(self):
        return self.name


DECRYPT_SETS = (
    [DecryptSet("p59-L%d" % L, 16, P59[:L], (2, T0, 1 << 58, min(P59[:L]) - 1)) for L in range(1, 17)]
    + [DecryptSet("narrow-chain", 16, list(MD.NARROW), (2, 1 << 19, min(MD.NARROW) - 1)),
       # the widest digit first: bfv_digit reduces a 59-bit digit into the 20- and 30-bit moduli (in `narrow` it comes last)
       DecryptSet("wide-first", 16, [MD.Q59] + P20 + P30, (2, 1 << 19, min(P20) - 1)),
       DecryptSet("not-prime", 16, [15, 77, 221], (2, 4), prime=False),   # 3 * 5, 7 * 11, 13 * 17
       DecryptSet("chunks4", 8192, P.P40[:2], (T0,))]                     # rows of four chunks
    + [DecryptSet("Q-of-" + s.name, s.n, list(s.q), s.ts) for s in SHAPES])

# end to end on the device (logn, L, M, k, alpha): a width of the fenced family, special primes of neither base
HYBRID = (4, 6, 7, 2, 3)
HYBRID_MEXT, HYBRID_AUX, HYBRID_T = P40W[:6] + P50W[:2], P40W[6:13], T0


# ---- the widths the tables reach, computed from them ----------------------------------------------------------------------------------
def scale_widths():
    return {s.L for s in SHAPES}


def decrypt_widths():
    return {len(d.q) for d in DECRYPT_SETS}


def lift_widths():
    """cnt of k_bfv_lift: L for Q -> B (lift, scale_round's input side is k_bfv_scale), M for B -> Q (scale_round)"""
    return {s.L for s in SHAPES} | {s.M for s in SHAPES}


# ---- the Garner step's strict reduction ----------------------------------------------------------------------------------------------
def barrett_lazy(x, q):
    """hp_barrett_lazy with the engine's c = floor((2^64 - 1) / q): below 2q, not always below q"""
    return x - q * ((x * (((1 << 64) - 1) // q)) >> 64)


def digit_wrap_values(q):
    """Integers of [0, Q) at which bfv_digit needs the strict reduction of v_b mod x_A (b = 0, A = 1): the residue modulo q_0 leaves
    q_1 + s after the lazy Barrett reduction modulo q_1, and the residue modulo q_1 is below s, so that u + q_1 - v_b would be negative
    in word arithmetic without it.  Uniform values practically never get there (s is small against q_1); [] where q_0 is too narrow
    against q_1 for a residue of it to be left at q_1 or above."""
    if len(q) < 2 or q[0] < 2 * q[1]:
        return []
    q0, q1 = q[0], q[1]
    k = q0 // q1 - 1
    for e in range(q1.bit_length() - 2, 0, -1):
        s = 1 << e
        if barrett_lazy(k * q1 + s, q1) == q1 + s:
            return [H.crt([k * q1 + s, r1] + [1] * (len(q) - 2), q)[0] for r1 in (0, s - 1)]
    return []


def digit_wrap_inputs(q, t):
    """the x of [0, Q) with t x + h = a value of digit_wrap_values (mod Q): the scaling and the decryption rounding run Garner on t x + h"""
    Q = 1
    for m in q:
        Q *= m
    return [(w - (Q - 1) // 2) * pow(t, -1, Q) % Q for w in digit_wrap_values(q)]


def plant_last(vals, extra):
    """`extra` in the place of the last values of `vals` (uniform fill: the planted ones come first)"""
    return list(vals[:len(vals) - len(extra)]) + list(extra)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def lazy(rng, rows, moduli):
    """canonical rows [..][len(moduli)][n] with q added to about half of the words: the calls take words below 2q"""
    up = rng.words(rows.size, 2).reshape(rows.shape).astype(U)
    return rows + up * np.array(moduli, dtype=U)[:, None]


def edge_rows(rng, shape, moduli):
    """moduli.lazy_rows: uniform words, a block in [q, 2q) and the word 2q - 1 in every row -- the largest word the calls promise to take.
    (A planted coefficient row has its transform's words, whatever they are: 2q - 1 is forced on rows of their own.)"""
    x = MD.lazy_rows(rng, shape, moduli)
    q = np.array(moduli, dtype=U)[:, None]
    assert (x < 2 * q).all() and (x == 2 * q - U(1)).any(axis=-1).all() and (x >= q).any(axis=-1).all()
    return x
