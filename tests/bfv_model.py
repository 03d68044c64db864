"""The exact integer model of the BFV calls (include/hehub_amd.h: hp_dev_bfv_lift, hp_dev_bfv_scale_round, hp_dev_bfv_mult_low_level,
hp_dev_bfv_mult_relin_hks, hp_dev_bfv_decrypt_round), the conventions they pin, and the planted-value generators of the tests.

    Q = q_0...q_{L-1} odd, h = (Q - 1) / 2; B = b_0...b_{M-1}; qb = q.., b..; t the plain modulus
    centre_X(x) = x if x < floor(X/2) else x - X
    lift        centre_Q(x) of the integer behind the strict coefficient residues over Q, reduced into every b_j
    scale       the residue mechanics: v = t x + h residue-wise; r = [v]_Q in [0, Q), NOT centred; y = (v - r) Q^-1 mod b_j;
                centre_B(y) into every q_i.  For |t x + h| < Q B / 2 and |y| < B / 2 that is y = floor((t x + h) / Q)
    decryption  m = (h - r) Q^-1 mod t, r = [t x + h]_Q reduced mod t  =  floor((t x + h) / Q) mod t  for x in [0, Q)

Python integers via CRT; the oracle's transforms where the engine uses hehub's (the NTT ordering), every output word canonical.
No test, no fixture: tests/test_bfv_model.py and tests/test_gpu_bfv.py import from here; the model needs no GPU
(tests/test_bfv_model.py holds it to schoolbook arithmetic)."""
import numpy as np

import hks_model as H

U = np.uint64


import moduli as MD
import params as P

T0, PLAIN_MODULI = 65537, (65537, 2, 2147483647)
# (logn, L, M, k, alpha) of tests/test_gpu_bfv.py: Garner width 1; two plain shapes; one spare aux prime and a single digit; bases of
# different widths; the widest templated Garner on Q with the guarded width on B; tiled transforms (the only shape where parity
# level A applies); moduli off the prime table
GPU_SHAPES = [(3, 1, 2, 1, 1), (4, 2, 3, 2, 2), (4, 3, 4, 1, 1), (4, 3, 5, 2, 3), (4, 4, 4, 2, 2), (4, 8, 9, 4, 4), (11, 2, 3, 2, 2),
              (4, 3, 5, 1, 3)]
WIDE_AUX, OFF_TABLE = GPU_SHAPES[4], GPU_SHAPES[7]
DECRYPT_SHAPES = [GPU_SHAPES[1], GPU_SHAPES[3], GPU_SHAPES[6]]
EXTRA40 = P.ntt_primes(3, 11, 40, exclude=P.P40)   # P40 has ten primes: the 8 + 9 shape takes the rest from P50 and from here


def shape_moduli(shape):
    """(mext = q.. + special primes, aux) of a GPU shape"""
    logn, L, M, k, alpha = shape
    if shape == OFF_TABLE:
        return MD.HIGHMID[:3] + [P.P50[0]], list(MD.ABOVE)
    mext = H.chain(L, k)
    if shape == WIDE_AUX:
        return mext, P.P50[:4]
    aux = (P.P40[L:] + P.P50 + EXTRA40)[:M]
    return mext, aux


def shape_plain_moduli(shape):
    """t = 65537 everywhere; t = 2 and t = 2^31 - 1 on the first and the last P40 shape wherever the base-size rule still holds"""
    logn, L, M, k, alpha = shape
    mext, aux = shape_moduli(shape)
    ts = PLAIN_MODULI if shape in (GPU_SHAPES[0], GPU_SHAPES[6]) else (T0,)
    return tuple(t for t in ts if t == T0 or base_ok(mext[:L] + aux, L, t, 1 << logn))


def prod(xs):
    p = 1
    for x in xs:
        p *= x
    return p


def centre(x, X):
    return x if x < X // 2 else x - X


def base_ok(qb, L, t, n):
    """the calls' base-size rule, B >= 4 t N Q"""
    return prod(qb[L:]) >= 4 * t * n * prod(qb[:L])


def tensor_bound(Q, n):
    """|x| <= N (Q + 1)^2 / 2 for every coefficient of a product of two centred polynomials (and of the sum of two such products / 2)"""
    return n * (Q + 1) ** 2 // 2


# ---- rows <-> integers -------------------------------------------------------------------------------------------------------------
def coeff_rows(orc, moduli, rows):
    """NTT-form rows [len(moduli)][n] (words below 2q) -> strict coefficient rows"""
    rows = np.ascontiguousarray(rows)
    return orc.poly_reduce_strict(moduli, orc.poly_intt(moduli, rows))


def ints_of(coef, moduli):
    """strict coefficient rows -> the integers in [0, prod moduli), one per coefficient"""
    return [H.crt([coef[a][i] for a in range(len(moduli))], moduli)[0] for i in range(coef.shape[1])]


def ntt_rows(orc, logn, moduli, ints):
    """integers (any sign, any size) -> canonical NTT rows [len(moduli)][n]"""
    return np.stack([orc.ntt(logn, q, np.array([int(x) % q for x in ints], dtype=U)) % U(q) for q in moduli])


# ---- the three rules on integers -----------------------------------------------------------------------------------------------------
def scale_int(x, t, Q):
    """floor((t x + h) / Q): rounding to nearest, no ties (Q odd)"""
    return (t * x + (Q - 1) // 2) // Q


def scale_residues(xq, xb, q, b, t):
    """the residue mechanics for one coefficient: residues of x over q and over b -> the integer centre_B(y)"""
    Q, Bp = prod(q), prod(b)
    h = (Q - 1) // 2
    r = H.crt([(t * int(x) + h) % m for x, m in zip(xq, q)], q)[0]                          # [v]_Q, in [0, Q)
    y = H.crt([((t * int(x) + h - r) * pow(Q % m, -1, m)) % m for x, m in zip(xb, b)], b)[0]
    return centre(y, Bp)


def decrypt_int(x, t, Q):
    return scale_int(x, t, Q) % t


def decrypt_residues(xq, q, t):
    """the decryption rule for one coefficient from its residues over q"""
    Q = prod(q)
    h = (Q - 1) // 2
    r = H.crt([(t * int(x) + h) % m for x, m in zip(xq, q)], q)[0]
    return (h - r) * pow(Q % t, -1, t) % t


# ---- the calls, one polynomial / ciphertext at a time ----------------------------------------------------------------------------------
def lift(orc, logn, qb, L, x):
    """hp_dev_bfv_lift: x [L][n] NTT form over Q -> [L + M][n] canonical words"""
    q, b = qb[:L], qb[L:]
    Q = prod(q)
    vals = [centre(v, Q) for v in ints_of(coeff_rows(orc, q, x), q)]
    return np.concatenate([np.ascontiguousarray(x) % np.array(q, dtype=U)[:, None], ntt_rows(orc, logn, b, vals)])


def scale(orc, logn, qb, L, t, x):
    """hp_dev_bfv_scale_round: x [L + M][n] NTT form over Q B -> [L][n] canonical words"""
    q, b = qb[:L], qb[L:]
    coef = coeff_rows(orc, qb, x)
    ys = [scale_residues(coef[:L, i], coef[L:, i], q, b, t) for i in range(coef.shape[1])]
    return ntt_rows(orc, logn, q, ys)


def mult_low_level(orc, logn, qb, L, t, ct1, ct2):
    """hp_dev_bfv_mult_low_level: ct1, ct2 [2][L][n] -> [3][L][n] canonical words: lift, hehub's tensor product over L + M limbs, scale"""
    a = np.stack([lift(orc, logn, qb, L, ct1[h]) for h in range(2)])
    c = np.stack([lift(orc, logn, qb, L, ct2[h]) for h in range(2)])
    wide = orc.mult_low_level(qb, np.ascontiguousarray(a), np.ascontiguousarray(c))
    return np.stack([scale(orc, logn, qb, L, t, wide[j]) for j in range(3)])


def mult_relin(orc, logn, mext, L, k, alpha, aux, t, ct1, ct2, key):
    """hp_dev_bfv_mult_relin_hks: the quadratic ciphertext, then hks_model.model_switch of y2 with (y0, y1) added -> the canonical
    residues [2][L][n] (dtype object)"""
    q = mext[:L]
    quad = mult_low_level(orc, logn, list(q) + list(aux), L, t, ct1, ct2)
    sw = H.model_switch(orc, logn, mext, L, k, alpha, np.ascontiguousarray(quad[2]), key).astype(object)
    qo = quad.astype(object)
    for h in range(2):
        for m in range(L):
            sw[h, m] = (sw[h, m] + qo[h, m]) % q[m]
    return sw


def decrypt_round(q, t, x):
    """hp_dev_bfv_decrypt_round: x [L][n] strict coefficient rows -> [n] words below t"""
    return np.array([decrypt_residues(x[:, i], q, t) for i in range(x.shape[1])], dtype=U)


# ---- plain arithmetic to hold the model to -----------------------------------------------------------------------------------------------
def negacyclic(a, b):
    """schoolbook product of integer polynomials modulo X^n + 1"""
    n = len(a)
    out = [0] * n
    for i in range(n):
        for j in range(n):
            if i + j < n:
                out[i + j] += int(a[i]) * int(b[j])
            else:
                out[i + j - n] -= int(a[i]) * int(b[j])
    return out


def encrypt(orc, rng, logn, q, t, s, m, bound=3):
    """a BFV ciphertext [2][L][n] (canonical NTT words) of the message m (integers below t) under the ternary secret s"""
    n, Q = 1 << logn, prod(q)
    a = ints_of(rng.poly((len(q), n), q), q)   # uniform in [0, Q)
    e = (rng.words(n, 2 * bound + 1).astype(np.int64) - bound)
    a_s = negacyclic(a, s)
    c0 = [(Q // t) * int(m[i]) + int(e[i]) - a_s[i] for i in range(n)]
    return np.stack([ntt_rows(orc, logn, q, c0), ntt_rows(orc, logn, q, a)])


def decrypt_quadratic(orc, q, t, s, quad):
    """quad [3][L][n]: the rounding of y0 + y1 s + y2 s^2 (mod Q) -> [n] integers below t"""
    Q = prod(q)
    y = [[centre(v, Q) for v in ints_of(coeff_rows(orc, q, quad[j]), q)] for j in range(3)]
    s2 = negacyclic(s, s)
    y1s, y2s2 = negacyclic(y[1], s), negacyclic(y[2], s2)
    return [decrypt_int((y[0][i] + y1s[i] + y2s2[i]) % Q, t, Q) for i in range(len(s))]


# ---- planted values --------------------------------------------------------------------------------------------------------------------
def fill(rng, planted, slots, lo, hi):
    """the planted integers first, then uniform integers of [lo, hi] up to `slots` values"""
    assert len(planted) <= slots, (len(planted), slots)
    span = hi - lo + 1
    out = list(planted)
    while len(out) < slots:
        w = 0
        for _ in range(span.bit_length() // 64 + 2):
            w = (w << 64) | int(rng.words(1)[0])
        out.append(lo + w % span)
    return out


def lift_planted(rng, qb, L, slots):
    """coefficients in [0, Q) for the lift: 0, floor(Q/2) - 1, floor(Q/2), floor(Q/2) + 1, Q - 1, and for every b_j the largest multiple
    of b_j below the half and the smallest x from the half on with x - Q a multiple of b_j (where b_j is small enough to have one)"""
    q, b = qb[:L], qb[L:]
    Q = prod(q)
    half = Q // 2
    vals = [0, half - 1, half, half + 1, Q - 1]
    for bj in b:
        vals.append((half - 1) // bj * bj)
        m = (Q - half) // bj
        if m:
            vals.append(Q - m * bj)
    return fill(rng, vals, slots, 0, Q - 1)


def lift_classes(vals, qb, L):
    q, b = qb[:L], qb[L:]
    Q = prod(q)
    half = Q // 2
    cls = {"zero": 0 in vals, "half-1": half - 1 in vals, "half": half in vals, "half+1": half + 1 in vals, "Q-1": Q - 1 in vals}
    for j, bj in enumerate(b):
        cls["multiple of b%d below the half" % j] = any(v < half and v % bj == 0 for v in vals)
        if (Q - half) // bj:   # (b_j > Q / 2 has no multiple in [-Q/2, 0))
            cls["multiple of b%d above the half" % j] = any(v >= half and (v - Q) % bj == 0 for v in vals)
    return cls


def scale_planted(rng, qb, L, t, n, slots):
    """signed integers x, |x| <= N (Q + 1)^2 / 2, for the scaling: for c in {0, 1, h, h + 1, Q - 1} the x = c t^-1 mod Q + j Q (so that
    t x + h = c + h mod Q: the rounding's edges) with j at both ends of the range -- and j = 0 where the slots allow --, x = 0, 1, -1,
    and the x with y = -1 and y = 0 around t x + h = 0"""
    Q = prod(qb[:L])
    h, bound = (Q - 1) // 2, tensor_bound(Q, n)
    tinv = pow(t, -1, Q)
    ends, mids = [], []
    for c in (0, 1, h, h + 1, Q - 1):
        x0 = c * tinv % Q
        ends += [x0 + ((bound - x0) // Q) * Q, x0 - ((bound + x0) // Q) * Q]
        mids.append(x0)
    vals = ends + [0, 1, -1, -(h // t) - 1, -(h // t)]
    if len(vals) + len(mids) < slots:
        vals += mids
    assert all(abs(v) <= bound for v in vals)
    return fill(rng, vals, slots, -bound, bound)


def scale_classes(vals, qb, L, t, n):
    Q = prod(qb[:L])
    h, bound = (Q - 1) // 2, tensor_bound(Q, n)
    cls = {"x = 0": 0 in vals, "x = 1": 1 in vals, "x = -1": -1 in vals,
           "y = -1": any(scale_int(v, t, Q) == -1 for v in vals), "y = 0": any(scale_int(v, t, Q) == 0 and v != 0 for v in vals),
           "random": len(vals) > 15}
    for c in (0, 1, h, h + 1, Q - 1):
        hit = [v for v in vals if (t * v - c) % Q == 0]
        cls["c = %d at the top" % c] = any(v > bound - Q for v in hit)
        cls["c = %d at the bottom" % c] = any(v < -bound + Q for v in hit)
    return cls


def decrypt_planted(rng, q, t, slots):
    """x in [0, Q): 0, 1, h, h + 1, Q - 1 and the solutions of t x + h = 0 and = Q - 1 (mod Q)"""
    Q = prod(q)
    h, tinv = (Q - 1) // 2, pow(t, -1, Q)
    return fill(rng, [0, 1, h, h + 1, Q - 1, (-h) * tinv % Q, (Q - 1 - h) * tinv % Q], slots, 0, Q - 1)


def decrypt_classes(vals, q, t):
    Q = prod(q)
    h = (Q - 1) // 2
    return {"0": 0 in vals, "1": 1 in vals, "h": h in vals, "h+1": h + 1 in vals, "Q-1": Q - 1 in vals,
            "t x + h = 0": any((t * v + h) % Q == 0 for v in vals), "t x + h = Q - 1": any((t * v + h) % Q == Q - 1 for v in vals)}


def residue_rows(ints, moduli):
    """integers -> strict coefficient rows [len(moduli)][len(ints)]"""
    return np.array([[int(x) % m for x in ints] for m in moduli], dtype=U)
