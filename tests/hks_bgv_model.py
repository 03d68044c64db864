"""The exact integer model of the BGV calls over the hybrid key switch (include/hehub_amd.h: hp_dev_bgv_hks_switch,
hp_dev_bgv_rotate_hoisted_hks, hp_dev_bgv_relin_modswitch_hks, hp_dev_bgv_mult_relin_modswitch_hks), built on tests/hks_model.py.

Of the hybrid path only ModDown knows the plain modulus t:
    u = ([x]_P * t^-1) mod P,   c = u if u < floor(P/2) else u - P,   delta = t * c,   ModDown_t(x) = (x - delta) / P  mod every q_i
and a BGV key is hks_model.keygen's with the error t * e.  Everything here is on RESIDUES (Python integers; the oracle's transforms for
the NTT ordering, its own BGV mod switch for the drop): what the calls promise, checked with hks_model.residues_match.

Also the planted accumulators: with pt the constant polynomial 1 every digit's integer is 1, every digit row is all ones, and the
accumulator of a switch is sum_d key_d -- so a key whose digit 0 holds NTT_m(w_h mod m) * 2^64 and whose other digits are zero makes
ModDown's input the chosen integers w_h in [0, QP), through the public call.

No test, no fixture: tests/test_hks_bgv_model.py and tests/test_gpu_hks_bgv.py import from here; the model needs no GPU."""
import numpy as np

from hks_model import U, centred, crt, digits_of, model_digits, move

PLAIN_MODULI = (2, 65537, 2147483647)


def prod(xs):
    p = 1
    for x in xs:
        p *= x
    return p


def crt_all(residues, moduli):
    """the integer in [0, prod moduli) behind one residue per modulus"""
    return crt(residues, moduli)[0]


# ---- ModDown_t -----------------------------------------------------------------------------------------------------------------------
def delta_of(x, t, Pm):
    """the remainder ModDown_t subtracts from the accumulator coefficient x (any integer): t * centre(x t^-1 mod P)"""
    u = (x % Pm) * pow(t, -1, Pm) % Pm
    return t * (u if u < Pm // 2 else u - Pm)


def mod_down_int(x, t, Pm):
    """(x - delta) / P as an integer: exact"""
    d = x - delta_of(x, t, Pm)
    assert d % Pm == 0
    return d // Pm


def mod_down_bgv(orc, logn, mext, L, k, t, acc):
    """acc [2][E][n] residues in NTT form (any representatives, Python integers or words) -> ModDown_t, the canonical residues
    [2][L][n] (dtype object) in NTT form.  Coefficient by coefficient: the special-prime part composed, delta, then
    (x_i - delta) P^-1 in every q_i -- the per-modulus form of (x - delta) / P."""
    n, E = 1 << logn, L + k
    pm, Pm = mext[L:], prod(mext[L:])
    out = np.zeros((2, L, n), dtype=object)
    for h in range(2):
        coef = [orc.intt(logn, mext[m], np.array([int(w) % mext[m] for w in acc[h][m]], dtype=U)).astype(object) % mext[m]
                for m in range(E)]
        deltas = [delta_of(crt_all([coef[L + a][i] for a in range(k)], pm), t, Pm) for i in range(n)]
        for m in range(L):
            q = mext[m]
            pinv = pow(Pm % q, -1, q)
            vals = np.array([(int(coef[m][i]) - deltas[i]) * pinv % q for i in range(n)], dtype=U)
            out[h, m] = orc.ntt(logn, q, vals).astype(object) % q
    return out


def inner(mext, D, key):
    """sum_d D_d * key_d with its one Montgomery reduction, residues [2][E][n] (dtype object)"""
    E = len(mext)
    Do, Ko = D.astype(object), key.astype(object)
    return np.array([[sum(Do[d, m] * Ko[d, h, m] for d in range(D.shape[0])) * pow(1 << 64, -1, mext[m]) % mext[m] for m in range(E)]
                     for h in range(2)], dtype=object)


def model_switch_bgv(orc, logn, mext, L, k, alpha, t, pt, key):
    """hp_dev_bgv_hks_switch for one polynomial: pt [L][n], key [nd][2][E][n] -> canonical residues [2][L][n] (dtype object)"""
    D = model_digits(orc, logn, mext, L, k, alpha, np.ascontiguousarray(pt))
    return mod_down_bgv(orc, logn, mext, L, k, t, inner(mext, D, key))


def model_hoisted_bgv(orc, logn, mext, L, k, alpha, t, ct, keys, steps, conj, D=None):
    """hp_dev_bgv_rotate_hoisted_hks for one ciphertext: ct [2][L][n] -> [R][2][L][n] (dtype object): the digit rows of the
    unrotated c1 moved (hks_model.model_hoisted's signed-digit property), ModDown_t, + the moved c0.  D: the digit rows of ct[1],
    where the caller already has them (they do not depend on t)"""
    if D is None:
        D = model_digits(orc, logn, mext, L, k, alpha, np.ascontiguousarray(ct[1]))
    outs = []
    for key, step, cj in zip(keys, steps, conj):
        Dm = np.stack([move(orc, D[d], step, cj) for d in range(D.shape[0])])
        sw = mod_down_bgv(orc, logn, mext, L, k, t, inner(mext, Dm, key))
        c0 = move(orc, ct[0], step, cj).astype(object)
        for m in range(L):
            sw[0, m] = (sw[0, m] + c0[m]) % mext[m]
        outs.append(sw)
    return np.array(outs, dtype=object)


def model_relin_modswitch_bgv(orc, logn, mext, L, k, alpha, t, quad, key):
    """hp_dev_bgv_relin_modswitch_hks for one quadratic ciphertext: quad [3][L][n] -> canonical residues [2][L-1][n] (dtype object).
    (d0, d1) + switch(d2), then the ORACLE's BGV mod switch (hehub's mod_drop_one_prime_inplace, q_last mod t included) on the
    canonical words of that -- arithmetic modulo the q_i: its residues do not depend on the representative it is given."""
    q = mext[:L]
    lin = model_switch_bgv(orc, logn, mext, L, k, alpha, t, quad[2], key)
    qo = quad.astype(object)
    for h in range(2):
        for m in range(L):
            lin[h, m] = (lin[h, m] + qo[h, m]) % q[m]
    out = orc.bgv_mod_drop(q, t, np.ascontiguousarray(lin.astype(U))).astype(object)
    for m in range(L - 1):
        out[:, m] %= q[m]
    return out


def model_mult_bgv(orc, logn, mext, L, k, alpha, t, ct1, ct2, key):
    quad = orc.mult_low_level(mext[:L], np.ascontiguousarray(ct1), np.ascontiguousarray(ct2))
    return model_relin_modswitch_bgv(orc, logn, mext, L, k, alpha, t, quad, key)


# ---- BGV encryption, keys, decryption ---------------------------------------------------------------------------------------------------
def to_ntt(orc, moduli, coeffs):
    """integer coefficients (any sign, any size) -> strict NTT rows [len(moduli)][n]"""
    rows = np.stack([np.array([int(c) % m for c in coeffs], dtype=U) for m in moduli])
    return orc.poly_reduce_strict(moduli, orc.poly_ntt(moduli, rows))


def ternary(rng, n):
    return rng.words(n, 3).astype(np.int64) - 1


def small_errors(rng, n, bound=8):
    return rng.words(n, 2 * bound + 1).astype(np.int64) - bound


def encrypt_bgv(orc, rng, q, t, s, msg):
    """ct [2][L][n] in NTT form with c0 + c1 s = msg + t e: msg integer coefficients in [0, t), s the secret's coefficients"""
    n = len(msg)
    c1 = rng.poly((len(q), n), q)
    body = to_ntt(orc, q, [int(m) + t * int(e) for m, e in zip(msg, small_errors(rng, n))])
    c0 = orc.poly_sub(q, body, orc.poly_mul(q, c1, to_ntt(orc, q, s)))
    return np.stack([orc.poly_reduce_strict(q, c0), c1])


def phase(orc, q, s, ct):
    """the centred integer coefficients of c0 + c1 s"""
    ct = np.ascontiguousarray(ct)
    return centred(orc, q, orc.poly_add(q, ct[0], orc.poly_mul(q, ct[1], to_ntt(orc, q, s))))


def decrypt_bgv(orc, q, t, s, ct):
    """the message in [0, t): the centred phase modulo t"""
    return np.array([int(v) % t for v in phase(orc, q, s, ct)], dtype=object)


def keygen_bgv(orc, rng, logn, mext, L, k, alpha, t, s_to, s_from, bound=8):
    """hks_model.keygen with the error t * e: row d = RLWE encryption under s_to of (P mod q_i) * s_from on the limbs of digit d,
    u64[nd][2][E][n] in NTT + Montgomery form -- what hp_dev_hks_keygen writes for the error rows t * e"""
    n, E = 1 << logn, L + k
    digs = digits_of(L, alpha)
    Pm = prod(mext[L:])
    key = np.zeros((len(digs), 2, E, n), dtype=U)
    to_rows, from_rows = to_ntt(orc, mext, s_to), to_ntt(orc, mext, s_from)
    for d, limbs in enumerate(digs):
        a = rng.poly((E, n), mext)
        e_rows = to_ntt(orc, mext, [t * int(e) for e in small_errors(rng, n, bound)])
        b = orc.poly_sub(mext, e_rows, orc.poly_mul(mext, a, to_rows))
        msg = np.zeros((E, n), dtype=U)
        for m in limbs:
            msg[m] = orc.poly_rns_scalar_mul([mext[m]], from_rows[m][None], [Pm % mext[m]])[0]
        b = orc.poly_reduce_strict(mext, orc.poly_add(mext, b, msg))
        mont = [(1 << 64) % m for m in mext]
        key[d, 0] = orc.poly_reduce_strict(mext, orc.poly_rns_scalar_mul(mext, b, mont))
        key[d, 1] = orc.poly_reduce_strict(mext, orc.poly_rns_scalar_mul(mext, a, mont))
    return key


def negacyclic(a, b, mod=None):
    """the product of two integer polynomials modulo X^n + 1 (and modulo `mod`, into [0, mod))"""
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            if i + j < n:
                out[i + j] += int(x) * int(y)
            else:
                out[i + j - n] -= int(x) * int(y)
    return np.array([v % mod if mod else v for v in out], dtype=object)


def negacyclic_ntt(orc, moduli, a, b, mod=None):
    """the same through the transforms, for degrees at which the schoolbook product is slow: exact while every coefficient of the
    product is below half the product of `moduli` in magnitude"""
    out = centred(orc, moduli, orc.poly_mul(moduli, to_ntt(orc, moduli, a), to_ntt(orc, moduli, b)))
    return np.array([int(v) % mod if mod else int(v) for v in out], dtype=object)


def moved_coeffs(orc, moduli, coeffs, step, cj):
    """the automorphism of a rotation entry on an integer polynomial with small coefficients: through the NTT form and back"""
    return centred(orc, moduli, move(orc, to_ntt(orc, moduli, coeffs), step, cj))


# ---- planted accumulators --------------------------------------------------------------------------------------------------------------
def planted_values(rng, mext, L, k, t, n):
    """w [2][n] integers in [0, QP): ModDown_t inputs of every edge class.  A coefficient is x = (t c + P y) mod QP for a chosen
    u = c mod P and a chosen quotient y:
      * u in {0, 1, floor(P/2) - 1, floor(P/2), floor(P/2) + 1, P - 1}, each once, with y cycling through 0, -1 and 3 q_0
        ((x - delta) / P = 0, = -1, = a multiple of q_0)
      * x = 0 and x = QP - 1
      * the rest uniform in [0, QP)"""
    Q, Pm = prod(mext[:L]), prod(mext[L:])
    half = Pm // 2
    us = [0, 1, half - 1, half, half + 1, Pm - 1]
    ys = [0, -1, 3 * mext[0]]
    vals = []
    for j, u in enumerate(us):
        c = u if u < half else u - Pm
        vals.append((t * c + Pm * ys[j % 3]) % (Q * Pm))
    vals += [0, Q * Pm - 1]
    while len(vals) < 2 * n:
        vals.append(crt_all([int(rng.words(1, m)[0]) for m in mext], mext))
    assert len(vals) == 2 * n, "logn >= 3"
    return [vals[0::2], vals[1::2]]   # the classes spread over both polynomials


def planted_classes(w, mext, L, k, t):
    """which of the classes of planted_values occur in w: {name: bool}"""
    Q, Pm = prod(mext[:L]), prod(mext[L:])
    half, q0 = Pm // 2, mext[0]
    xs = [x for row in w for x in row]
    us = {(x % Pm) * pow(t, -1, Pm) % Pm for x in xs}
    ys = [mod_down_int(x, t, Pm) for x in xs]
    found = {f"u={name}": u in us for name, u in (("0", 0), ("1", 1), ("half-1", half - 1), ("half", half), ("half+1", half + 1),
                                                   ("P-1", Pm - 1))}
    # (a negative delta wraps x to x + QP: the quotient then reads y + Q, the same residues)
    found["y=0"] = any(y % Q == 0 for y in ys)
    found["y=-1"] = any(y % Q == Q - 1 for y in ys)
    found["y=multiple of q0"] = any(y % Q != 0 and y % q0 == 0 for y in ys)
    found["x=0"] = 0 in xs
    found["x=QP-1"] = Q * Pm - 1 in xs
    found["random"] = len(set(xs)) > 8
    return found


def planted_key(orc, logn, mext, L, k, alpha, w):
    """the key u64[nd][2][E][n] whose switch of the constant polynomial 1 has the accumulator w: digit 0 = NTT_m(w_h mod m) * 2^64
    mod m, the other digits zero"""
    n, E = 1 << logn, L + k
    key = np.zeros((len(digits_of(L, alpha)), 2, E, n), dtype=U)
    for h in range(2):
        for m in range(E):
            q = mext[m]
            row = orc.ntt(logn, q, np.array([x % q for x in w[h]], dtype=U)).astype(object) % q
            key[0, h, m] = np.array([int(v) * ((1 << 64) % q) % q for v in row], dtype=U)
    return key


def planted_pt(L, n):
    """the constant polynomial 1 in NTT form: all ones"""
    return np.ones((L, n), dtype=U)


def planted_expected(orc, logn, mext, L, k, t, w):
    """plain integer arithmetic: NTT_m( ((x - delta(x)) / P) mod q_m ), canonical residues [2][L][n] (dtype object)"""
    Pm = prod(mext[L:])
    out = np.zeros((2, L, 1 << logn), dtype=object)
    for h in range(2):
        ys = [mod_down_int(x, t, Pm) for x in w[h]]
        for m in range(L):
            q = mext[m]
            out[h, m] = orc.ntt(logn, q, np.array([y % q for y in ys], dtype=U)).astype(object) % q
    return out

