"""Inputs and range arithmetic for the BGV calls over the hybrid key switch, lazy relinearisation and the any-level (_at) calls on wide
and off-table moduli (tests/test_gpu_hks_bgv_moduli.py on the GPU, tests/test_hks_bgv_edges.py for the inputs' own conditions, no GPU).
The pattern of tests/hks_edges.py, whose chains, fills and range arithmetic are imported, not copied.

Chains: hks_edges.chain_of for W59, ABOVE, PACKEDGE, HIGHMID, LOWMID and WIDE58 (HIGHMID gets one more special prime of its own kind for
the shape with k = 3), NARROW once with t = 2 (its 20-bit limbs refuse the sweep's 2^31 - 1: t < every modulus), and W59LAST:
the 59-bit prime as the LAST ciphertext modulus over 40-bit limbs -- the BGV drop's quotient at a wide q_last after ModDown_t.
WIDE58R is WIDE58 with its ciphertext moduli reordered so that the 58-bit high_mid prime is q_last: the calls that end in one of hehub's
drops have a model only where no high_mid limb is KEPT by the drop (drop_premise below), which WIDE58 and HIGHMID themselves are not.

The premise the exact models (tests/hks_bgv_model.py) rest on: the oracle's transforms of the words the model hands them are congruent
to the true transforms.  The model hands them strict rows (below q) everywhere, the input bound behind the figures of
tests/test_hks_edges.py (moduli.fold_bound(q, q, logn)); the DEVICE hands the inverse transforms of the special primes and of the last
ciphertext modulus lazy words (below 2q: the inner product's Montgomery words, the drop's input), so there the bound is 2q -- the model
and the device then transform different representatives of the same residues, and agree only if hehub's fold does not wrap for either.
`premise` is both; the case lists below hold only (chain, degree) pairs that pass it -- tests/test_hks_bgv_edges.py asserts that, nothing is
skipped at run time.  LOWMID's 1.1 * 2^40 limb passes at N = 16 (9 q = 9.9 * 2^40: m = 9, 9 delta < 2^40) and fails from N = 32 on,
which is why every chain is swept at logn 4 and the tiled degree is left to W59, HIGHMID and WIDE58."""
import numpy as np

import hks_edges as H
import moduli as M
import params as P

U = np.uint64
F = M.FAMILIES
T0 = 65537
BATCH = 2

# ---- chains --------------------------------------------------------------------------------------------------------------------------
SWEEP_CHAINS = H.MODEL_CHAINS                  # W59, ABOVE, PACKEDGE, HIGHMID, LOWMID, WIDE58: NARROW is not in the t-sweep
WIDE_CHAINS = ("W59", "HIGHMID", "WIDE58")     # the tiled degree, the max fill, the dot
PLANTED_CHAINS = ("WIDE58", "HIGHMID", "ABOVE")
MORE_P = {"HIGHMID": [F[49]["high_mid"], F[48]["high_mid"]]}       # special primes in front of hks_edges' own, where k asks for more


def chain_of(name, L, k):
    """hks_edges.chain_of, and the chains of this file's own"""
    if name == "W59LAST":
        return P.P40[:L - 1] + [M.Q59] + P.P50[:k]
    if name == "NARROW":
        return M.NARROW[:L] + M.NARROW[-k:]
    if name == "WIDE58R":
        m, hm = H.wide58(L, k), F[58]["high_mid"]
        return [q for q in m[:L] if q != hm] + [hm] + m[L:]
    if name in MORE_P and L + k > len(M.CHAINS[name]):
        kk = min(k, 1 + len(H.EXTRA[name]["p"]))
        short = H.chain_of(name, L, kk)
        return short[:L] + MORE_P[name][:k - kk] + short[L:]
    return H.chain_of(name, L, k)


# ---- shapes (logn, L, k, alpha): the smallest at which each path exists -----------------------------------------------------------------
FIRST = (4, 4, 2, 2)
PARTIAL = (4, 5, 2, 3)       # a partial last digit
SHORT = (4, 2, 3, 3)         # L < alpha: every ciphertext-modulus digit row is the caller's own word
WIDEST = (4, 3, 8, 3)        # the widest Garner, on WIDE58 only
TILED = (11, 3, 2, 2)        # the tiled transforms and the fused drop
SMALL_SHAPES = [FIRST, PARTIAL, SHORT]
NARROW_CASE = ("NARROW", 3, 3, 2, 2)           # [20, 20, 30 | 30, 59 bits], t = 2; N = 8: the 2^20 + 2^17 limb passes the premise up to there
DOT_SHAPES = [(5, 4, 2, 2), TILED]


# The (chain, degree) pairs of the sweep that FAIL the premise (below) and are therefore in no case list.  LOWMID cut to (5, 2) takes the
# 1.1 * 2^45 prime as a special prime: the device hands its inverse transform words below 2p, 10 p = 11 * 2^45 gives m = 11 and
# 11 delta = 1.1 * 2^45 >= 2^45 -- hehub's fold may wrap there already at N = 16.  (As a ciphertext modulus, where only strict rows are
# transformed, the 1.1 * 2^40 limb of the same chain passes at N = 16.)
PREMISE_FAILS = [("LOWMID",) + PARTIAL]
LEVEL_A_CASE = ("ABOVE",) + TILED              # 2^k + small limbs below 2^50 at a tiled degree: the one chain here that level A serves


def sweep_cases():
    """(name, logn, L, k, alpha): every chain x the small shapes, the widest Garner on WIDE58, the tiled degree on the wide chains
    and on the chain level A serves"""
    out = [(name,) + s for name in SWEEP_CHAINS for s in SMALL_SHAPES if (name,) + s not in PREMISE_FAILS]
    return out + [("WIDE58",) + WIDEST] + [(name,) + TILED for name in WIDE_CHAINS] + [LEVEL_A_CASE]


def edge_t(mext):
    """the largest odd plain modulus the ABI takes for the chain: t < every modulus, and the moduli are odd primes, so min - 1 is even
    and min - 2 it is (below a prime: invertible modulo every modulus)"""
    t = min(mext) - 1
    return t if t % 2 else t - 1


def plain_moduli(case):
    """t = 65537 everywhere, t = 2 and 2^31 - 1 on the first and the last shape"""
    return (T0, 2, 2147483647) if case[1:] in (FIRST, TILED) else (T0,)


EDGE_T_CASE = ("WIDE58",) + FIRST              # t = min(chain) - 2: a 58-bit plain modulus
MAX_CASES = [(name,) + FIRST for name in WIDE_CHAINS]
PLANTED_CASES = [(name,) + FIRST for name in PLANTED_CHAINS]
HOISTED_CASES = [(name,) + FIRST for name in SWEEP_CHAINS] + [("WIDE58",) + PARTIAL, ("HIGHMID",) + SHORT] + \
                [(name,) + TILED for name in ("HIGHMID", "WIDE58")]
# relinearisation + mod switch: the model's drop is hehub's own (oracle.bgv_mod_drop), which is a function of the residues only where
# drop_premise (below) holds -- no high_mid limb below q_last.  HIGHMID and WIDE58 (whose high_mid prime is q_0) fail it at every shape
# but WIDE58's (2, 3) cut, two 58-bit limbs (DROP_FAILS).  WIDE58R, the same primes with the high_mid one as q_last, stands in for WIDE58
# up to L + k = 6 (a longer cut draws a second high_mid prime); the partial last digit and L < alpha are run on ABOVE, PACKEDGE and WIDE58
RELIN_CASES = [(name,) + FIRST for name in ("W59", "ABOVE", "PACKEDGE", "LOWMID", "WIDE58R", "W59LAST")] + \
              [("ABOVE",) + PARTIAL, ("PACKEDGE",) + SHORT, ("WIDE58",) + SHORT] + [(name,) + TILED for name in ("W59", "WIDE58R")]
DROP_FAILS = [(name,) + s for name in ("HIGHMID", "WIDE58") for s in (FIRST, PARTIAL, SHORT, TILED) if (name, s) != ("WIDE58", SHORT)]
RELIN_WORD_CASES = [(name,) + s for name in ("HIGHMID", "WIDE58") for s in (FIRST, TILED)]      # no model: the fused call against its halves
# the dot's model ends in hehub's rescale: the same premise.  HIGHMID and WIDE58 are run against the two calls the dot is composed of,
# word for word (the same code on the same quad: no model, no premise)
DOT_CASES = [(name,) + s for name in ("W59", "WIDE58R") for s in DOT_SHAPES]
DOT_WORD_CASES = [(name,) + s for name in ("HIGHMID", "WIDE58") for s in DOT_SHAPES]
DOT_MAX_CASE = ("WIDE58R", 5, 4, 2, 2)
DECRYPT_CASES = [("WIDE58R",) + FIRST, ("WIDE58R",) + TILED]
# (name, logn, key_L0, L, k, alpha): a top key of key_L0 = L + 2 moduli called at levels L and L - 1; at L the last digit is partial
# (alpha = 3 at L = 4, alpha = 2 at L = 3), at L - 1 it is full
AT_CASES = [("WIDE58", 4, 6, 4, 2, 3), ("HIGHMID", 4, 5, 3, 2, 2), ("WIDE58", 11, 5, 3, 2, 2), ("HIGHMID", 11, 5, 3, 2, 2)]


# hks_edges.covers (P at least every digit's product) is what the NOISE of a switch needs, not its residues: ModUp lifts the digit's
# exact non-negative integer whatever its size and ModDown_t divides exactly, so the models hold on any chain.  The shapes above are fixed
# and the named chains are what they are, so these cases have alpha limbs wider than their k special primes together (a 59-bit limb
# beside a 40-bit one against 40 + 50 bits; three limbs against two primes of the same width; two 40-bit limbs against two 40-bit primes
# a trifle smaller).  They are compared on residues only; every case that DECRYPTS is covered (tests/test_hks_bgv_edges.py holds both).
UNCOVERED = [("W59",) + FIRST, ("W59",) + PARTIAL, ("W59",) + TILED, ("W59", 5, 4, 2, 2), ("ABOVE",) + PARTIAL, ("PACKEDGE",) + FIRST,
             ("PACKEDGE",) + PARTIAL, ("HIGHMID",) + PARTIAL, ("LOWMID",) + FIRST, ("WIDE58",) + PARTIAL]
UNCOVERED_AT = [("WIDE58", 4, 6, 4, 2, 3)]     # alpha = 3 limbs of 59 bits against two 60-bit primes, at both levels


def at_chains(name, key_L0, k):
    """the top chain of an _at case"""
    return chain_of(name, key_L0, k)


def every_case():
    """every (name, logn, L, k, alpha) some test of tests/test_gpu_hks_bgv_moduli.py runs (the _at cases have their own list)"""
    out = sweep_cases() + [NARROW_CASE, EDGE_T_CASE] + MAX_CASES + PLANTED_CASES + HOISTED_CASES + RELIN_CASES + RELIN_WORD_CASES
    out += DOT_CASES + DOT_WORD_CASES + [DOT_MAX_CASE] + DECRYPT_CASES
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


# ---- the premise ---------------------------------------------------------------------------------------------------------------------------
def premise(mext, L, logn):
    """see the module's docstring: no fold wraps for strict rows at any modulus, nor for lazy words at the special primes and q_last"""
    strict = all(not M.fold_bound(q, q, logn)[0] for q in mext)
    lazy = all(not M.fold_bound(q, 2 * q, logn)[0] for q in mext[L - 1:])
    return strict and lazy


def drop_premise(q, logn):
    """What the models of the calls that end in one of hehub's drops (bgv::mod_drop_one_prime_inplace, ckks rescale) rest on: hehub
    subtracts the lazy forward transform of the remainder rows with a lazy subtraction that takes its operand below 2q, so the result is
    a function of the residues only if that transform's words stay below 2q at every modulus that is kept -- the second half of
    moduli.hehub_fold_exact.  At a high_mid modulus (kb = k + 1, large delta) they do not: the subtraction wraps, what comes out depends
    on the representative it is subtracted from, and is not (x - rem) / q_last for any of them (tests/test_hks_bgv_edges.py shows it:
    1432 of 2048 residues of the high_mid limb of HIGHMID, on canonical input).  The engine's drop follows hehub word for word there, as
    its contract says, on the lazy words of ITS switch; the model runs hehub on canonical words; the two then differ."""
    return all(M.fold_bound(m, 2 * m, logn)[2] <= 2 * m for m in q[:-1])


def exact_mod_drop(orc, logn, q, t, lin):
    """hehub's BGV mod switch in Python integers: lin [2][L][n] (any representatives) -> the canonical residues [2][L-1][n] of
    (c_i - t * centre([c_last t^-1]_{q_last})) * q_last^-1 * (q_last mod t), centre(u) = u - q_last from floor(q_last / 2) on"""
    L, n, ql = len(q), 1 << logn, q[-1]
    out = np.zeros((2, L - 1, n), dtype=object)
    for h in range(2):
        coef = [orc.intt(logn, q[m], np.array([int(w) % q[m] for w in lin[h][m]], dtype=U)).astype(object) % q[m] for m in range(L)]
        u = [int(c) * pow(t, -1, ql) % ql for c in coef[L - 1]]
        cen = [x - ql if x >= ql // 2 else x for x in u]
        for m in range(L - 1):
            f = pow(ql % q[m], -1, q[m]) * (ql % t)
            out[h, m] = orc.ntt(logn, q[m], np.array([(int(coef[m][i]) - t * cen[i]) * f % q[m] for i in range(n)], dtype=U)).astype(object) % q[m]
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
FILLS = H.FILLS[:3]          # lazy, kinds, max


def nd_of(L, alpha):
    return (L + alpha - 1) // alpha


def seed_of(case, salt=0):
    name, logn, L, k, alpha = case
    return 9500 + 131 * (sorted(SWEEP_CHAINS + ("NARROW", "W59LAST", "WIDE58R")).index(name)) + 17 * logn + 5 * L + k + salt


def rows(rng, fill, shape, moduli):
    """[..., len(moduli), n] words of a fill: lazy = moduli.lazy_rows (strict words, a block in [q, 2q), some 2q - 1); kinds = every
    row one of moduli.INPUT_KINDS, cycled; max = every word 2q - 1"""
    if fill == "lazy":
        return M.lazy_rows(rng, shape, moduli)
    if fill == "kinds":
        return H.kind_rows(rng, shape, moduli)
    return H.max_rows(shape, moduli)


def key_rows(rng, fill, mext, nd, n, start=0):
    """a key [nd][2][E][n]: uniform below 2q, rows of every kind, or every word 2q - 1"""
    shape = (nd, 2, len(mext), n)
    if fill == "lazy":
        return H.lazy_uniform(rng, shape, mext)
    if fill == "kinds":
        return H.kind_rows(rng, shape, mext, start=start)
    return H.max_rows(shape, mext)


def switch_inputs(case, fill, batch=BATCH):
    """(mext, pt [batch][L][n], key [nd][2][E][n]) of a switch case"""
    from oracle.pyoracle import SplitMix

    name, logn, L, k, alpha = case
    mext, n = chain_of(name, L, k), 1 << logn
    rng = SplitMix(seed_of(case, FILLS.index(fill)))
    return mext, rows(rng, fill, (batch, L, n), mext[:L]), key_rows(rng, fill, mext, nd_of(L, alpha), n)


def planted(case, t):
    """hks_bgv_model.planted_values of a case: the ModDown_t inputs w [2][n] of every edge class, for the plain modulus t"""
    from hks_bgv_model import planted_values
    from oracle.pyoracle import SplitMix

    name, logn, L, k, alpha = case
    return planted_values(SplitMix(seed_of(case, 40 + t % 1000)), chain_of(name, L, k), L, k, t, 1 << logn)


# ---- range arithmetic ----------------------------------------------------------------------------------------------------------------------
def max_fill_sums(orc, case):
    """the digit-loop sums of the max fill's switch, recomputed with Python integers (hks_edges.sums, one rotation: step 0, no
    diagonals): {"inner": (largest sum_d digit * key, (modulus index, 0)), "digit": ..., "ratio": ..., "word": ...}.  pt stands in as
    c1; c0 = 0 adds nothing"""
    name, logn, L, k, alpha = case
    mext, pt, key = switch_inputs(case, "max", batch=1)
    ct = np.stack([np.zeros_like(pt[0]), pt[0]])
    return mext, H.sums(orc, logn, mext, L, k, alpha, ct, [(key, 0, False)], [], carries=False)


def report_max_fill(case, mext, worst):
    """one line: how close the largest digit-loop sum comes to 2^128"""
    v, where = worst["inner"]
    lg = float(np.log2(float(v)))
    print(f"{case}: largest digit-loop sum 2^{lg:.3f} at modulus {where[0]} ({mext[where[0]].bit_length()} bits), "
          f"2^128 / sum = 2^{128 - lg:.3f}; largest digit word {worst['ratio'][0]:.3f} q at modulus {worst['ratio'][1][0]}")
    return 128 - lg
