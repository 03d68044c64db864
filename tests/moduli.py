"""NTT moduli off the prime table: the places in an octave where hehub's lazy fold (ntt.cpp:171-175, :215-219) and the engine's
bound reasoning about it change behaviour.  Every table prime (P40, P50, C3, C5) sits just below a power of two (fix = 0, tiny
delta); these families vary exactly what the table does not.

For a prime q, kb = round(log2 q), fix = (q >= 2^kb), delta = |q - 2^kb|.  Positions in the octave [2^k, 2^(k+1)):
  below     just under 2^k                      fix = 0, tiny delta (like the table)
  above     2^k + the first admissible step     fix = 1, tiny delta
  low_mid   about 1.05, 1.1, 1.3 times 2^k      fix = 1, large delta: hehub's fold wraps for large lazy words, from some N on
  high_mid  about 1.6 times 2^k                 kb = k + 1, fix = 0, large delta: no wrap, but lazy words reach 2q and more

Plain Python (the engine's decisions mirrored from hehub_amd/csrc/hp_tables.cpp: lazy_fold_bound, level_a_modulus, and
hp_api_scheme.cpp: spread_pack_mask)."""
import math

import params as P

LOGN_MAX = 16
WIDTHS = (17, 20, 30, 36, 40, 41, 44, 45, 46, 47, 48, 49, 50, 51, 55, 58, 59)
LOW_MID = (1.05, 1.1, 1.3)
HIGH_MID = 1.6


def step_bits(k):
    """primes of width k are drawn q = 1 (mod 2^step_bits): ring degrees up to 2^(step_bits - 1); narrow octaves get a smaller
    step so that the positions can still be hit"""
    return min(LOGN_MAX + 1, k - 6)


def prime_at(target, bits, up=True):
    """the first prime q = 1 (mod 2^bits) at or above (up) / below (not up) `target`"""
    step = 1 << bits
    q = (target // step) * step + 1
    if up and q < target:
        q += step
    if not up and q >= target:
        q -= step
    while not P.is_prime(q):
        q += step if up else -step
    return q


def log_modulus(q):
    return int(math.log2(float(q)) + 0.5)      # ntt.cpp:170 (u64)(log2(modulus) + 0.5)


def fold_consts(q):
    kb = log_modulus(q)
    fix = 1 if q >= (1 << kb) else 0
    return kb, fix, abs(q - (1 << kb))


def max_logn(q):
    """the largest logN with 2N | q - 1 (capped at LOGN_MAX)"""
    t = ((q - 1) & -(q - 1)).bit_length() - 1
    return min(LOGN_MAX, t - 1)


def family(k):
    """{position name: prime} for width k; low_mid names carry their factor (low_mid_1.1)"""
    if k == 17:
        return {"above": 65537}
    b, base = step_bits(k), 1 << k
    out = {"below": prime_at(base, b, up=False), "above": prime_at(base, b)}
    for f in LOW_MID:
        out[f"low_mid_{f}"] = prime_at(int(f * base), b)
    q = prime_at(int(HIGH_MID * base), b)
    if log_modulus(q) <= 59:                    # (1.6 * 2^59 rounds to 60 bits: the ABI refuses it)
        out["high_mid"] = q
    return out


FAMILIES = {k: family(k) for k in WIDTHS}
ALL = sorted({q for fam in FAMILIES.values() for q in fam.values()})


# ---- the engine's decisions --------------------------------------------------------------------------------------------------

def fold_bound(q, x_in, logn):
    """hp::lazy_fold_bound: (wraps, m_max * delta, word_end) for input words below x_in.  Each of the logn stages raises the largest
    word by less than 2q, the fold sees x < x_in + 2q logn, m = x >> kb <= m_max; the folded word is (x mod 2^kb) + m delta for
    fix = 0 and (x mod 2^kb) + q - m delta for fix = 1."""
    kb, fix, delta = fold_consts(q)
    x_end = x_in + 2 * q * logn
    m_delta = ((x_end - 1) >> kb) * delta
    wraps = x_end > (1 << 64) or (fix == 1 and m_delta >= (1 << kb))
    return wraps, m_delta, ((1 << kb) + q) if fix else ((1 << kb) + m_delta)


def pack48(q, cmax, logn):
    """spread_pack_mask's per-limb rule (the context's switches and the tiled-degree / batch >= 2 preconditions aside): the digit
    rows of output modulus q (strict coefficient rows below cmax transformed) may travel as 48-bit words"""
    kb = log_modulus(q)
    return 20 <= kb <= 46 and fold_bound(q, cmax, logn)[1] < (1 << kb)


def hehub_fold_exact(q, cmax, logn):
    """hp::level_a_modulus, the level-A predicate: for every input a pipeline of the chain hands hehub's transform -- a lazy word
    (< 2q) or a strict row of another modulus (< cmax) -- the fold does not wrap, and the forward words of a lazy input (words hehub
    hands back to its caller) stay below 2q"""
    return not fold_bound(q, max(2 * q, cmax), logn)[0] and fold_bound(q, 2 * q, logn)[2] <= 2 * q


def level_a_chain(mext, logn):
    """ensure_plan_a: the chain runs at level A (ring degree with tiled kernels, every q < 2^50 and level_a_modulus)"""
    cmax = max(mext)
    return 11 <= logn <= 15 and all(3 <= q < (1 << 50) and hehub_fold_exact(q, cmax, logn) for q in mext)


# ---- named chains (q_0 .. q_{L-1}, p), every modulus = 1 (mod 2^16): usable up to N = 2^15 -----------------------------------

def _chain_prime(target, up=True):
    return prime_at(target, LOGN_MAX, up)


Q59 = P.ntt_primes(1, 15, 59)[0]
# a 59-bit q0 in front of nine table 40-bit limbs and a 50-bit p: spread_pack_mask packs P40[0] and leaves P40[1..8] plain
W59 = [Q59] + P.P40[:9] + [P.P50[0]]
# narrow limbs (20 and 30 bits) and a 59-bit special prime
NARROW = [_chain_prime(1 << 20, up=False), _chain_prime(1 << 20), _chain_prime(1 << 30, up=False), _chain_prime(1 << 30),
          P.ntt_primes(1, 15, 59, exclude=(Q59,))[0]]
# 46-, 47- and 48-bit limbs, each just below and just above 2^k, behind a wide q0: only kb <= 46 may be packed
PACKEDGE = [Q59] + [_chain_prime(1 << k, up) for k in (46, 47, 48) for up in (False, True)] + [P.P50[0]]
# every limb 2^k + small (fix = 1, tiny delta)
ABOVE = [_chain_prime(1 << k) for k in (44, 40, 41, 45, 49)]
# one low_mid limb of about 1.1 * 2^40 among P40s: kb = 40, its fold wraps from N = 4096 on
LOWMID_Q = _chain_prime(int(1.1 * (1 << 40)))
LOWMID = P.P40[:2] + [LOWMID_Q] + P.P40[2:4] + [P.P40[4]]
# a prime just above 2^50 (level A serves q < 2^50 only)
OVER50 = P.P40[:3] + [_chain_prime(1 << 50)]
# primes just below and just above 2^40 (the 40-bit digit-row format of level A)
PACK40EDGE = [_chain_prime(1 << 40, up=False), _chain_prime(1 << 40), P.P40[1], P.P50[0]]
# a chain with high_mid limbs (kb = k + 1, large delta): lazy words reach 2q and more
HIGHMID = [_chain_prime(int(HIGH_MID * (1 << 40))), P.P40[0], _chain_prime(int(HIGH_MID * (1 << 44))), P.P50[0]]

CHAINS = {"W59": W59, "NARROW": NARROW, "PACKEDGE": PACKEDGE, "ABOVE": ABOVE, "LOWMID": LOWMID, "OVER50": OVER50,
          "PACK40EDGE": PACK40EDGE, "HIGHMID": HIGHMID}


# ---- inputs and an independent exact reference --------------------------------------------------------------------------------

INPUT_KINDS = ("strict", "lazy", "max", "alt")


def edge_words(rng, kind, q, n):
    """one row of input words: uniform strict, uniform lazy (< 2q), all 2q - 1, or 2q - 1 / 0 alternating"""
    import numpy as np

    if kind == "strict":
        return rng.words(n, q)
    if kind == "lazy":
        return rng.words(n, 2 * q)
    x = np.full(n, 2 * q - 1, dtype=np.uint64)
    if kind == "alt":
        x[1::2] = 0
    return x


def lazy_rows(rng, shape, moduli):
    """[..., L, n] words as a chained hehub call hands them in: uniform strict words, a block of words in [q, 2q) and some 2q - 1"""
    import numpy as np

    x = rng.poly(shape, moduli)
    q = np.array(moduli, dtype=np.uint64)[:, None]
    n = shape[-1]
    x[..., : max(1, n // 4)] += q
    x[..., 1::7] = 2 * q - np.uint64(1)
    return x


def negacyclic_product(a, b, q):
    """a b mod (X^N + 1, q) with Python integers by Kronecker substitution: each coefficient (< 2^64) in a 192-bit slot, one big
    product, the top half folded back with a minus sign.  Exact; about a second at N = 2^15."""
    import numpy as np

    n, slot = len(a), 3

    def pack(v):
        buf = np.zeros((n, slot), dtype=np.uint64)
        buf[:, 0] = v
        return int.from_bytes(buf.tobytes(), "little")

    c = pack(np.asarray(a, dtype=np.uint64) % np.uint64(q)) * pack(np.asarray(b, dtype=np.uint64) % np.uint64(q))
    w = np.frombuffer(c.to_bytes(2 * n * slot * 8, "little"), dtype=np.uint64).reshape(2 * n, slot)
    v = [int(x) | (int(y) << 64) | (int(z) << 128) for x, y, z in w]
    return np.array([(v[i] - v[i + n]) % q for i in range(n)], dtype=np.uint64)
