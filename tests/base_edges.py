"""Planted inputs for the RNS base transforms (hp_edge.hip: k_base_from_single, k_base_to_single, k_base_to_single_crt), built from
Python integers: the values at which the centring compare x < half, the small-coefficient consistency check and the lexicographic
comparison of the mixed-radix digits with floor(Q / 2) change sides.  tests/test_drop_edges.py runs them oracle against reference
without a GPU, tests/test_gpu_base_edges.py engine against oracle."""
import numpy as np

import moduli as M
import params as P

U = np.uint64
T17 = 65537
Q20 = M.NARROW[0]


def product(mods):
    out = 1
    for q in mods:
        out *= q
    return out


def crt_value(res, mods):
    Q = product(mods)
    return sum(int(r) * (Q // q) * pow(Q // q, -1, q) for r, q in zip(res, mods)) % Q


def single_of(v, Q, t):
    """rns_base_transform to one modulus, CRT branch: x mod t below floor(Q / 2), t - ((Q - x) mod t) from there on (t itself, not 0,
    where t divides Q - x)"""
    return v % t if v < Q // 2 else t - ((Q - v) % t)


# ---- one modulus -> many ------------------------------------------------------------------------------------------------------------
FROM_SINGLE = [
    (P.P50[0], [P.P40[0], P.P40[1]]),        # old > q
    (P.P40[0], [P.P50[0], P.P50[1]]),        # old < q
    (T17, [M.Q59, P.P40[0]]),                # a 17-bit old modulus under a 59-bit new one
    (M.Q59, [Q20, T17]),                     # a 59-bit old modulus over a 20-bit new one
    (2, [P.P40[0], T17, M.Q59]),
]


def from_single_values(old):
    h = old // 2
    strict = [0, max(h - 1, 0), h, old - 1]
    return strict + [v + old for v in strict]          # the same, lazy: up to 2 old - 1


def from_single_cases(n):
    """(old, new moduli, x [n]): the edge words in turn, from a different one in each eighth of the row"""
    out = []
    for old, new in FROM_SINGLE:
        vals = np.array(from_single_values(old), dtype=U)
        i = np.arange(n)
        out.append((old, new, vals[(i + i // max(n // 8, 8)) % len(vals)]))
    return out


# ---- many -> one: the small-coefficient branch at its boundary -----------------------------------------------------------------------
CHAIN16 = P.P40 + P.P50 + [T17, Q20]           # HP_CRT_MAX_LIMBS old moduli (pairwise coprime: distinct primes)
CHAIN17 = CHAIN16 + [P.NTT_TEST_Q[1]]
SMALL = {
    "P40x3": (P.P40[:3], T17),
    "narrow_first": ([T17, P.P50[0]], P.P40[0]),       # a 17-bit and a 50-bit modulus: the half of limb 0 is the small one
    "wide_first": ([P.P50[0], T17], P.P40[0]),         # ... and the large one: min(q) / 2 is far below limb 0's half
    "sixteen": (CHAIN16, T17),
}


def special_index(p, n):
    return (n // 2 + 3 * p) % n


def small_signed(old):
    """the six planted coefficients, one per polynomial: magnitude m - 1, m, m + 1 for m = min(q) // 2, positive then negative"""
    m = min(old) // 2
    return [m - 1, m, m + 1, -(m - 1), -m, -(m + 1)]


def small_cases(n):
    """(name, old moduli, new modulus, x [6][L][n]): small random polynomials (|coefficient| < 1000, params.small_rns_poly) with one
    planted coefficient each, and one lazy word on limb 0"""
    from oracle.pyoracle import SplitMix

    out = []
    for name, (old, new) in SMALL.items():
        rng = SplitMix(6200 + n + len(old))
        x = np.stack([P.small_rns_poly(rng, n, old) for _ in range(6)])
        for p, s in enumerate(small_signed(old)):
            x[p, :, special_index(p, n)] = [s % q for q in old]
        x[:, 0, 1] += U(old[0])
        out.append((name, old, new, x))
    return out


# ---- many -> one: the CRT branch around floor(Q / 2) ---------------------------------------------------------------------------------
CRT = {
    "P40x3": (P.P40[:3], T17),
    "P40x5_t257": (P.P40[:5], 257),
    "with59": ([M.Q59, P.P40[0], P.P50[0]], T17),
    "with59_t50": ([P.P40[1], M.Q59], P.P50[2]),
}


def crt_values(old, t):
    Q = product(old)
    return [0, 1, Q // 2 - 1, Q // 2, Q // 2 + 1, Q - 1, Q - t, Q - 2 * t]


def crt_cases(n):
    """(name, old moduli, new modulus, x [2][L][n], expected [n]): the values in turn as strict residues, and the same polynomial once
    more with + q_0 on every word of limb 0"""
    out = []
    for name, (old, t) in CRT.items():
        Q, vals = product(old), crt_values(old, t)
        turn = np.arange(n) % len(vals)
        strict = np.array([[v % q for v in vals] for q in old], dtype=U)[:, turn]
        lazy = strict.copy()
        lazy[0] += U(old[0])
        want = np.array([single_of(v, Q, t) for v in vals], dtype=U)[turn]
        out.append((name, old, t, np.stack([strict, lazy]), want))
    return out
