"""Host-side logic of the BFV calls without a GPU (hehub_amd/csrc/hp_bfv.h through tests/cpp/bfv_shim.cpp): the exact base-size
decision B >= 4 t N Q -- multiword integers, one below and at the bound -- and every constant the kernels read, against Python
integers: Garner inverses, the digits of floor(X/2), prefix products, Q^-1 mod b_j, h mod every modulus, and the t-dependent words.
59-bit moduli and L = M = 16 included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bfv_model as F
import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "cpp", "libbfv_shim.so")
HDR = os.path.join(ROOT, "hehub_amd", "csrc", "hp_bfv.h")
MX = 16
P59 = P.ntt_primes(32, 4, 59)
CASES = {
    "small": (P.P40[:2], P.P40[2:5]),
    "width1": (P.P40[:1], P.P40[1:3]),
    "mixed": (P.P40[:4], P.P50[:4]),
    "wide": (P.P40[:8], P.P40[8:10] + P.P50[:4] + F.EXTRA40),
    "full59": (P59[:16], P59[16:]),
}


@pytest.fixture(scope="module")
def bs():
    src = os.path.join(ROOT, "tests", "cpp", "bfv_shim.cpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", SO, src], check=True)
    lib = C.CDLL(SO)
    u, z, p = C.c_uint64, C.c_size_t, C.c_void_p
    lib.bs_base_ok.argtypes = [p, z, z, u, u]
    lib.bs_consts.argtypes = [p, z, z, p]
    lib.bs_plain.argtypes = [p, z, u, p]
    lib.bs_dec_plain.argtypes = [p, z, u, p]
    lib.bs_inverse.argtypes, lib.bs_inverse.restype = [u, u], u
    for f in (lib.bs_consts_words, lib.bs_plain_words, lib.bs_dec_words):
        f.restype = z
    assert lib.bs_max() == MX
    assert (lib.bs_consts_words(), lib.bs_plain_words(), lib.bs_dec_words()) == (1 + 2 * (4 * MX * MX + 2 * MX) + 4 * MX, 4 * MX, 5 + 4 * MX)
    return lib


def arr(v):
    return np.array([int(x) for x in v], dtype=np.uint64)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def base_ok(bs, q, b, t, n):
    qb = arr(list(q) + list(b))
    return bool(bs.bs_base_ok(ptr(qb), len(q), len(b), t, n))


def harvey(v, q):
    return (v << 64) // q


def mixed_radix(x, moduli):
    digits = []
    for m in moduli:
        digits.append(x % m)
        x //= m
    assert x == 0
    return digits


def check_base(words, x, y):
    """one HpBfvBase block (inv, inv_h, half, pref, pref_h, prod) for the conversion from the moduli x into the moduli y"""
    sq = MX * MX
    inv, inv_h = words[:sq].reshape(MX, MX), words[sq:2 * sq].reshape(MX, MX)
    half = words[2 * sq:2 * sq + MX]
    pref, pref_h = words[2 * sq + MX:3 * sq + MX].reshape(MX, MX), words[3 * sq + MX:4 * sq + MX].reshape(MX, MX)
    prod = words[4 * sq + MX:4 * sq + 2 * MX]
    X = F.prod(x)
    for a in range(MX):
        for c in range(MX):
            if c < a < len(x):
                assert int(inv[c][a]) == pow(x[c], -1, x[a]) and int(inv_h[c][a]) == harvey(int(inv[c][a]), x[a]), (c, a)
            else:
                assert inv[c][a] == 0 and inv_h[c][a] == 0
    assert [int(w) for w in half] == mixed_radix(X // 2, x) + [0] * (MX - len(x))
    for m in range(MX):
        for a in range(MX):
            if m < len(y) and a < len(x):
                assert int(pref[m][a]) == F.prod(x[:a]) % y[m] and int(pref_h[m][a]) == harvey(int(pref[m][a]), y[m]), (m, a)
            else:
                assert pref[m][a] == 0 and pref_h[m][a] == 0
        assert int(prod[m]) == (X % y[m] if m < len(y) else 0)


@pytest.mark.parametrize("name", CASES)
def test_chain_constants_against_python_integers(bs, name):
    q, b = CASES[name]
    L, M = len(q), len(b)
    out = np.zeros(bs.bs_consts_words(), dtype=np.uint64)
    assert bs.bs_consts(ptr(arr(q + b)), L, M, ptr(out)) == 1
    assert int(out[0]) == L | (M << 32)
    blk = 4 * MX * MX + 2 * MX
    check_base(out[1:1 + blk], q, b)
    check_base(out[1 + blk:1 + 2 * blk], b, q)
    rest = out[1 + 2 * blk:]
    Q = F.prod(q)
    h = (Q - 1) // 2
    for j in range(MX):
        want = pow(Q, -1, b[j]) if j < M else 0
        assert int(rest[j]) == want and int(rest[MX + j]) == (harvey(want, b[j]) if j < M else 0), j
    assert [int(w) for w in rest[2 * MX:]] == [h % m for m in q + b] + [0] * (2 * MX - L - M)
    # decryption reads the same block with no auxiliary base
    dec = np.zeros(bs.bs_consts_words(), dtype=np.uint64)
    assert bs.bs_consts(ptr(arr(q)), L, 0, ptr(dec)) == 1
    assert np.array_equal(dec[1:1 + 2 * MX * MX + MX], out[1:1 + 2 * MX * MX + MX]) and int(dec[0]) == L   # inv, inv_h, half of Q
    assert [int(w) for w in dec[1 + 2 * blk + 2 * MX:]] == [h % m for m in q] + [0] * (2 * MX - L)


def test_moduli_that_share_a_factor_are_refused(bs):
    out = np.zeros(bs.bs_consts_words(), dtype=np.uint64)
    assert bs.bs_consts(ptr(arr([15, 21, 1099510054913])), 2, 1, ptr(out)) == 0        # inside Q
    assert bs.bs_consts(ptr(arr([15, 1099510054913, 21])), 2, 1, ptr(out)) == 0        # Q against b_j
    assert bs.bs_inverse(3, 7) == 5 and bs.bs_inverse(6, 9) == 0 and bs.bs_inverse(1, 2) == 1


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("t", [2, 65537, 2147483647, 6])
def test_plain_modulus_words(bs, name, t):
    q, b = CASES[name]
    qb = q + b
    out = np.zeros(bs.bs_plain_words(), dtype=np.uint64)
    bs.bs_plain(ptr(arr(qb)), len(qb), t, ptr(out))
    pad = [0] * (2 * MX - len(qb))
    assert [int(w) for w in out[:2 * MX]] == [t % m for m in qb] + pad
    assert [int(w) for w in out[2 * MX:]] == [harvey(t % m, m) for m in qb] + pad
    dec = np.zeros(bs.bs_dec_words(), dtype=np.uint64)
    assert bs.bs_dec_plain(ptr(arr(q)), len(q), t, ptr(dec)) == 1
    Q, padq = F.prod(q), [0] * (MX - len(q))
    assert int(dec[0]) == t and int(dec[1]) == ((1 << 64) - 1) // t
    rows = dec[2:2 + 4 * MX].reshape(4, MX)
    assert [int(w) for w in rows[0]] == [t % m for m in q] + padq and [int(w) for w in rows[1]] == [harvey(t % m, m) for m in q] + padq
    assert [int(w) for w in rows[2]] == [F.prod(q[:a]) % t for a in range(len(q))] + padq
    assert [int(w) for w in rows[3]] == [harvey(F.prod(q[:a]) % t, t) for a in range(len(q))] + padq
    qinv = pow(Q, -1, t)
    assert [int(w) for w in dec[2 + 4 * MX:]] == [((Q - 1) // 2) % t, qinv, harvey(qinv, t)]


def test_a_plain_modulus_that_divides_into_q_is_refused(bs):
    dec = np.zeros(bs.bs_dec_words(), dtype=np.uint64)
    assert bs.bs_dec_plain(ptr(arr([15, 77])), 2, 6, ptr(dec)) == 0
    assert bs.bs_dec_plain(ptr(arr([15, 77])), 2, 4, ptr(dec)) == 1


def test_base_size_decision_at_and_one_below_the_bound(bs):
    """base_ok takes any words (the primality of the moduli is the caller's business), so the bound can be met exactly"""
    q0 = P.P40[0]
    # one word: t = 2, N = 8, B = 64 q0 against 64 q0 - 1
    assert base_ok(bs, [q0], [64 * q0], 2, 8) and not base_ok(bs, [q0], [64 * q0 - 1], 2, 8) and base_ok(bs, [q0], [64 * q0 + 1], 2, 8)
    # several words: Q = 2^90, 4 t N = 64, B = 2^96 against 2^96 - 1 = (2^48 - 1)(2^48 + 1)
    q = [1 << 45, 1 << 45]
    assert base_ok(bs, q, [1 << 48, 1 << 48], 2, 8) and not base_ok(bs, q, [(1 << 48) - 1, (1 << 48) + 1], 2, 8)
    assert base_ok(bs, q, [1 << 32, 1 << 32, 1 << 32], 2, 8) and not base_ok(bs, q, [1 << 32, 1 << 32, (1 << 32) - 1], 2, 8)
    assert not base_ok(bs, q, [1 << 48, 1 << 48], 2, 16) and not base_ok(bs, q, [1 << 48, 1 << 48], 3, 8)
    # equality through the moduli themselves: B = 64 * q0 * q1
    q = P.P40[:2]
    assert base_ok(bs, q, [64] + q, 2, 8) and not base_ok(bs, q, [63] + q, 2, 8) and base_ok(bs, q, [32] + q, 2, 4)


@pytest.mark.parametrize("name", CASES)
def test_base_size_decision_against_python_integers(bs, name):
    q, b = CASES[name]
    for t in (2, 65537, 2147483647, (1 << 39) - 7):
        for logn in (3, 4, 11, 16):
            for M in range(1, len(b) + 1):
                assert base_ok(bs, q, b[:M], t, 1 << logn) == F.base_ok(q + b[:M], len(q), t, 1 << logn), (t, logn, M)
    # L = M = 16 at 59 bits: 944-bit products on both sides; every subset size of the auxiliary base
    if name == "full59":
        assert base_ok(bs, q, b, 65537, 1 << 16) is False and base_ok(bs, q[:12], b, 65537, 1 << 16) is True
