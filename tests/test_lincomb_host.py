"""hpi::lincomb_max_terms (hp_drop.cpp): how many terms one launch of k_ct_lincomb (hp_lincomb.hip) may sum before the high word of
its 128-bit accumulators leaves the range of the Montgomery step.  Below 2^60.9 the answer is the whole table
(tests/test_gpu_lincomb.py plants the largest sum at a 59-bit modulus); the shorter tables and the refusal start above, where only
this test reaches (CPU tier, through tests/cpp/lincomb_shim.cpp, built with g++).  Checked against the documented formula in Python
integers AND against the property it exists for: with operand words up to 2q - 1, coefficients up to q - 1, the constant (below q)
and an accumulated word (below 2q) on top, R terms sum to at most R (q - 1)(2q - 1) + 3q, and hp_montgomery128_lazy returns
hi + mulhi(u, q) + 1 in a 64-bit word, mulhi(u, q) <= q - 1: the sum must stay at most (2^64 - q) 2^64 - 1."""
import ctypes as C
import os
import subprocess

import pytest

import moduli as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "cpp", "liblincomb_shim.so")
CSRC = os.path.join(ROOT, "hehub_amd", "csrc")
TABLE = 32   # HP_LINCOMB_MAX


@pytest.fixture(scope="module")
def lc():
    src = [os.path.join(ROOT, "tests", "cpp", "lincomb_shim.cpp"), os.path.join(CSRC, "hp_drop.cpp"), os.path.join(CSRC, "hp_tables.cpp")]
    dep = src + [os.path.join(CSRC, "hp_drop.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in dep):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO] + src, check=True)
    lib = C.CDLL(SO)
    lib.lc_max_terms.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t]
    lib.lc_max_terms.restype = C.c_size_t
    return lambda moduli, table=TABLE: lib.lc_max_terms((C.c_uint64 * len(moduli))(*moduli), len(moduli), table)


def montgomery_limit(q):
    """the largest 128-bit sum whose Montgomery word hi + mulhi(u, q) + 1 still fits 64 bits for every u"""
    return ((1 << 64) - q) * (1 << 64) - 1


def worst_sum(q, R):
    """R terms of the largest word times the largest coefficient, the largest constant, the largest accumulated word"""
    return R * (q - 1) * (2 * q - 1) + (q - 1) + (2 * q - 1)


def formula(q, table):
    if q < 2 or q >= 1 << 62:
        return 0
    return min(table, (montgomery_limit(q) - 3 * q) // ((q - 1) * (2 * q - 1)))


Q50 = (1 << 50) - 27


@pytest.mark.parametrize("q", [Q50, M.Q59, 1 << 60, (1 << 61) - 1, (1 << 62) - 57, 1 << 62, 1, 0], ids=lambda q: f"{q.bit_length()}b_{q}")
def test_max_terms_at_the_moduli_no_gpu_test_reaches(lc, q):
    got = lc([3, q, 5] if q > 5 else [q])
    exp = formula(q, TABLE)
    print(q.bit_length(), got, formula(q, 1 << 40))
    assert got == exp
    if got:
        assert worst_sum(q, got) <= montgomery_limit(q)
    uncapped = lc([q], 1 << 40)
    if uncapped:   # the answer without the table: one more term may leave the range (the formula's 3q covers q - 1 + 2q - 1 with 2 to spare)
        assert worst_sum(q, uncapped) <= montgomery_limit(q) < worst_sum(q, uncapped + 1) + 2


def test_what_the_documents_say(lc):
    """the whole table for every modulus below 2^60.9; 28 terms at q = 2^61 - 1, 6 just below 2^62; nothing from 2^62 on"""
    assert formula(int(2 ** 60.9), TABLE) == TABLE == lc([int(2 ** 60.9)])
    assert formula((1 << 61) - 1, TABLE) == 28 == lc([(1 << 61) - 1])
    assert lc([(1 << 62) - 57]) == 6 and lc([1 << 62]) == 0 and lc([(1 << 64) - 59]) == 0


def test_largest_modulus_of_the_chain_decides_and_the_table_caps(lc):
    big, small = (1 << 61) - 1, (1 << 40) - 87
    assert lc([small, big]) == lc([big, small, small]) == formula(big, TABLE) < TABLE
    assert lc([small]) == TABLE and lc([small], 7) == 7
    assert lc([small, 0]) == TABLE and lc([0]) == 0 and lc([1]) == 0
