"""hpi::tensor_sum_max_terms (hp_drop.cpp): how many terms one launch of k_tensor_sum (hp_ks.hip) may sum before the high word of its
128-bit accumulators leaves the range of the Montgomery step.  Every modulus the transforms accept is below 2^59.5, where the answer
is the whole table (tests/test_gpu_tensor_sum.py plants the largest sum there); the shorter tables and the refusal start at 2^60, which
only this test reaches (CPU tier, through tests/cpp/tensor_sum_shim.cpp, built with g++).  Checked against the documented formula in
Python integers AND against the property it exists for: with operand words up to 2q - 1 and the d1 column's two products per term, R
terms sum to at most 2 R (2q - 1)^2, and hp_montgomery128_lazy returns hi + mulhi(u, q) + 1 in a 64-bit word, mulhi(u, q) <= q - 1:
the sum must stay at most (2^64 - q) 2^64 - 1."""
import ctypes as C
import os
import subprocess

import pytest

import moduli as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "cpp", "libtensor_sum_shim.so")
CSRC = os.path.join(ROOT, "hehub_amd", "csrc")
TABLE = 32   # HP_TENSOR_SUM_MAX


@pytest.fixture(scope="module")
def ts():
    src = [os.path.join(ROOT, "tests", "cpp", "tensor_sum_shim.cpp"), os.path.join(CSRC, "hp_drop.cpp"), os.path.join(CSRC, "hp_tables.cpp")]
    dep = src + [os.path.join(CSRC, "hp_drop.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in dep):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO] + src, check=True)
    lib = C.CDLL(SO)
    lib.ts_max_terms.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t]
    lib.ts_max_terms.restype = C.c_size_t
    return lambda moduli, table=TABLE: lib.ts_max_terms((C.c_uint64 * len(moduli))(*moduli), len(moduli), table)


def montgomery_limit(q):
    """the largest 128-bit sum whose Montgomery word hi + mulhi(u, q) + 1 still fits 64 bits for every u"""
    return ((1 << 64) - q) * (1 << 64) - 1


def formula(q, table):
    if q == 0 or q >= 1 << 62:
        return 0
    return min(table, montgomery_limit(q) // (2 * (2 * q - 1) ** 2))


def worst_sum(q, R):
    return 2 * R * (2 * q - 1) ** 2


Q50 = (1 << 50) - 27


@pytest.mark.parametrize("q", [Q50, M.Q59, 1 << 60, (1 << 61) - 1, (1 << 62) - 57, 1 << 62, 0], ids=lambda q: f"{q.bit_length()}b_{q}")
def test_max_terms_at_the_moduli_no_gpu_test_reaches(ts, q):
    got = ts([3, q, 5] if q else [0])
    exp = formula(q, TABLE)
    print(q.bit_length(), got, formula(q, 1 << 40))
    assert got == exp
    if got:
        assert worst_sum(q, got) <= montgomery_limit(q)
        if got < TABLE:   # (where the table capped the answer a longer sum may still fit)
            assert worst_sum(q, got + 1) > montgomery_limit(q)


def test_what_the_documents_say(ts):
    """the whole table for every modulus the transforms accept (below 2^59.5); 30 terms at q = 2^60; nothing from 2^62 on"""
    assert formula(int(2 ** 59.5), TABLE) == TABLE == ts([int(2 ** 59.5)])
    assert formula(1 << 60, TABLE) == 30 == ts([1 << 60])
    assert ts([(1 << 62) - 57]) >= 1 and ts([1 << 62]) == 0 and ts([(1 << 64) - 59]) == 0


def test_largest_modulus_of_the_chain_decides_and_the_table_caps(ts):
    big, small = 1 << 60, (1 << 40) - 87
    assert ts([small, big]) == ts([big, small, small]) == formula(big, TABLE)
    assert ts([small]) == TABLE and ts([small], 7) == 7
    assert ts([small, 0]) == TABLE and ts([0]) == 0
