"""hpi::hks_lintrans_max_rotations (hp_drop.cpp): how many rotations one launch of k_hks_inner_lintrans may sum before its 128-bit
accumulators could wrap.  Every modulus the transforms accept is below 2^59.5, where the answer is the whole table
(tests/test_gpu_hks_moduli.py runs it at 58 and 59 bits, tests/test_hks_edges.py has the sums); the smaller tables and the
refusal start near 2^60, which only this test reaches (CPU tier, through tests/cpp/lintrans_shim.cpp, built with g++).  Checked against
the documented formula in Python integers AND against the property it exists for, with the largest words of the formula's premise
(digit words below 2q; the lifted rows at level B can exceed that -- tests/test_hks_edges.py measures what they reach and that the
sums fit all the same)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "cpp", "liblintrans_shim.so")
CSRC = os.path.join(ROOT, "hehub_amd", "csrc")
TABLE = 32   # HP_HOIST_TABLE_MAX


@pytest.fixture(scope="module")
def ls():
    src = [os.path.join(ROOT, "tests", "cpp", "lintrans_shim.cpp"), os.path.join(CSRC, "hp_drop.cpp"), os.path.join(CSRC, "hp_tables.cpp")]
    dep = src + [os.path.join(CSRC, "hp_drop.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in dep):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO] + src, check=True)
    lib = C.CDLL(SO)
    lib.ls_max_rotations.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t]
    lib.ls_max_rotations.restype = C.c_size_t
    return lambda mext, nd, table=TABLE: lib.ls_max_rotations((C.c_uint64 * len(mext))(*mext), len(mext), nd, table)


def formula(q, nd, table):
    if q == 0 or q >= 1 << 62:
        return 0
    w = 4 * nd * ((q * q >> 64) + 1) + 3 * q
    if w >= 1 << 64:
        return 0
    return min(table, ((1 << 128) - 1) // (w * 2 * q))


def worst_sum(q, nd, R):
    """the largest value R rotations can put into the outer accumulator: digit and key words up to 2q - 1, the Montgomery reduction
    adding less than q, the folded c0 word up to 2q - 1, the diagonal word up to 2q - 1"""
    word = (nd * (2 * q - 1) ** 2 >> 64) + q + (2 * q - 1)
    assert word < 1 << 64
    return R * word * (2 * q - 1)


@pytest.mark.parametrize("q,nd,expect", [
    ((1 << 50) - 27, 16, 32),     # the moduli of the GPU tests: the whole table
    ((1 << 59) - 55, 16, 32),     # still the whole table
    (1 << 60, 16, 18),            # the first shorter tables
    (1 << 60, 4, 31),
    ((1 << 61) - 1, 1, 9),
    ((1 << 61) - 1, 16, 0),       # one rotation's word no longer fits 64 bits
    ((1 << 62) - 57, 1, 2),
    (1 << 62, 1, 0),              # 2q needs the room
])
def test_max_rotations_at_the_moduli_no_gpu_test_reaches(ls, q, nd, expect):
    got = ls([3, q, 5], nd)
    print(q.bit_length(), nd, got)
    assert got == formula(q, nd, TABLE) == expect
    if got:
        assert worst_sum(q, nd, got) < 1 << 128


def test_largest_modulus_of_the_chain_decides_and_the_table_caps(ls):
    big, small = 1 << 60, (1 << 40) - 87
    assert ls([small, big], 16) == ls([big, small, small], 16) == formula(big, 16, TABLE)
    assert ls([small], 16) == TABLE and ls([small], 16, 7) == 7
    assert ls([0], 1) == 0
