"""hpi::hks_bsgs_plan (hp_drop.cpp): the pass plan and the workspace of hp_dev_ckks_lintrans_bsgs_hks, against the formula documented
in hp_drop.h written with Python integers (CPU tier, through tests/cpp/bsgs_shim.cpp, built with g++).  The babies per pre-sum pass
are hks_lintrans_max_rotations' answer: the whole table for every modulus of the GPU tests, shorter near 2^60, which only this test
reaches.  The plan is a function of the shape alone: it has no argument through which steps or absent diagonals could enter."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "cpp", "libbsgs_shim.so")
CSRC = os.path.join(ROOT, "hehub_amd", "csrc")
TABLE, GIANT_MAX, DIAG_MAX = 32, 32, 256   # HP_BSGS_TABLE_MAX (== HP_HOIST_TABLE_MAX), HP_BSGS_GIANT_MAX, HP_BSGS_DIAG_MAX


@pytest.fixture(scope="module")
def plan():
    src = [os.path.join(ROOT, "tests", "cpp", "bsgs_shim.cpp"), os.path.join(CSRC, "hp_drop.cpp"), os.path.join(CSRC, "hp_tables.cpp")]
    dep = src + [os.path.join(CSRC, "hp_drop.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in dep):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO] + src, check=True)
    lib = C.CDLL(SO)
    lib.bs_plan.argtypes = [C.c_void_p] + [C.c_size_t] * 7 + [C.c_void_p]
    lib.bs_plan.restype = C.c_int

    def call(mext, n, L, k, alpha, batch, babies, giants):
        assert len(mext) == L + k
        out = (C.c_size_t * 5)()
        ok = lib.bs_plan((C.c_uint64 * len(mext))(*mext), n, L, k, alpha, batch, babies, giants, out)
        return bool(ok), dict(zip(("baby_pass", "giant_pass", "presum_giants", "overlay_words", "words"), out))
    return call


def max_rotations(q, nd, table):
    """tests/test_lintrans_host.py pins hks_lintrans_max_rotations to this"""
    if q == 0 or q >= 1 << 62:
        return 0
    w = 4 * nd * ((q * q >> 64) + 1) + 3 * q
    if w >= 1 << 64:
        return 0
    return min(table, ((1 << 128) - 1) // (w * 2 * q))


def formula(mext, n, L, k, alpha, B, babies, G):
    E, nd = L + k, -(-L // alpha)
    cap = max_rotations(max(mext), nd, TABLE)
    if cap == 0 or babies == 0 or G == 0:
        return None

    def pad(words):
        return -(-words * 8 // 256) * 256 // 8

    baby_pass = min(cap, babies)
    overlay = max(pad(B * L * n) + pad(B * nd * E * n) + pad(B * babies * 2 * E * n), pad(B * G * L * n) + pad(B * G * nd * E * n))
    words = overlay + pad(B * 2 * E * n) + pad(B * G * 2 * E * n) + pad(2 * B * G * k * n) + pad(2 * B * G * L * n) + pad(B * G * 2 * L * n)
    return dict(baby_pass=baby_pass, giant_pass=min(G, TABLE), presum_giants=min(G, GIANT_MAX, DIAG_MAX // baby_pass),
                overlay_words=overlay, words=words)


SMALL = (1 << 40) - 87


@pytest.mark.parametrize("q,logn,L,k,alpha,B,babies,giants", [
    (SMALL, 15, 10, 4, 3, 1, 16, 16),        # the shape of DESIGN 4.7b
    (SMALL, 15, 10, 4, 3, 1, 8, 8),
    (SMALL, 4, 4, 2, 2, 1, 33, 2),           # babies past one table: the baby rows outweigh the giants' digit rows
    (SMALL, 4, 3, 1, 1, 2, 2, 34),           # giants past one table, and past one pre-sum launch: the digit rows outweigh
    (SMALL, 5, 5, 2, 2, 3, 3, 3),            # rows that need padding (3 * 5 * 32 words is no multiple of 32)
    (SMALL, 4, 1, 1, 1, 1, 1, 1),
    ((1 << 59) - 55, 11, 4, 2, 2, 2, 40, 40),  # still the whole table
    (1 << 60, 11, 16, 2, 1, 1, 40, 5),       # nd = 16: 18 babies per pass, 14 giants would fit a pre-sum launch
    (1 << 60, 11, 4, 2, 1, 1, 40, 40),       # nd = 4: 31
    ((1 << 61) - 1, 11, 1, 1, 1, 1, 20, 40),  # nd = 1: 9 babies per pass, 28 giants per pre-sum launch
    ((1 << 62) - 57, 11, 1, 1, 1, 1, 5, 40),  # 2: the pre-sum launch is capped by its 32 giants
])
def test_plan_is_the_documented_formula(plan, q, logn, L, k, alpha, B, babies, giants):
    mext = [SMALL] * (L + k)
    mext[L // 2] = q
    n = 1 << logn
    ok, got = plan(mext, n, L, k, alpha, B, babies, giants)
    exp = formula(mext, n, L, k, alpha, B, babies, giants)
    print(q.bit_length(), got)
    assert ok and got == exp
    # what the engine relies on: a launch's tables hold its share, and the overlay holds either occupant
    assert 1 <= got["baby_pass"] <= TABLE and 1 <= got["giant_pass"] <= TABLE
    assert 1 <= got["presum_giants"] <= GIANT_MAX and got["presum_giants"] * got["baby_pass"] <= DIAG_MAX
    assert got["overlay_words"] % 32 == 0 and got["words"] % 32 == 0 and got["words"] > got["overlay_words"]


def test_passes_shorten_near_2_to_the_60(plan):
    """the figures of tests/test_lintrans_host.py, reached through the plan"""
    for q, L, alpha, babies in (((1 << 60), 16, 1, 18), ((1 << 60), 4, 1, 31), ((1 << 61) - 1, 1, 1, 9), ((1 << 62) - 57, 1, 1, 2)):
        ok, got = plan([q] + [SMALL] * L, 16, L, 1, alpha, 1, 40, 3)
        assert ok and got["baby_pass"] == babies, (q, got)


def test_refusals(plan):
    mext = [SMALL] * 3
    assert not plan(mext, 16, 2, 1, 1, 1, 0, 2)[0] and not plan(mext, 16, 2, 1, 1, 1, 2, 0)[0]
    assert not plan([SMALL, 1 << 62, SMALL], 16, 2, 1, 1, 1, 2, 2)[0]                        # 2q needs the room
    assert not plan([(1 << 61) - 1] + [SMALL] * 16, 16, 16, 1, 1, 1, 2, 2)[0]                # 16 digits: one word no longer fits
    assert plan(mext, 16, 2, 1, 1, 1, 2, 2)[0]


def test_the_size_follows_the_shape_alone(plan):
    """(f) of the GPU tests on the CPU: the same shape twice is the same plan, and every argument of the shape moves the size"""
    base = ([SMALL] * 5, 2048, 3, 2, 2, 2, 3, 4)
    ok, ref = plan(*base)
    assert ok and plan(*base)[1] == ref
    for at, other in ((1, 4096), (5, 3), (6, 9), (7, 5)):
        args = list(base)
        args[at] = other
        assert plan(*args)[1]["words"] > ref["words"], at
