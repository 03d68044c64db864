"""Host-side logic without a GPU: the work-item numbering of the transform launches (hehub_amd/csrc/hp_ntt_job.h: hp_decode_item,
hp_inv_item and the item counts; hp_device.h: hp_xcd_remap, hp_xcd_unit).

A launch of W workgroups finds its rows through this integer arithmetic alone, and a wrong term shows only where a tail exists
(L % G != 0, P % LPW != 0, W % 8 != 0, the special prime alone in the last group, one digit).  The functions are host-callable, so
every workgroup of every shape is decoded here on the CPU -- with src = dst = NULL and logn = 1 a pointer divided by the row size is a
row index and no memory is touched -- and the multiset of (source row, destination row, limb[, polynomial]) is compared with the
set of rows the launch has to cover, written down independently below: each item exactly once.  The GPU tests
(tests/test_gpu_launch_shapes.py) then only have to show that the kernels use the numbering correctly at the edge shapes."""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "cpp", "libntt_items_shim.so")
CSRC = os.path.join(ROOT, "hehub_amd", "csrc")
ML = 32   # HP_MAX_LIMBS
BATCH, SPREAD, HKS = 0, 1, 2   # HpNttMode

u32, u64, ptr = C.c_uint32, C.c_uint64, C.c_void_p


class HpNttJob(C.Structure):   # hp_kernels.h, field by field
    _fields_ = [("limbs", ptr), ("src", ptr), ("dst", ptr),
                ("logn", u32), ("L", u32), ("P", u32), ("src_pstride", u32), ("dst_pstride", u32), ("src_kstride", u32), ("W", u32),
                ("k_first", u32), ("pair_moduli", u32), ("hks_nd", u32), ("hks_E", u32), ("hks_alpha", u32), ("pack_mask", u32),
                ("pack40_mask", u32), ("mode", C.c_int), ("inverse", C.c_int), ("strict", C.c_int),
                ("post_scalar", u64), ("post_scalar_h", u64), ("use_post_scalar", C.c_int),
                ("limbs_a", ptr), ("src_words", u32), ("dst_f64", u32)]


@pytest.fixture(scope="module")
def ni():
    from hehub_amd.build import ARCH, _hipcc

    src = os.path.join(ROOT, "tests", "cpp", "ntt_items_shim.cpp")
    dep = [src] + [os.path.join(CSRC, h) for h in ("hp_ntt_job.h", "hp_kernels.h", "hp_device.h", "hp_drop.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in dep):
        # host side only: no device code is generated, the numbering is compiled for the CPU from the headers the kernels include
        subprocess.run([_hipcc(), f"--offload-arch={ARCH}", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared", "-x", "hip", src,
                        "-o", SO], check=True)
    lib = C.CDLL(SO)
    J = C.POINTER(HpNttJob)
    for name, args in (("ni_spread_items", [u32] * 4), ("ni_hks_items", [u32] * 4), ("ni_inv_grid", [J, u32]), ("ni_xcd_remap", [u32, ptr]),
                       ("ni_decode", [J, ptr]), ("ni_inv_items", [J, u32, u32, ptr]), ("ni_xcd_units", [u32, u32, ptr])):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, u32
    assert lib.ni_max_limbs() == ML
    return lib


def job(mode, L, P, W, **kw):
    return HpNttJob(logn=1, L=L, P=P, W=W, mode=mode, **kw)


def decode(ni, j, with_poly):
    """every workgroup of the launch through the forward kernels' prologue -> [(src row, dst row, limb[, poly])]"""
    out = np.full((j.W, 4), 0xDEAD, dtype=np.uint64)
    assert ni.ni_decode(C.byref(j), out.ctypes.data_as(ptr)) == j.W
    return [tuple(r) if with_poly else tuple(r[:3]) for r in out.tolist()]


def problems(items, expected):
    """what keeps the decoded items from being the expected set, each once: [] when nothing does.  `expected` is a list without
    repetitions"""
    got, exp = Counter(items), Counter(expected)
    assert all(c == 1 for c in exp.values()), "the expected rows are a set"
    out = [f"item {it} decoded {c} times" for it, c in got.items() if c > 1 and it in exp]
    out += [f"item {it} is no item of the launch" for it in got if it not in exp]
    out += [f"item {it} is never decoded" for it in exp if it not in got]
    if len(items) != len(expected):
        out.append(f"{len(items)} items decoded, {len(expected)} expected")
    return out


def check(items, expected, what):
    bad = problems(items, expected)
    assert not bad, (what, bad[:4])


# ---- the rows a launch has to cover ------------------------------------------------------------------------------------------------
def batch_rows(L, P, sps, sks, dps):
    return [(p * sps + k * sks, p * dps + k, k, p) for k in range(L) for p in range(P)]


def spread_rows(L, P, k0=0, k1=None):
    """digit j of polynomial p under every output modulus k != j of q_0 .. q_{L-1}, p (k = L: the special prime, never a digit)"""
    k1 = L + 1 if k1 is None else k1
    return [(p * L + j, (p * L + j) * (L + 1) + k, k) for k in range(k0, k1) for j in range(L) if j != k for p in range(P)]


def hks_rows(L, alpha, k, P):
    """in place: row (polynomial p, digit d, modulus m) of [P][nd][E] for every m outside digit d (the moduli d alpha .. d alpha + alpha - 1)"""
    nd, E = -(-L // alpha), L + k
    rows = [((p * nd + d) * E + m, m) for m in range(E) for d in range(nd) for p in range(P) if not (m < L and m // alpha == d)]
    return [(r, r, m) for r, m in rows]


# ---- HP_NTT_BATCH --------------------------------------------------------------------------------------------------------------------
def test_struct_mirror_has_the_size_of_the_struct(ni):
    assert ni.ni_sizeof_job() == C.sizeof(HpNttJob)


@pytest.mark.parametrize("P", [1, 2, 3, 5, 8])
def test_batch_items_with_and_without_groups(ni, P):
    shapes = 0
    for L in range(1, ML + 1):
        for G in range(L + 1):
            # rows [P][L] on both sides; the drop's shape: every limb of a polynomial reads the same row of [P]
            for sps, sks in ((L, 1), (1, 0)):
                j = job(BATCH, L, P, L * P, pair_moduli=G, src_pstride=sps, src_kstride=sks, dst_pstride=L)
                check(decode(ni, j, True), batch_rows(L, P, sps, sks, L), ("batch", L, P, G, sks))
                shapes += 1
    assert shapes == 2 * sum(L + 1 for L in range(1, ML + 1))


# ---- HP_NTT_SPREAD -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_spread_items_of_a_whole_launch(ni, P):
    for L in range(2, ML + 1):
        W = ni.ni_spread_items(L, P, 0, L + 1)
        assert W == L * L * P      # L+1 output moduli x L digits, less the L diagonal ones
        for G in range(L + 1):
            check(decode(ni, job(SPREAD, L, P, W, pair_moduli=G), False), spread_rows(L, P), ("spread", L, P, G))


@pytest.mark.parametrize("P", [1, 3])
def test_spread_items_of_a_modulus_range(ni, P):
    for L in range(2, 13):
        for k0 in range(L + 1):
            for k1 in range(k0 + 1, L + 2):
                W = ni.ni_spread_items(L, P, k0, k1)
                exp = spread_rows(L, P, k0, k1)
                assert W == len(exp), (L, P, k0, k1)
                check(decode(ni, job(SPREAD, L, P, W, k_first=k0), False), exp, ("spread range", L, P, k0, k1))


# ---- HP_NTT_HKS ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 5])
def test_hks_items(ni, k):
    digits = set()
    for L in range(1, 17):
        for alpha in range(1, 9):
            nd = -(-L // alpha)
            digits.add(nd)
            for P in (1, 2, 3):
                W = ni.ni_hks_items(L, nd, k, P)
                exp = hks_rows(L, alpha, k, P)
                assert W == len(exp), (L, alpha, k, P)
                check(decode(ni, job(HKS, L, P, W, hks_nd=nd, hks_E=L + k, hks_alpha=alpha), False), exp, ("hks", L, alpha, k, P))
    assert {1, 2, 16} <= digits   # one digit (only the special primes are items) up to HP_HKS_MAX_DIGITS


# ---- hp_xcd_remap --------------------------------------------------------------------------------------------------------------------
def test_xcd_remap_is_a_permutation_with_an_identity_tail(ni):
    for W in range(4097):
        out = np.full(W, 0xFFFFFFFF, dtype=np.uint32)
        ni.ni_xcd_remap(W, out.ctypes.data_as(ptr))
        assert np.array_equal(np.sort(out), np.arange(W, dtype=np.uint32)), W
        head = 8 * (W >> 3)
        assert np.array_equal(out[head:], np.arange(head, W, dtype=np.uint32)), W
        # XCD x (the blocks b = x mod 8) gets the contiguous slice [x W/8, (x+1) W/8), in order
        b = np.arange(head, dtype=np.uint32)
        assert np.array_equal(out[:head], (b & 7) * (W >> 3) + (b >> 3)), W


# ---- the tiled inverse kernels' groups of LPW polynomials of one modulus --------------------------------------------------------------
@pytest.mark.parametrize("LPW", [1, 2, 4, 8])
def test_inverse_groups(ni, LPW):
    for L in range(1, 13):
        for P in range(1, 3 * LPW + 2):
            # rows [P][L] in place; and a one-modulus launch out of / into wider rows (src_pstride, dst_pstride as the drops have them)
            for sps, dps in ((L, L), (L + 3, L + 1)):
                j = job(BATCH, L, P, L * P, src_pstride=sps, src_kstride=1, dst_pstride=dps)
                grid = ni.ni_inv_grid(C.byref(j), LPW)
                assert grid == L * -(-P // LPW), (LPW, L, P)
                out = np.full((grid * LPW, 5), 0xDEAD, dtype=np.uint64)
                ni.ni_inv_items(C.byref(j), LPW, grid, out.ctypes.data_as(ptr))
                rows = out.tolist()
                check([tuple(r[1:]) for r in rows if r[0]], batch_rows(L, P, sps, 1, dps), ("inverse", LPW, L, P, sps))
                idle = [r for r in rows if not r[0]]
                assert len(idle) == grid * LPW - L * P
                for _, s, d, k, p in idle:      # stores nothing, but loads: a row of the launch
                    assert k < L and p == P - 1 and s == p * sps + k and d == p * dps + k, (LPW, L, P, sps)
                # a workgroup's sub-limbs share one modulus (they share its staged twiddles)
                limbs = np.array([r[3] for r in rows]).reshape(grid, LPW)
                assert (limbs == limbs[:, :1]).all(), (LPW, L, P)


# ---- units by XCD (hp_hks.hip) -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 3, 8, 9])
def test_units_by_xcd(ni, W):
    for units in range(1, 41):
        out = np.full((units * W, 2), 0xFFFFFFFF, dtype=np.uint32)
        ni.ni_xcd_units(units, W, out.ctypes.data_as(ptr))
        check([tuple(r) for r in out.tolist()], [(u, w) for u in range(units) for w in range(W)], ("units", units, W))
        # of eight consecutive workgroups of the grouped part each has its own unit
        g = (units & ~7) * W
        assert (out[:g, 0].reshape(-1, 8) % 8 == np.arange(8)).all(), (units, W)


# ---- the comparison has teeth --------------------------------------------------------------------------------------------------------
def test_wrong_numberings_are_rejected(ni):
    """a launch with a tail in every direction (L % G != 0, the special prime alone in the last group, W % 8 != 0), decoded
    correctly and then damaged the three ways a wrong term damages it"""
    L, P, G = 5, 3, 4
    W = ni.ni_spread_items(L, P, 0, L + 1)
    assert W % 8 != 0 and L % G == 1
    good, exp = decode(ni, job(SPREAD, L, P, W, pair_moduli=G), False), spread_rows(L, P)
    assert problems(good, exp) == []
    swapped = list(good)      # two transforms written into each other's rows
    (s0, d0, k0), (s1, d1, k1) = swapped[3], swapped[W - 2]
    assert d0 != d1
    swapped[3], swapped[W - 2] = (s0, d1, k0), (s1, d0, k1)
    assert problems(swapped, exp)
    repeated = good[:-1] + [good[-2]]      # the last item of the tail done twice, the one after it never
    assert any("decoded 2 times" in m for m in problems(repeated, exp)) and any("never decoded" in m for m in problems(repeated, exp))
    assert any("never decoded" in m for m in problems(good[:-1], exp))      # a count one short: a row left unwritten
    assert problems(good + [good[0]], exp)                                    # a count one over
    with pytest.raises(AssertionError):
        check(good[:-1], exp, "missing")
    # the same for a batch launch, where the polynomial is part of the item
    j = job(BATCH, 7, 3, 21, pair_moduli=4, src_pstride=1, src_kstride=0, dst_pstride=7)
    good, exp = decode(ni, j, True), batch_rows(7, 3, 1, 0, 7)
    assert problems(good, exp) == []
    wrong_poly = [(s, d, k, (p + 1) % 3) if i == 20 else (s, d, k, p) for i, (s, d, k, p) in enumerate(good)]
    assert problems(wrong_poly, exp)
