"""Moduli off the prime table (tests/moduli.py) on the CPU.

* the families and named chains reach both sides of the thresholds they are named for, and the Python mirrors of the engine's
  decisions agree with the engine's own host code (hp_tables.cpp through tests/cpp/tables_shim.cpp);
* the oracle equals the compiled reference word for word on every family and chain (where the reference is not built: its recorded
  digests, tests/golden/make_ref_digests.py) -- the domain the GPU tests of tests/test_gpu_moduli.py rely on;
* an independent exact reference (Kronecker substitution) pins what "exact" means: where hehub_fold_exact holds the oracle's
  transforms give the true negacyclic product, and on low_mid primes they do not (hehub's own fold wraps)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import moduli as M
import params as P
from oracle.pyoracle import SplitMix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = np.uint64
CPU_LOGN = (3, 6, 11)


def strict(q, x):
    return x % U(q)


# ---- part 1: the families reach their thresholds -------------------------------------------------------------------------------

def test_family_positions():
    for k, fam in M.FAMILIES.items():
        for name, q in fam.items():
            kb, fix, delta = M.fold_consts(q)
            assert M.log_modulus(q) <= 59 and M.max_logn(q) >= 11, (k, name)
            if name == "below":
                assert (kb, fix) == (k, 0) and delta < (1 << (k - 4))
            elif name == "above":
                assert fix == 1 and delta < (1 << (k - 4))
            elif name.startswith("low_mid"):
                assert (kb, fix) == (k, 1) and delta > (1 << (k - 5))
            else:
                assert (kb, fix) == (k + 1, 0) and delta > (1 << (k - 2))
    assert M.FAMILIES[17] == {"above": 65537} and set(M.FAMILIES[59]) == {"below", "above", "low_mid_1.05", "low_mid_1.1",
                                                                          "low_mid_1.3"}


@pytest.mark.parametrize("logn", [12, 15])
def test_chains_reach_both_sides_of_their_thresholds(logn):
    def packed(mext):
        cmax = max(mext[:-1])
        return [M.pack48(q, cmax, logn) for q in mext]

    for name, mext in M.CHAINS.items():
        assert all(M.max_logn(q) >= 15 for q in mext), name
        assert len(set(mext)) == len(mext), name
    w = packed(M.W59)
    assert any(w[1:10]) and not all(w[1:10]), "W59: packed and plain 40-bit limbs in one launch"
    nar = packed(M.NARROW)
    assert any(nar) and not all(nar) and M.NARROW[-1].bit_length() == 59 and min(M.NARROW).bit_length() <= 20
    pe = packed(M.PACKEDGE)
    kbs = [M.log_modulus(q) for q in M.PACKEDGE]
    assert [pe[i] for i in range(len(kbs)) if kbs[i] == 46] == [True, True]
    assert {47, 48} <= set(kbs) and not any(pe[i] for i in range(len(kbs)) if kbs[i] > 46)
    assert any(q > (1 << 48) and M.log_modulus(q) == 48 for q in M.PACKEDGE)
    assert all(M.fold_consts(q)[1] == 1 for q in M.ABOVE) and M.level_a_chain(M.ABOVE, logn)
    lm = packed(M.LOWMID)
    i = M.LOWMID.index(M.LOWMID_Q)
    assert M.fold_consts(M.LOWMID_Q)[:2] == (40, 1) and not lm[i] and all(lm[j] for j in range(len(lm) - 1) if j != i)
    assert not M.hehub_fold_exact(M.LOWMID_Q, max(M.LOWMID), logn) and not M.level_a_chain(M.LOWMID, logn)
    assert max(M.OVER50) > (1 << 50) and not M.level_a_chain(M.OVER50, logn) and M.level_a_chain(M.OVER50[:-1] + [P.P50[0]], logn)
    assert any(q + 2 <= (1 << 40) < q + (1 << 22) for q in M.PACK40EDGE) and any((1 << 40) < q < (1 << 40) + (1 << 22) for q in M.PACK40EDGE)
    assert M.level_a_chain(M.PACK40EDGE, logn)
    assert not M.level_a_chain(M.HIGHMID, logn)


@pytest.fixture(scope="module")
def tb():
    so = os.path.join(ROOT, "tests", "cpp", "libtables_shim.so")
    src = [os.path.join(ROOT, "tests", "cpp", "tables_shim.cpp"), os.path.join(ROOT, "hehub_amd", "csrc", "hp_tables.cpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in src):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so] + src, check=True)
    lib = C.CDLL(so)
    lib.tbl_fold.argtypes = [C.c_uint64, C.c_uint64, C.c_size_t, C.c_void_p]
    lib.tbl_level_a.argtypes = [C.c_uint64, C.c_uint64, C.c_size_t]
    return lib


def test_mirrors_agree_with_the_engine(tb):
    """moduli.fold_bound / hehub_fold_exact are the engine's hp::lazy_fold_bound / hp::level_a_modulus"""
    primes = sorted(set(M.ALL) | {q for c in M.CHAINS.values() for q in c} | set(P.P40 + P.P50))
    out = np.zeros(5, dtype=U)
    for q in primes:
        for logn in (1, 3, 6, 11, 12, 13, 15, 16):
            for x_in in (q, 2 * q, M.Q59, (1 << 64) - 1):
                tb.tbl_fold(q, x_in, logn, out.ctypes.data_as(C.c_void_p))
                wraps, m_delta, word_end = M.fold_bound(q, x_in, logn)
                assert (bool(out[0]), int(out[1]) | int(out[2]) << 64, int(out[3]) | int(out[4]) << 64) == (wraps, m_delta, word_end)
            for cmax in (q, P.P50[0], M.Q59):
                assert bool(tb.tbl_level_a(q, cmax, logn)) == M.hehub_fold_exact(q, cmax, logn), (q, cmax, logn)


# ---- part 2: the oracle against the compiled reference -------------------------------------------------------------------------

@pytest.mark.parametrize("k", M.WIDTHS)
def test_transforms_on_families(orc, ref, k):
    for name, q in M.FAMILIES[k].items():
        for logn in CPU_LOGN:
            n = 1 << logn
            for kind in M.INPUT_KINDS:
                x = M.edge_words(SplitMix(1000 * k + logn), kind, q, n)
                y = orc.ntt(logn, q, x)
                assert (y == ref.ntt(logn, q, x)).all(), (name, logn, kind)
                assert (orc.intt(logn, q, y) == ref.intt(logn, q, y)).all(), (name, logn, kind)
                assert (orc.intt(logn, q, x) == ref.intt(logn, q, x)).all(), (name, logn, kind)


@pytest.mark.parametrize("logn", CPU_LOGN)
@pytest.mark.parametrize("name", sorted(M.CHAINS))
def test_scheme_level_on_chains(orc, ref, name, logn):
    mext = M.CHAINS[name]
    n, L = 1 << logn, len(mext) - 1
    q = mext[:L]
    rng = SplitMix(100 * sorted(M.CHAINS).index(name) + logn)
    ct1 = M.lazy_rows(rng, (2, L, n), q)
    ct2 = rng.poly((2, L, n), q)
    key = rng.poly((L, 2, L + 1, n), mext)
    assert (orc.poly_mul(q, ct1[0], ct2[0]) == ref.poly_mul(q, ct1[0], ct2[0])).all()
    quad = orc.mult_low_level(q, ct1, ct2)
    assert (quad == ref.mult_low_level(q, ct1, ct2)).all()
    ext = orc.ext_prod(mext, quad[2], key)
    assert (ext == ref.ext_prod(mext, quad[2], key)).all()
    assert (orc.ckks_rescale(mext, ext) == ref.ckks_rescale(mext, ext)).all()
    if L >= 2:
        assert (orc.ckks_rescale(q, ct1) == ref.ckks_rescale(q, ct1)).all()
        for t in (65537, 2, 1):
            assert (orc.bgv_mod_drop(q, t, ct2) == ref.bgv_mod_drop(q, t, ct2)).all()
        assert (orc.ckks_mult(mext, ct1, ct2, key) == ref.ckks_mult(mext, ct1, ct2, key)).all()
        assert (orc.bgv_mult(mext, 65537, ct1, ct2, key) == ref.bgv_mult(mext, 65537, ct1, ct2, key)).all()
    for t in (65537, 2, 1):
        assert (orc.bgv_mod_drop(mext, t, ext) == ref.bgv_mod_drop(mext, t, ext)).all()
    assert (orc.ckks_rotate(mext, ct1, key, 3) == ref.ckks_rotate(mext, ct1, key, 3)).all()


# ---- part 2: the exact reference -------------------------------------------------------------------------------------------------

def _round_trip(orc, logn, q, x):
    return strict(q, orc.intt(logn, q, orc.ntt(logn, q, x)))


EXACT_CASES = [(q, logn) for q in M.ALL for logn in (3, 11) if M.hehub_fold_exact(q, q, logn)] + \
              [(q, logn) for k in (17, 30, 40, 50, 59) for q in (M.FAMILIES[k].get("below"), M.FAMILIES[k]["above"]) if q
               for logn in (13, 15) if logn <= M.max_logn(q) and M.hehub_fold_exact(q, q, logn)]


@pytest.mark.parametrize("q,logn", EXACT_CASES)
def test_exact_product_where_the_fold_is_exact(orc, q, logn):
    n = 1 << logn
    rng = SplitMix(q % 9973 + logn)
    a, b = M.edge_words(rng, "lazy", q, n), M.edge_words(rng, "max" if logn < 13 else "strict", q, n)
    A, B = orc.ntt(logn, q, a), orc.ntt(logn, q, b)
    assert (A < U(2 * q)).all() and (B < U(2 * q)).all()
    c = strict(q, orc.intt(logn, q, orc.poly_mul([q], A[None], B[None])[0]))
    assert (c == M.negacyclic_product(a, b, q)).all()
    assert (_round_trip(orc, logn, q, a) == strict(q, a)).all()


@pytest.mark.parametrize("k", [k for k in M.WIDTHS if k != 17])
def test_hehub_differs_from_the_exact_product_on_low_mid(orc, k):
    """hehub's quirk, not the oracle's: the oracle equals the reference there (test_transforms_on_families)"""
    for name, q in M.FAMILIES[k].items():
        if not name.startswith("low_mid"):
            continue
        for logn in (11, 13, 15):
            if logn > M.max_logn(q):
                continue
            x = M.edge_words(SplitMix(k + logn), "lazy", q, 1 << logn)
            if not (_round_trip(orc, logn, q, x) == strict(q, x)).all():
                y = M.edge_words(SplitMix(k), "strict", q, 1 << logn)
                prod = orc.intt(logn, q, orc.poly_mul([q], orc.ntt(logn, q, x)[None], orc.ntt(logn, q, y)[None])[0])
                assert not M.hehub_fold_exact(q, q, logn)
                if not (strict(q, prod) == M.negacyclic_product(x, y, q)).all():
                    return
    pytest.fail(f"no low_mid prime of width {k} makes hehub's fold wrap")


def test_predicate_is_sound(orc):
    """hehub_fold_exact never holds where the observed words break linearity modulo q or reach 2q"""
    for k, fam in M.FAMILIES.items():
        for name, q in fam.items():
            for logn in (3, 6, 11, 13):
                if logn > M.max_logn(q) or not M.hehub_fold_exact(q, q, logn):
                    continue
                n = 1 << logn
                rng = SplitMix(k * 7 + logn)
                xs = [M.edge_words(rng, kind, q, n) for kind in M.INPUT_KINDS]
                for x in xs:
                    y = orc.ntt(logn, q, x)
                    assert (y < U(2 * q)).all(), (k, name, logn)
                    assert (_round_trip(orc, logn, q, x) == strict(q, x)).all(), (k, name, logn)
                s = (xs[0] + xs[1]) % U(q)
                lhs = (orc.ntt(logn, q, xs[0]) % U(q) + orc.ntt(logn, q, xs[1]) % U(q)) % U(q)
                assert (lhs == orc.ntt(logn, q, s) % U(q)).all(), (k, name, logn)


def test_predicate_is_not_vacuous():
    for logn in range(1, 16):
        assert M.hehub_fold_exact(65537, 65537, logn)
    for mext, logn in ((P.C3_MODULI_EXT, P.C3_LOGN), (P.C5_MODULI_EXT, P.C5_LOGN), (P.C2_MODULI, P.C2_LOGN)):
        for lg in range(11, 16):
            assert M.level_a_chain(mext, lg)
    for logn in range(1, 16):
        for q in P.P40 + P.P50:
            assert M.hehub_fold_exact(q, max(P.P50), logn)
    # the chains of the level-A tests (tests/test_gpu_level_a.py): narrow limbs behind a 50-bit special prime included
    for logn in (11, 13, 15):
        top40, bit30, over40 = P.ntt_primes(1, logn, 40)[0], P.ntt_primes(1, logn, 30)[0], P.ntt_primes(1, logn, 41)[0]
        assert M.level_a_chain([top40, bit30, over40, P.P40[1], P.P50[0]], logn)
    assert M.level_a_chain([1099510054913, 1073479681, 1072496641, 1099507695617], 11)
    assert M.level_a_chain(P.ntt_primes(2, 13, 44) + P.ntt_primes(2, 13, 45) + P.ntt_primes(1, 13, 49), 13)
    # every prime just below 2^k (the table's kind) at every width level A takes, behind the widest modulus it takes
    for k, fam in M.FAMILIES.items():
        if "below" in fam and k < 50:
            for logn in range(11, min(15, M.max_logn(fam["below"])) + 1):
                assert M.level_a_chain([fam["below"], P.P50[0]], logn), (k, logn)
