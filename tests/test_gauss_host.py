"""The discrete Gaussian rule of hehub_amd/csrc/hp_sample.h (kind 4) and the host samplers of hp_sample_host.cpp under it, against
tests/gauss_model.py (CPU tier, through tests/cpp/gauss_shim.cpp, built with g++).  The header's constexpr functions are the very
functions the kernels of hp_sample.hip call, so what holds here holds for the code the device runs, up to the kernel's own indexing,
which tests/test_gpu_gauss.py covers."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import gauss_cases as GC
import gauss_model as G
import sample_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "cpp", "libgauss_shim.so")
CSRC = os.path.join(ROOT, "hehub_amd", "csrc")
U = np.uint64
TOP = (1 << 63) - 1


@pytest.fixture(scope="module")
def gs():
    src = [os.path.join(ROOT, "tests", "cpp", "gauss_shim.cpp"), os.path.join(CSRC, "hp_sample_host.cpp")]
    dep = src + [os.path.join(CSRC, "hp_sample.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in dep):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", SO] + src, check=True)
    lib = C.CDLL(SO)
    lib.gs_kind.restype = lib.gs_entries.restype = C.c_uint
    lib.gs_table.argtypes = [C.c_uint]
    lib.gs_table.restype = lib.gs_max_scale.restype = C.c_uint64
    lib.gs_gauss_word.argtypes = [C.c_uint64]
    lib.gs_small_word.argtypes = [C.c_uint, C.c_uint64]
    lib.gs_gauss_word.restype = lib.gs_small_word.restype = C.c_longlong
    lib.gs_signed.argtypes = [C.c_uint, C.c_size_t, C.c_size_t, C.c_char_p, C.c_uint64, C.c_longlong, C.c_void_p]
    lib.gs_signed.restype = None
    lib.gs_small.argtypes = [C.c_uint, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_char_p, C.c_uint64, C.c_uint64, C.c_longlong,
                             C.c_void_p]
    lib.gs_small.restype = None
    return lib


# ---- 1. the table -------------------------------------------------------------------------------------------------------------------------
def test_table_literals_are_the_recomputed_cumulatives(gs):
    assert gs.gs_kind() == G.GAUSS == 4 and gs.gs_entries() == G.ENTRIES == 30
    assert G.PRECISION * math.log2(10) >= 200
    assert [gs.gs_table(i) for i in range(G.ENTRIES)] == G.TABLE
    # the entries the issue quotes, and the end of the table
    assert G.TABLE[:4] == [1149872835429266008, 3340023666152832877, 5231742854224525755, 6713673034491318533]
    assert G.TABLE[28] == (1 << 63) - 4 and G.TABLE[29] == TOP
    assert all(a < b for a, b in zip(G.TABLE, G.TABLE[1:]))


def test_a_31st_entry_would_repeat_the_30th_and_no_entry_hangs_on_the_last_digits():
    longer = G.table(40)
    assert longer[:G.ENTRIES] == G.TABLE and all(c == TOP for c in longer[G.ENTRIES - 1:])
    # the fractional part of every scaled cumulative is far from 0 and 1: the floor does not depend on the precision
    fractions = [float(x - int(x)) for x in G.scaled_cumulatives(G.ENTRIES)]
    assert 0.008 < min(fractions) and max(fractions) < 0.94, (min(fractions), max(fractions))
    assert abs(G.variance() - G.Decimal("10.24")) < G.Decimal(10) ** -80
    # 30 * scale fits an int64 for every scale the calls admit
    assert G.ENTRIES * ((1 << 58) - 1) < 1 << 63


def test_max_scale_is_where_it_was(gs):
    assert gs.gs_max_scale() == 1 << 58


# ---- 2. the word rule on planted candidates -----------------------------------------------------------------------------------------------
def planted():
    """[(candidate, word)]: for every m, u = C[m] - 1 and u = C[m] under both signs (120 words), then the ends of the range"""
    out = []
    for m, c in enumerate(G.TABLE):
        for u, mag in ((c - 1, m), (c, m + 1)):
            out += [(u << 1, mag), (u << 1 | 1, -mag)]
    out += [(0 << 1, 0), (0 << 1 | 1, 0), (TOP << 1, 30), (TOP << 1 | 1, -30), (0, 0), (1, 0)]
    return out


def test_planted_candidates_through_the_shared_word_rule(gs):
    words = planted()
    assert len(words) == 126 and sorted({w for _, w in words}) == list(range(-30, 31))
    for v, w in words:
        assert 0 <= v <= S.M64
        assert gs.gs_gauss_word(v) == G.gauss_word(v) == w == gs.gs_small_word(G.GAUSS, v), hex(v)
    assert gs.gs_gauss_word(0) == gs.gs_gauss_word(1) == 0          # zero carries no sign
    # the other kinds of the shared dispatch are as they were
    for v, _ in words[:16]:
        assert gs.gs_small_word(S.TERNARY, v) == S.ternary_word(v) and gs.gs_small_word(S.CBD, v) == S.cbd_word(v)


def test_keystream_candidates_through_the_word_rule(gs):
    cands = S.candidates(S.chacha20_blocks(S.states(GC.SEED, np.arange(64), S.word13(0, G.GAUSS, 0), 1))).reshape(-1)
    row = G.gauss_row(9, GC.SEED, 1)
    for v, w in zip(cands, row):
        assert gs.gs_gauss_word(int(v)) == G.gauss_word(int(v)) == int(w)


# ---- 3. rows ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", GC.HOST_LOGN)
def test_host_signed_rows_equal_the_model(gs, logn):
    batch, stream = 3, (1 << 32) - 2                             # (the ids carry into word 15)
    exp = G.sample_gauss(logn, GC.SEED, stream, batch)
    for scale in GC.SCALES:
        out = np.zeros((batch, 1 << logn), dtype=np.int64)
        gs.gs_signed(G.GAUSS, logn, batch, GC.SEED, stream, scale, out.ctypes.data)
        assert np.array_equal(out, scale * exp)
    assert np.array_equal(exp[1], G.gauss_row(logn, GC.SEED, stream + 1))


@pytest.mark.parametrize("logn", GC.HOST_LOGN)
def test_host_residue_rows_equal_the_model(gs, logn):
    moduli, batch, stream = GC.SMALL_Q, 2, 77
    assert min(moduli) < 30 * max(GC.SCALES)                      # hp_sample_residue's division runs
    marr = (C.c_uint64 * len(moduli))(*moduli)
    for scale in GC.SCALES:
        for id_step in (1, 2):
            out = np.zeros((batch, len(moduli), 1 << logn), dtype=U)
            gs.gs_small(G.GAUSS, logn, len(moduli), marr, batch, GC.SEED, stream, id_step, scale, out.ctypes.data)
            assert np.array_equal(out, G.sample_small(logn, moduli, GC.SEED, stream, scale, batch, id_step)), (scale, id_step)
            assert bool((out < np.array(moduli, dtype=U)[None, :, None]).all())
    big = scale * np.abs(G.sample_gauss(logn, GC.SEED, stream, batch))
    assert int(big.max()) >= 65537                                # (some magnitude did reach the small modulus)


# ---- 4. the kind tag separates the keystream ----------------------------------------------------------------------------------------------
def test_kind_4_shares_no_block_with_kinds_1_to_3():
    seen = {}
    for kind in (S.UNIFORM, S.TERNARY, S.CBD, G.GAUSS):
        out = S.chacha20_blocks(S.states(GC.SEED, np.arange(32), S.word13(0, kind, 0), 4))
        seen[kind] = {bytes(b) for b in out.astype("<u4")}
        assert len(seen[kind]) == 32
    for kind in (S.UNIFORM, S.TERNARY, S.CBD):
        assert not (seen[G.GAUSS] & seen[kind]), kind
    # and the rows drawn from them differ: were the blocks shared, the Gaussian row would be a function of the binomial row's candidates
    g, c = G.gauss_row(8, GC.SEED, 4), S.cbd_row(8, GC.SEED, 4)
    assert not np.array_equal(np.sign(g), np.sign(c)) and not np.array_equal(np.clip(g, -1, 1), S.ternary_row(8, GC.SEED, 4))
    assert not np.array_equal(g, G.gauss_row(8, GC.SEED, 5)) and not np.array_equal(g, G.gauss_row(8, GC.SEED2, 4))


# ---- 5. the distribution under a fixed seed -----------------------------------------------------------------------------------------------
DF = 19
QUANTILE = 63.68      # the 1 - 10^-6 quantile of chi-square with 19 degrees of freedom (63.677), rounded up


def chi2_sf_odd(x, df):
    """P(X > x) of chi-square with an odd number of degrees of freedom: the closed form, erfc plus a finite sum"""
    assert df % 2 == 1
    term, total = 1.0, 0.0
    for k in range((df - 1) // 2):
        total += term                      # x^k / (1 * 3 * .. * (2k + 1))
        term *= x / (2 * k + 3)
    return math.erfc(math.sqrt(x / 2)) + math.sqrt(2 * x / math.pi) * math.exp(-x / 2) * total


def test_chi_square_and_variance_of_a_million_words():
    assert chi2_sf_odd(QUANTILE, DF) <= 1e-6 < chi2_sf_odd(QUANTILE - 0.05, DF)
    x = G.sample_gauss(GC.DIST_LOGN, GC.DIST_SEED, GC.DIST_STREAM, GC.DIST_BATCH).reshape(-1)
    n = len(x)
    assert n == 1 << 20
    p = [float(v) for v in G.probabilities()]
    expected = [p[0]] + [p[m] / 2 for m in range(1, 10) for _ in (1, -1)] + [sum(p[10:])]
    observed = [int((x == 0).sum())] + [int((x == s * m).sum()) for m in range(1, 10) for s in (1, -1)] + [int((np.abs(x) >= 10).sum())]
    assert len(expected) == DF + 1 and sum(observed) == n and abs(sum(expected) - 1) < 1e-12
    stat = sum((o - n * e) ** 2 / (n * e) for o, e in zip(observed, expected))
    var = float(x.astype(np.float64).var())
    print(f"chi-square {stat:.3f} (bound {QUANTILE}), sample variance {var:.4f}, mean {float(x.mean()):.5f}, range {x.min()} .. {x.max()}")
    assert stat < QUANTILE
    assert abs(var - 10.24) <= 0.01 * 10.24
    assert -30 <= int(x.min()) and int(x.max()) <= 30


# ---- 6. the premise of the GPU inputs -----------------------------------------------------------------------------------------------------
def test_gpu_rows_hold_every_magnitude_up_to_11_with_both_signs():
    assert GC.SIGNED_SHAPES[-1] == (11, 8)
    rows = GC.model_signed(11, 8)
    for m in GC.PREMISE_MAGNITUDES:
        assert bool((rows == m).any()) and bool((rows == -m).any()), m
