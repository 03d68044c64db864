"""The planted coefficient rows of tests/drop_edges.py and tests/base_edges.py before any GPU sees them (no GPU here): the builders'
conditions, the exact model against the oracle, the oracle against the reference at exactly these inputs, and which copy and flavour
of the drop each case of tests/test_gpu_drop_edges.py reaches -- so the path named in a GPU test's id is a checked fact."""
import numpy as np
import pytest

import base_edges as BE
import drop_edges as DE
import moduli as M
from oracle.pyoracle import SplitMix, have_ref
from test_host_drop_consts import ds  # noqa: F401  (the fixture: hp_drop.cpp behind tests/cpp/drop_shim.cpp)

U = np.uint64
ALL_CHAINS = [(name, 16 if name == "W59ish16" else 11) for name in ("SAME40", "WIDE_LAST", "NARROW_LAST", "W59ish", "W59ish16", "SMALL_MID", "PACK40EDGE")]


def _chain(name, logn):
    return DE.chain_of("W59ish" if name == "W59ish16" else name, logn)


# ---- builder conditions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,logn", ALL_CHAINS)
def test_every_listed_edge_value_is_in_the_set(name, logn):
    """re-derived here by search, not by the builder's formulas"""
    chain = _chain(name, logn)
    ql = chain[-1]
    h, vals = ql // 2, DE.edge_values(chain)
    assert all((q - 1) % (2 << logn) == 0 for q in chain) and len(set(chain)) == len(chain)
    assert vals == sorted(set(vals)) and all(0 <= v < ql for v in vals)
    assert {0, 1, h - 1, h, h + 1, ql - 2, ql - 1} <= set(vals)
    for q in chain[:-1]:
        r = ql % q
        for v in (q - 1, q, q + 1, 2 * q - 1):
            assert (v in vals) == (v < ql), (name, q, v)
        below = [v for v in vals if v < h and v % q == r]
        above = [v for v in vals if v >= h and v % q == r]
        if r < h:                                   # such a value exists below h
            assert below and h - max(below) <= q    # ... and the set has the largest one
        if h + ((r - h) % q) < ql:
            v = min(above)
            assert v - h < q and (v % q) + (q - r) == q      # remainder plus bump is exactly q, the lazy word for 0
        mult = [v for v in vals if v % q == 0]
        assert max(v for v in mult if v < h) + q >= h
        if -(-h // q) * q < ql:
            assert min(v for v in mult if v >= h) - q < h
    ext = DE.edge_values(chain, extended=True)
    assert set(ext) - set(vals) == {ql, ql + 1, 2 * ql - 1, 1 << 63, (1 << 64) - 1}


def test_chain_shapes():
    for logn in (3, 11, 15, 16):
        ch = DE.chains(logn)
        s = ch["SAME40"]
        assert all(q.bit_length() == 40 for q in s) and s[0] > s[-1] > s[1]
        assert [q.bit_length() for q in ch["WIDE_LAST"]] == [40, 40, 50]
        assert [q.bit_length() for q in ch["NARROW_LAST"]] == [50, 50, 40]
        assert [q.bit_length() for q in ch["W59ish"]] == [59, 20, 59]
        m = ch["SMALL_MID"]
        assert m[0] > m[-1] > m[1] and M.fold_consts(m[1])[2] > 1 << 38 and M.fold_consts(m[-1])[2] < 1 << 21
        for name in DE.LEVEL_B_CHAINS:
            assert DE.small(ch[name]) == (name in DE.SMALL_CHAINS), name          # q_last <= 2 q_k for every limb, or not for some limb
        assert not DE.small(ch["WIDE_LAST"], 0, 1) and not DE.small(ch["W59ish"], 1, 2) and DE.small(ch["W59ish"], 0, 1)
    for logn in (11, 13, 15):
        for name, chain in DE.chains_a(logn).items():
            assert M.level_a_chain(chain, logn), name
        assert DE.small(DE.chains_a(logn)["SAME40"]) and not DE.small(DE.chains_a(logn)["PACK40EDGE"])


@pytest.mark.parametrize("logn", [3, 10, 11, 12, 16])
@pytest.mark.parametrize("name", DE.LEVEL_B_CHAINS)
def test_rows_cover_every_block_and_parity(name, logn):
    chain, n = DE.chain_of(name, logn), 1 << logn
    ql = chain[-1]
    for extended in (False, True):
        vals = DE.edge_values(chain, extended)
        rows = DE.coefficient_rows(chain, n, 1, extended)
        assert rows.shape == (6, n) and rows.dtype == U
        assert (rows[0] == U(ql // 2 - 1)).all() and (rows[1] == U(ql // 2)).all() and (rows[2] == U(ql - 1)).all()
        assert set(int(v) for v in rows[3:].ravel()) <= set(vals)
        if not extended:
            assert (rows < U(ql)).all()
        if logn >= 10:                                   # 3 rows * n / 64 slots per (block, parity) cell >= 48 > the values
            assert DE.covered(rows[3:], vals)
            for i in range(3, 6):
                assert DE.covered(rows[i:i + 1], vals) == DE.per_row(n, len(vals)) or DE.covered(rows[i:i + 1], vals)
        if logn >= 12:
            assert DE.per_row(n, len(vals)) and all(DE.covered(rows[i:i + 1], vals) for i in range(3, 6))
    # the check itself notices a value that is missing from one cell
    broken = rows.copy()
    cell = broken[3:, n - n // 32:][:, 1::2]
    cell[cell == U(ql // 2)] = U(0)
    broken[3:, n - n // 32:][:, 1::2] = cell
    if logn >= 10:
        assert not DE.covered(broken[3:], vals)


# ---- the model is right ----------------------------------------------------------------------------------------------------------------
def _whole(orc, impl, chain, n, seed):
    """planted rows through the whole rescale / mod switch of `impl`, per scheme: (input, planted rows, output words)"""
    planted = DE.coefficient_rows(chain, n, seed)
    out = {}
    for t in (0,) + DE.PLAIN:
        x = DE.planted_ct(orc, SplitMix(seed + 1), chain, n, planted, t)
        words = np.stack([impl.bgv_mod_drop(chain, t, x[b]) if t else impl.ckks_rescale(chain, x[b]) for b in range(x.shape[0])])
        out[t] = (x, words)
    return planted, out


@pytest.mark.parametrize("logn", [3, 11])
@pytest.mark.parametrize("name", DE.LEVEL_B_CHAINS + ("PACK40EDGE",))
def test_model_gives_the_oracles_residues(orc, name, logn):
    chain, n = DE.chain_of(name, logn), 1 << logn
    planted, out = _whole(orc, orc, chain, n, 4100 + logn)
    note = {}
    for t, (x, words) in out.items():
        # the coefficient rows the engine will see ARE the planted ones
        ql = chain[-1]
        for p2 in range(planted.shape[0]):
            c = orc.batched_reduce_strict(ql, orc.intt(logn, ql, x[p2 // 2, p2 % 2, -1]))
            if t:
                c = ((c.astype(object) * pow(t, -1, ql)) % ql).astype(U)
            assert np.array_equal(c, planted[p2]), (name, t, p2)
            model = DE.model_drop(orc, chain, t, x[p2 // 2, p2 % 2], planted[p2], note=note)
            assert np.array_equal(model, DE.canon(words[p2 // 2, p2 % 2], chain[:-1])), (name, t, p2)
    # the plain formula on every chain of table-like moduli; at W59ish's 20-bit limb (0.75 * 2^20) hehub's transform words pass 2q and
    # its subtraction does wrap
    assert note["wraps"] == 0 or name not in DE.TABLE_CHAINS, note
    assert note["wraps"] > 0 or name != "W59ish", note


@pytest.mark.parametrize("logn", [11, 15])
def test_where_an_unreduced_small_remainder_shows(orc, logn):
    """The SMALL form's remainder is c - [c >= q_k] q_k.  Left unreduced (c itself, still below 2 q_k with the bump) it is the same
    residue, and next to a power of two hehub's transform gives it the SAME words -- no word-exact test on SAME40 can tell the two
    apart.  At SMALL_MID's mid-octave limb the words differ: that chain is what holds the subtraction in place."""
    n, differing = 1 << logn, {}
    for name in ("SAME40", "SMALL_MID"):
        chain = DE.chain_of(name, logn)
        q, ql = chain[1], chain[-1]
        assert q < ql <= 2 * q
        rows = DE.coefficient_rows(chain, n, 4100 + logn)
        assert (rows >= U(q)).any(axis=1).sum() >= 4                     # coefficients in [q_k, q_last): in the mixed rows and in row 2
        bump = np.where(rows >= U(ql // 2), U(q - ql % q), U(0))
        assert (rows + bump < U(2 * q)).all()
        differing[name] = sum(int((orc.ntt(logn, q, r % U(q) + b) != orc.ntt(logn, q, r + b)).sum()) for r, b in zip(rows, bump))
    assert differing["SAME40"] == 0 and differing["SMALL_MID"] > n // 8, differing


def test_model_centres_any_word():
    ql = 1099507695617
    h = ql // 2
    assert [DE.cen(c, ql) for c in (0, h - 1, h, ql - 1, ql, 2 * ql - 1, (1 << 64) - 1)] == \
        [0, h - 1, h - ql, -1, 0, ql - 1, (1 << 64) - 1 - ql]


# ---- the oracle is the reference at these inputs -----------------------------------------------------------------------------------------
needs_ref = pytest.mark.skipif(not have_ref(), reason="the compiled reference is not built here (oracle/_ref)")


@needs_ref
@pytest.mark.parametrize("logn", [3, 11])
@pytest.mark.parametrize("name", DE.LEVEL_B_CHAINS + ("PACK40EDGE",))
def test_oracle_is_the_reference_on_planted_drops(orc, ref, name, logn):
    chain, n = DE.chain_of(name, logn), 1 << logn
    _, mine = _whole(orc, orc, chain, n, 4100 + logn)
    _, theirs = _whole(orc, ref, chain, n, 4100 + logn)
    for t in mine:
        assert np.array_equal(mine[t][1], theirs[t][1]), (name, t)


@needs_ref
@pytest.mark.parametrize("n", [8, 4096])
def test_oracle_is_the_reference_on_planted_base_transforms(orc, ref, n):
    for old, new, x in BE.from_single_cases(n):
        assert np.array_equal(orc.rns_base_from_single(old, new, x), ref.rns_base_from_single(old, new, x)), (old, new)
    for name, old, new, x in BE.small_cases(n):
        for poly in x:
            assert np.array_equal(orc.rns_base_to_single(old, new, poly), ref.rns_base_to_single(old, new, poly)), name
            ok, got = orc.rns_base_to_single_small(old, new, poly)
            if ok:       # (the compiled reference falls into its CRT branch by itself where the polynomial is not small)
                assert np.array_equal(got, ref.rns_base_to_single_small(old, new, poly)[1]), name
    for name, old, new, x, want in BE.crt_cases(n):
        for poly in x:
            assert np.array_equal(orc.rns_base_to_single(old, new, poly), ref.rns_base_to_single(old, new, poly)), name


@pytest.mark.parametrize("n", [8, 4096])
def test_crt_values_in_python_integers_are_the_oracles(orc, n):
    for name, old, new, x, want in BE.crt_cases(n):
        for poly in x:
            assert not orc.rns_base_to_single_small(old, new, poly)[0], name      # the polynomial takes the CRT branch
            assert np.array_equal(orc.rns_base_to_single(old, new, poly), want), name


def test_base_case_builders():
    """the planted base-transform rows hold what they claim (Python integers)"""
    assert len(BE.CHAIN16) == 16 and len(set(BE.CHAIN17)) == 17 and all(q % 2 == 1 for q in BE.CHAIN17)
    widths = sorted(q.bit_length() for q in BE.SMALL["narrow_first"][0])
    assert widths == [17, 50] and BE.SMALL["wide_first"][0] == BE.SMALL["narrow_first"][0][::-1]
    for n in (8, 4096):
        for old, new, x in BE.from_single_cases(n):
            got = set(int(v) for v in x)
            assert {0, max(old // 2 - 1, 0), old // 2, old - 1, old, old + old // 2, 2 * old - 1} <= got, old
            assert old == 2 or any(q < old for q in new) or any(q > old for q in new)
        for name, old, new, x in BE.small_cases(n):
            m, Q = min(old) // 2, BE.product(old)
            assert x.shape == (6, len(old), n), name
            seen = [BE.crt_value([int(v) for v in x[p, :, BE.special_index(p, n)]], old) for p in range(6)]
            assert seen == [m - 1, m, m + 1, Q - (m - 1), Q - m, Q - (m + 1)], name
            assert (x[:, 0, 1] >= U(old[0])).all(), name                     # the lazy word
        for name, old, new, x, want in BE.crt_cases(n):
            Q = BE.product(old)
            for poly in x:
                vals = [BE.crt_value([int(v) % q for v, q in zip(poly[:, i], old)], old) for i in range(8)]
                assert vals == [0, 1, Q // 2 - 1, Q // 2, Q // 2 + 1, Q - 1, Q - new, Q - 2 * new], name
            assert (x[0] < np.array(old, dtype=U)[:, None]).all() and (x[1][0] >= U(old[0])).all(), name
            assert int(want[6]) == new and int(want[7]) == new and int(want[0]) == 0, name     # new | Q - x gives new itself, not 0


# ---- which copy each GPU case reaches ----------------------------------------------------------------------------------------------------
def _flavours(ds, addend, mask, bgv, small_rem):  # noqa: F811
    import ctypes as C
    out = (C.c_int * 2)()
    a = ds.ds_flavours(0, 0, 0, int(addend), mask, int(bgv), int(small_rem), out)
    return out[0], bool(out[1]), a


def _small_rem(ds, chain, k0, k1):  # noqa: F811
    import ctypes as C
    from test_host_drop_consts import ML
    out = (C.c_uint64 * (18 + 12 * ML))()
    ds.ds_drop((C.c_uint64 * len(chain))(*chain), len(chain), k0, k1, 0, 0, 0, out)
    return int(out[3])


def test_flavours_and_copies_of_the_gpu_cases(ds):  # noqa: F811
    """(BGV, add_mask) of the stage calls -> level-B flavours 0 .. 5 exactly; SMALL on for the strict calls on the SMALL chains and off
    elsewhere; every copy of the drop reached; level A reaches its flavours 1 .. 5 and hands BGV with add_mask 1 to level B's flavour 0."""
    import test_gpu_drop_edges as G

    seen_b, seen_small, seen_copy, seen_a = set(), set(), set(), set()
    for case in G.stage_calls():
        chain = DE.chain_of(case.chain, case.logn)
        sr = _small_rem(ds, chain, case.k0, case.k1) if case.strict else 0
        assert sr == int(case.strict and DE.small(chain, case.k0, case.k1))
        fb, small, fa = _flavours(ds, case.mask != 0, case.mask, case.t != 0, sr)
        assert fb == G.FLAVOUR_B[(case.t != 0, case.mask)], case
        assert small == (sr == 1 and fb != 0)
        seen_b.add(fb), seen_small.add(small)
    assert seen_b == {0, 1, 2, 3, 4, 5} and seen_small == {True, False}
    for name, logn, route in G.WHOLE_CASES:
        items = 6 * (len(DE.chain_of(name, logn)) - 1)
        copy = DE.copy_reached(logn, route, items)
        assert copy == G.whole_copy(logn, route), (name, logn, route)
        seen_copy.add(copy)
    assert seen_copy == {"rem/fin", "eager", "DropPre", "split"}
    assert DE.flavour_copy("DropPre", 0) == "eager"
    for t, mask in G.FLAVOUR_B:
        fb, _, fa = _flavours(ds, mask != 0, mask, t, 1)
        assert fa == G.FLAVOUR_A[(t, mask)]
        seen_a.add(fa)
    assert seen_a == {1, 2, 3, 4, 5, -1} and G.FLAVOUR_A[(True, 1)] == -1       # no level-A kernel: drop_apply's a_shape sends it to level B
    for logn in G.LEVEL_A_LOGNS:
        assert DE.copy_reached(logn, "default", 12, level_a=True) == "DropPreA"
