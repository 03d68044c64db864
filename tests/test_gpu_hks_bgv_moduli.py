"""The BGV calls over the hybrid key switch, lazy relinearisation and the any-level (_at) calls on wide and off-table moduli: the chains
of tests/moduli.py cut to (L, k), WIDE58 (tests/hks_edges.py: every modulus 58 or 59 bits, the 58-bit high_mid prime among them), NARROW
once, and W59LAST (the 59-bit prime as q_last).  tests/test_gpu_hks_bgv.py, test_gpu_hks_dot.py and test_gpu_hks_levels.py run the same
calls on 40-bit limbs and 50-bit special primes only; here
  * k_hks_moddown_t (the one kernel that knows t) meets 58- to 60-bit special primes, primes just above a power of two, high_mid limbs
    whose lazy transform words exceed 2q, limbs wider than the special primes, and a 58-bit plain modulus;
  * the operands are lazy (words in [q, 2q), some 2q - 1), rows of every moduli.INPUT_KINDS kind, and everything 2q - 1;
  * the _at addressing reads a top-level key over limbs of different widths;
  * the whole dot call sums 32 products of all-(2q - 1) words at 59-bit moduli before its one switch.
The inputs are those of tests/hks_bgv_edges.py; tests/test_hks_bgv_edges.py holds them to their own conditions without a GPU (the
premise of the exact models, t < every modulus, the planted classes, the 128-bit sums).  The models are tests/hks_bgv_model.py and
tests/dot_model.py: Python integers around the oracle's transforms.  The comparison is hks_model.residues_match -- the same residues,
every word below 2q -- at parity level B and in a level-A context; the model of a case is computed once and held against both.

What these cases found, and why some chains are absent from sections 3, 5 and 6: the calls that END in one of hehub's drops (the BGV mod
switch of relin_modswitch / mult, the rescale of the dot below the fused degrees) follow hehub word for word there, and hehub's lazy
subtraction of the remainder's transform wraps at a high_mid limb that the drop keeps -- its result is then no function of the residues
(hks_bgv_edges.drop_premise; tests/test_hks_bgv_edges.py shows it on the oracle alone: 1423 of 2048 residues of that limb of HIGHMID, on
canonical input).  On HIGHMID, and on WIDE58 (whose high_mid prime is q_0), bgv_relin_modswitch_hks and the model's hehub drop were given
different representatives of the same residues and differed on that limb only.  The models of those sections are therefore held on
chains that pass the drop premise -- WIDE58R, WIDE58's primes with the high_mid one as q_last, in WIDE58's place -- and HIGHMID / WIDE58
run through them against the engine's own two-step compositions, word for word."""
import time

import numpy as np
import pytest

import hks_bgv_edges as E
import hks_bgv_model as B
import hks_edges as H
import moduli as M
from dot_model import below_2q, model_dot, strict_rows
from gpu_words import at_both_levels, case_id, dev_i64, residues
from hks_levels import embed_key, level_chain, level_digits, sub_key
from hks_model import model_digits, residues_match
from oracle.pyoracle import SplitMix
from test_tensor_sum_host import TABLE, ts  # noqa: F401  (the fixture around hpi::tensor_sum_max_terms)

pytestmark = pytest.mark.gpu
U = np.uint64
BATCH, T0 = E.BATCH, E.T0
SPENT = {"model": 0.0, "start": None}


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    SPENT["start"] = time.perf_counter()
    yield e
    e.close()
    wall = time.perf_counter() - SPENT["start"]
    print(f"\ntest_gpu_hks_bgv_moduli: {SPENT['model']:.1f} s in the CPU models, {wall - SPENT['model']:.1f} s elsewhere (GPU, transfers, inputs)")


class modelled:
    """with modelled(): ... -- the time the exact models take, summed for the module's closing line"""

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        SPENT["model"] += time.perf_counter() - self.t0


def mismatch(got, exp, q):
    """for the failure message: the differing residues per (polynomial, limb) row and the first three places"""
    qa = np.array(q, dtype=U)[None, :, None]
    bad = (got % qa).astype(object) != exp
    return bad.sum(axis=2).tolist(), [(w, int(got[tuple(w)]), int(exp[tuple(w)])) for w in np.argwhere(bad)[:3].tolist()]


def plain_moduli(case):
    """hks_bgv_edges.plain_moduli, and the 58-bit plain modulus where the case is the one for it"""
    ts_ = E.plain_moduli(case)
    if case == E.EDGE_T_CASE:
        ts_ += (E.edge_t(E.chain_of(case[0], case[2], case[3])),)
    return ts_


# ---- 1. the switch ---------------------------------------------------------------------------------------------------------------------
def switch_is_the_model(eng, orc, case, fill, ts_):
    name, logn, L, k, alpha = case
    mext, pt, key = E.switch_inputs(case, fill)
    q, n = mext[:L], 1 << logn
    with modelled():
        acc = [B.inner(mext, model_digits(orc, logn, mext, L, k, alpha, pt[b]), key) for b in range(BATCH)]   # (no t before ModDown)
    d_pt, d_key = eng.to_device(pt), eng.to_device(key)
    for t in ts_:
        with modelled():
            exp = [B.mod_down_bgv(orc, logn, mext, L, k, t, a) for a in acc]
        got = at_both_levels(eng, lambda: eng.to_host(eng.bgv_hks_switch(mext, t, k, alpha, d_pt, d_key)))
        for level, g in got.items():
            assert g.shape == (BATCH, 2, L, n)
            for b in range(BATCH):
                assert residues_match(g[b], exp[b], q), (level, t, b, mismatch(g[b], exp[b], q))


@pytest.mark.parametrize("fill", ["lazy", "kinds"])
@pytest.mark.parametrize("case", E.sweep_cases(), ids=case_id)
def test_switch_matches_the_model(eng, orc, case, fill):
    switch_is_the_model(eng, orc, case, fill, plain_moduli(case))


@pytest.mark.parametrize("case", E.MAX_CASES, ids=case_id)
def test_switch_of_the_largest_words(eng, orc, case):
    """every ciphertext and key word 2q - 1 (tests/test_hks_bgv_edges.py has the digit-loop sums: within 2^7.4 of the register)"""
    switch_is_the_model(eng, orc, case, "max", plain_moduli(case))


@pytest.mark.parametrize("fill", ["lazy", "kinds"])
def test_switch_on_narrow_limbs_with_t_2(eng, orc, fill):
    switch_is_the_model(eng, orc, E.NARROW_CASE, fill, (2,))


@pytest.mark.parametrize("case", E.PLANTED_CASES, ids=case_id)
def test_switch_of_planted_accumulators(eng, orc, case):
    """ModDown_t's input chosen coefficient by coefficient through the public call (hks_bgv_model.planted_values has the classes): the
    expected output is plain integer arithmetic"""
    name, logn, L, k, alpha = case
    mext, n = E.chain_of(name, L, k), 1 << logn
    q = mext[:L]
    d_pt = eng.to_device(np.stack([B.planted_pt(L, n)] * BATCH))
    for t in plain_moduli(case):
        with modelled():
            w = E.planted(case, t)
            assert all(B.planted_classes(w, mext, L, k, t).values())
            key = B.planted_key(orc, logn, mext, L, k, alpha, w)
            exp = B.planted_expected(orc, logn, mext, L, k, t, w)
        d_key = eng.to_device(key)
        got = at_both_levels(eng, lambda: eng.to_host(eng.bgv_hks_switch(mext, t, k, alpha, d_pt, d_key)))
        for level, g in got.items():
            for b in range(BATCH):
                assert residues_match(g[b], exp, q), (level, t, b, mismatch(g[b], exp, q))


@pytest.mark.parametrize("case", E.sweep_cases() + [E.NARROW_CASE], ids=case_id)
def test_plain_modulus_one_gives_the_residues_of_the_ckks_switch(eng, case):
    name, logn, L, k, alpha = case
    mext, pt, key = E.switch_inputs(case, "lazy")
    q = mext[:L]
    d_pt, d_key = eng.to_device(pt), eng.to_device(key)
    got = at_both_levels(eng, lambda: (eng.to_host(eng.bgv_hks_switch(mext, 1, k, alpha, d_pt, d_key)),
                                       eng.to_host(eng.hks_switch(mext, k, alpha, d_pt, d_key))))
    for level, (bgv, ckks) in got.items():
        assert (bgv < 2 * np.array(q, dtype=U)[:, None]).all(), level
        assert np.array_equal(residues(bgv, q), residues(ckks, q)), level


# ---- 2. hoisted rotations ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.HOISTED_CASES, ids=case_id)
def test_hoisted_rotations_match_the_model(eng, orc, case):
    name, logn, L, k, alpha = case
    mext, n = E.chain_of(name, L, k), 1 << logn
    q, nd = mext[:L], E.nd_of(L, alpha)
    rng = SplitMix(E.seed_of(case, 100))
    steps, conj = [3, 0, 0], [False, False, True]   # a rotation of the rows, step 0, the row swap
    ct = M.lazy_rows(rng, (BATCH, 2, L, n), q)
    keys = [E.key_rows(rng, "lazy", mext, nd, n) for _ in steps]
    with modelled():
        D = [model_digits(orc, logn, mext, L, k, alpha, np.ascontiguousarray(ct[b, 1])) for b in range(BATCH)]
    d_ct, d_keys = eng.to_device(ct), [eng.to_device(key) for key in keys]
    for t in plain_moduli(case):
        with modelled():
            exp = [B.model_hoisted_bgv(orc, logn, mext, L, k, alpha, t, ct[b], keys, steps, conj, D[b]) for b in range(BATCH)]
        got = at_both_levels(eng, lambda: (eng.to_host(eng.bgv_rotate_hoisted_hks(mext, t, k, alpha, d_ct, d_keys, steps, conj)),
                                           eng.to_host(eng.bgv_rotate_hoisted_hks(mext, t, k, alpha, d_ct, d_keys[:1], steps[:1]))))
        for level, (g, single) in got.items():
            assert g.shape == (BATCH, 3, 2, L, n) and single.shape == (BATCH, 1, 2, L, n)
            for b in range(BATCH):
                for r in range(3):
                    assert residues_match(g[b, r], exp[b][r], q), (level, t, b, r, mismatch(g[b, r], exp[b][r], q))
                assert residues_match(single[b, 0], exp[b][0], q), (level, t, b)   # rotations == 1: row 0 of the longer call
                assert np.array_equal(residues(single[b, 0], q), residues(g[b, 0], q)), (level, t, b)


# ---- 3. relinearisation + mod switch, and the multiplication -------------------------------------------------------------------------------
QUADS = ("low", "max", "sum")


@pytest.mark.parametrize("quad_kind", QUADS)
@pytest.mark.parametrize("case", E.RELIN_CASES, ids=case_id)
def test_relin_modswitch_and_mult_match_the_model(eng, orc, case, quad_kind):
    """three quadratic ciphertexts: mult_low_level of lazy operands (and the fused multiplication on the same operands, word for word),
    every word 2q - 1, and a ckks_tensor_sum of three products"""
    name, logn, L, k, alpha = case
    mext, n = E.chain_of(name, L, k), 1 << logn
    q = mext[:L]
    rng = SplitMix(E.seed_of(case, 200 + QUADS.index(quad_kind)))
    key = E.key_rows(rng, "lazy", mext, E.nd_of(L, alpha), n)
    d_key = eng.to_device(key)
    ops = [eng.to_device(M.lazy_rows(rng, (BATCH, 2, L, n), q)) for _ in range(4)]
    if quad_kind == "low":
        d_quad = eng.mult_low_level(q, ops[0], ops[1])
    elif quad_kind == "max":
        d_quad = eng.to_device(H.max_rows((BATCH, 3, L, n), q))
    else:
        d_quad = eng.ckks_tensor_sum(q, [ops[0], ops[1], ops[2]], [ops[1], ops[3], ops[2]])
    quad = eng.to_host(d_quad)
    assert below_2q(quad, q)
    for t in plain_moduli(case):
        with modelled():
            exp = [B.model_relin_modswitch_bgv(orc, logn, mext, L, k, alpha, t, quad[b], key) for b in range(BATCH)]

        def run():
            tail = eng.to_host(eng.bgv_relin_modswitch_hks(mext, t, k, alpha, d_quad, d_key))
            return tail, (eng.to_host(eng.bgv_mult_hks(mext, t, k, alpha, ops[0], ops[1], d_key)) if quad_kind == "low" else None)

        for level, (tail, mult) in at_both_levels(eng, run).items():
            assert tail.shape == (BATCH, 2, L - 1, n)
            for b in range(BATCH):
                assert residues_match(tail[b], exp[b], q[:-1]), (level, t, b, mismatch(tail[b], exp[b], q[:-1]))
            if mult is not None:
                assert np.array_equal(mult, tail), (level, t)   # the fused call IS mult_low_level + the tail: word for word


@pytest.mark.parametrize("case", E.RELIN_WORD_CASES, ids=case_id)
def test_mult_is_its_two_halves_word_for_word_where_the_drop_has_no_model(eng, case):
    """HIGHMID and WIDE58 (a high_mid limb below q_last: hks_bgv_edges.drop_premise fails): the fused multiplication against
    mult_low_level followed by the exposed tail -- the same code on the same quad, the same WORDS, every word below 2q"""
    name, logn, L, k, alpha = case
    mext, n = E.chain_of(name, L, k), 1 << logn
    q = mext[:L]
    rng = SplitMix(E.seed_of(case, 250))
    d_key = eng.to_device(E.key_rows(rng, "lazy", mext, E.nd_of(L, alpha), n))
    d_a, d_b = (eng.to_device(M.lazy_rows(rng, (BATCH, 2, L, n), q)) for _ in range(2))
    for t in plain_moduli(case):
        got = at_both_levels(eng, lambda: (eng.to_host(eng.bgv_mult_hks(mext, t, k, alpha, d_a, d_b, d_key)),
                                           eng.to_host(eng.bgv_relin_modswitch_hks(mext, t, k, alpha, eng.mult_low_level(q, d_a, d_b), d_key))))
        for level, (mult, tail) in got.items():
            assert mult.shape == (BATCH, 2, L - 1, n) and below_2q(mult, q[:-1]), (level, t)
            assert np.array_equal(mult, tail), (level, t)


# ---- 4. one top-level key set at two levels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.AT_CASES, ids=case_id)
def test_at_calls_with_a_top_level_key_over_limbs_of_different_widths(eng, orc, case):
    """a top key of key_L0 = L + 2 at levels L (partial last digit) and L - 1: every _at call, BGV and CKKS, equals the plain call on
    hks_levels.sub_key's compact extraction word for word at both parity levels; at N = 16 the BGV switch is also held to the model.
    The level key is planted into a top-shaped block of words of another stream (embed_key)."""
    name, logn, key_L0, L0, k, alpha = case
    n, mtop, t = 1 << logn, E.at_chains(name, key_L0, k), T0
    rng, fill = SplitMix(E.seed_of((name, logn, L0, k, alpha), 300)), SplitMix(E.seed_of((name, logn, L0, k, alpha), 377))
    steps, conj = [3, 0, 0], [False, False, True]
    h = eng.to_host
    for L in (L0, L0 - 1):
        mext = level_chain(mtop, key_L0, L, k)
        q = mext[:L]
        assert mext[L:] == mtop[key_L0:] and mext != mtop[:L + k]          # the special primes sit key_L0 - L rows further down

        def key_pair():
            level = E.key_rows(rng, "lazy", mext, level_digits(L, alpha), n)
            top = embed_key(H.lazy_uniform(fill, (level_digits(key_L0, alpha), 2, key_L0 + k, n), mtop), level, key_L0, L, k, alpha)
            assert np.array_equal(sub_key(top, key_L0, L, k, alpha), level)
            return eng.to_device(top), eng.to_device(level), level

        pt = M.lazy_rows(rng, (BATCH, L, n), q)
        d_pt = eng.to_device(pt)
        d_a, d_b = (eng.to_device(M.lazy_rows(rng, (BATCH, 2, L, n), q)) for _ in range(2))
        d_quad = eng.mult_low_level(q, d_a, d_b)
        (top, sub, level_key), rots = key_pair(), [key_pair() for _ in steps]
        tops, subs = [x[0] for x in rots], [x[1] for x in rots]

        def run():
            at = dict(key_L0=key_L0)
            return [(h(eng.bgv_hks_switch(mext, t, k, alpha, d_pt, top, **at)), h(eng.bgv_hks_switch(mext, t, k, alpha, d_pt, sub))),
                    (h(eng.bgv_rotate_hoisted_hks(mext, t, k, alpha, d_a, tops, steps, conj, **at)),
                     h(eng.bgv_rotate_hoisted_hks(mext, t, k, alpha, d_a, subs, steps, conj))),
                    (h(eng.bgv_relin_modswitch_hks(mext, t, k, alpha, d_quad, top, **at)),
                     h(eng.bgv_relin_modswitch_hks(mext, t, k, alpha, d_quad, sub))),
                    (h(eng.bgv_mult_hks(mext, t, k, alpha, d_a, d_b, top, **at)), h(eng.bgv_mult_hks(mext, t, k, alpha, d_a, d_b, sub))),
                    (h(eng.hks_switch(mext, k, alpha, d_pt, top, **at)), h(eng.hks_switch(mext, k, alpha, d_pt, sub))),
                    (h(eng.ckks_rotate_hoisted_hks(mext, k, alpha, d_a, tops, steps, conj, **at)),
                     h(eng.ckks_rotate_hoisted_hks(mext, k, alpha, d_a, subs, steps, conj))),
                    (h(eng.ckks_mult_hks(mext, k, alpha, d_a, d_b, top, **at)), h(eng.ckks_mult_hks(mext, k, alpha, d_a, d_b, sub)))]

        if logn <= 6:
            with modelled():
                exp = [B.model_switch_bgv(orc, logn, mext, L, k, alpha, t, pt[b], level_key) for b in range(BATCH)]
        for level, pairs in at_both_levels(eng, run).items():
            for i, (got, want) in enumerate(pairs):
                assert got.shape == want.shape and np.array_equal(got, want), (level, L, i)
            if logn <= 6:
                for b in range(BATCH):
                    assert residues_match(pairs[0][0][b], exp[b], q), (level, L, b)


# ---- 5. the dot ------------------------------------------------------------------------------------------------------------------------------
def dot_is_the_model(orc, got, case, mext, a, b, key):
    name, logn, L, k, alpha = case
    qm = mext[:L - 1]
    assert below_2q(got, qm)
    for p in range(got.shape[0]):
        with modelled():
            exp = model_dot(orc, logn, mext, L, k, alpha, [x[p] for x in a], [x[p] for x in b], key)
        assert got[p].shape == exp.shape
        assert np.array_equal(strict_rows(got[p], qm), strict_rows(exp, qm)), p


@pytest.mark.parametrize("case", E.DOT_CASES, ids=case_id)
def test_dot_matches_the_exact_model(eng, orc, case):
    """T = 3 lazy operands; and T = 1: the residues of the fused multiplication on the same operands"""
    name, logn, L, k, alpha = case
    mext, n, T = E.chain_of(name, L, k), 1 << logn, 3
    q, Bn = mext[:L], BATCH
    rng = SplitMix(E.seed_of(case, 400))
    a = [M.lazy_rows(rng, (Bn, 2, L, n), q) for _ in range(T)]
    b = [M.lazy_rows(rng, (Bn, 2, L, n), q) for _ in range(T)]
    key = E.key_rows(rng, "lazy", mext, E.nd_of(L, alpha), n)
    d_a, d_b, d_key = [eng.to_device(x) for x in a], [eng.to_device(x) for x in b], eng.to_device(key)
    got = at_both_levels(eng, lambda: (eng.to_host(eng.ckks_dot_hks(mext, k, alpha, d_a, d_b, d_key)),
                                       eng.to_host(eng.ckks_dot_hks(mext, k, alpha, d_a[:1], d_b[:1], d_key)),
                                       eng.to_host(eng.ckks_mult_hks(mext, k, alpha, d_a[0], d_b[0], d_key))))
    dot_is_the_model(orc, got["B"][0], case, mext, a, b, key)
    qm = mext[:L - 1]
    for level, (dot, one, mult) in got.items():
        assert below_2q(dot, qm) and np.array_equal(strict_rows(dot, qm), strict_rows(got["B"][0], qm)), level
        assert below_2q(one, qm) and np.array_equal(strict_rows(one, qm), strict_rows(mult, qm)), level


@pytest.mark.parametrize("case", E.DOT_CASES + E.DOT_WORD_CASES, ids=case_id)
def test_dot_is_its_two_halves_word_for_word(eng, case):
    """the sum into a caller's quad, then the exposed tail: the same code on the same quad, the same WORDS -- on HIGHMID too, where
    hehub's rescale is no function of the residues (hks_bgv_edges.drop_premise) and no model is held against the call"""
    name, logn, L, k, alpha = case
    mext, n, T = E.chain_of(name, L, k), 1 << logn, 3
    q = mext[:L]
    rng = SplitMix(E.seed_of(case, 450))
    d_a = [eng.to_device(M.lazy_rows(rng, (BATCH, 2, L, n), q)) for _ in range(T)]
    d_b = [eng.to_device(M.lazy_rows(rng, (BATCH, 2, L, n), q)) for _ in range(T)]
    d_key = eng.to_device(E.key_rows(rng, "lazy", mext, E.nd_of(L, alpha), n))

    def run():
        quad = eng.ckks_tensor_sum(q, d_a, d_b)
        return eng.to_host(eng.ckks_dot_hks(mext, k, alpha, d_a, d_b, d_key)), eng.to_host(eng.ckks_relin_rescale_hks(mext, k, alpha, quad, d_key))

    for level, (dot, tail) in at_both_levels(eng, run).items():
        assert dot.shape == (BATCH, 2, L - 1, n) and below_2q(dot, mext[:L - 1]), level
        assert np.array_equal(dot, tail), level


def test_dot_of_the_largest_words_at_the_largest_term_count_of_one_launch(eng, orc, ts):  # noqa: F811
    """WIDE58, every operand and key word 2q - 1, T = hpi::tensor_sum_max_terms for the chain (the engine's own host rule, through
    tests/cpp/tensor_sum_shim.cpp): the largest sum one launch of k_tensor_sum forms, then the switch.  The ABI refuses no term count
    (include/hehub_amd.h: one launch per tensor_sum_max_terms terms, the next ones adding to the quad): T + 1 is a second launch of
    one term on top of the largest words the first can leave, and is held to the model too; the refusal that does exist -- no terms --
    leaves the output at its fill pattern."""
    import ctypes as C

    from hehub_amd import capi

    case = E.DOT_MAX_CASE
    name, logn, L, k, alpha = case
    mext, n = E.chain_of(name, L, k), 1 << logn
    q = mext[:L]
    T = ts(q)
    assert T == TABLE and 2 * T * (2 * max(q) - 1) ** 2 <= ((1 << 64) - max(q)) * (1 << 64) - 1
    x = H.max_rows((1, 2, L, n), q)
    key = H.max_rows((E.nd_of(L, alpha), 2, L + k, n), mext)
    dx, d_key = eng.to_device(x), eng.to_device(key)
    for terms in (T, T + 1):
        got = eng.to_host(eng.ckks_dot_hks(mext, k, alpha, [dx] * terms, [dx] * terms, d_key))
        dot_is_the_model(orc, got, case, mext, [x] * terms, [x] * terms, key)
    out = eng.empty((1, 2, L - 1, n))
    out.fill_(7)
    one = (capi.P * 1)(dx.data_ptr())
    rc = eng.lib.hp_dev_ckks_dot_relin_rescale_hks(eng.h, logn, L, k, alpha, (capi.u64 * (L + k))(*mext), 1, 0, one, one,
                                                   C.c_void_p(d_key.data_ptr()), C.c_void_p(out.data_ptr()))
    assert rc == capi.HP_EINVAL
    eng.sync()
    assert (eng.to_host(out) == 7).all()


# ---- 6. by decryption, with keys made on the device from error rows t * e ---------------------------------------------------------------------
@pytest.mark.parametrize("case", E.DECRYPT_CASES, ids=case_id)
def test_mult_of_two_encryptions_decrypts_to_the_product(eng, orc, case):
    name, logn, L, k, alpha = case
    mext, n, t = E.chain_of(name, L, k), 1 << logn, T0
    q, nd = mext[:L], E.nd_of(L, alpha)
    rng = SplitMix(E.seed_of(case, 500))
    with modelled():
        s = B.ternary(rng, n)
        msgs = [np.array([int(v) for v in rng.words(n, t)], dtype=object) for _ in range(2 * BATCH)]
        ct_a = np.stack([B.encrypt_bgv(orc, rng, q, t, s, m) for m in msgs[:BATCH]])
        ct_b = np.stack([B.encrypt_bgv(orc, rng, q, t, s, m) for m in msgs[BATCH:]])
        s2 = B.negacyclic_ntt(orc, q, s, s)
    rows = eng.poly_from_signed(mext, dev_i64(eng, np.stack([np.array([int(v) for v in x], dtype=np.int64) for x in (s, s2)])))
    uniform = eng.to_device(rng.poly((1, nd, L + k, n), mext))
    errors = dev_i64(eng, (t * B.small_errors(rng, nd * n)).reshape(1, nd, n))      # the BGV recipe: error rows t * e
    d_key = eng.hks_keygen(mext, k, alpha, rows[0], rows[1:], uniform, errors)[0]
    d_a, d_b = eng.to_device(ct_a), eng.to_device(ct_b)
    got = at_both_levels(eng, lambda: eng.to_host(eng.bgv_mult_hks(mext, t, k, alpha, d_a, d_b, d_key)))
    with modelled():
        want = [B.negacyclic_ntt(orc, q, msgs[b], msgs[BATCH + b], t) for b in range(BATCH)]
        for level, mult in got.items():
            assert mult.shape == (BATCH, 2, L - 1, n)
            for b in range(BATCH):
                assert np.array_equal(B.decrypt_bgv(orc, q[:-1], t, s, mult[b]), want[b]), (level, b)
                assert not np.array_equal(want[b], msgs[b])
