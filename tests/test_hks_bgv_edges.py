"""The inputs of tests/test_gpu_hks_bgv_moduli.py held to their own conditions with the models alone (no GPU), so that a failure on the
GPU means the engine and not the case:
  * every chain is a chain for its degree, and every (chain, degree) pair passes the premise the exact models rest on
    (hks_bgv_edges.premise: hehub's fold wraps neither for the strict rows the model transforms nor for the lazy words the device hands
    the inverse transforms of the special primes and of q_last) -- and the pairs left out of the case lists do fail it;
  * the transforms really are congruent to the true ones there: round trips and representatives of the same residues;
  * hks_edges.covers holds exactly where hks_bgv_edges says it does, and in every case that decrypts;
  * every plain modulus is below every modulus of its chain;
  * the planted accumulators hit every class on the wide chains;
  * the max fill's digit-loop sums, recomputed with Python integers, stay below 2^128 (printed: how close they come);
  * hks_bgv_model's own identities hold on WIDE58 at (4, 4, 2, 2) -- tests/test_hks_bgv_model.py holds them on the table chain."""
import numpy as np
import pytest

import hks_bgv_edges as E
import hks_bgv_model as B
import hks_edges as H
import moduli as M
import params as P
from hks_levels import level_chain
from oracle.pyoracle import SplitMix

U = np.uint64


def at_levels():
    """(name, logn, L, k, alpha, chain) of every level an _at case is called at"""
    out = []
    for name, logn, key_L0, L, k, alpha in E.AT_CASES:
        mtop = E.at_chains(name, key_L0, k)
        out += [(name, logn, lv, k, alpha, level_chain(mtop, key_L0, lv, k)) for lv in (L, L - 1)]
    return out


def chains_in_use():
    return [c + (E.chain_of(c[0], c[2], c[3]),) for c in E.every_case()] + at_levels()


def test_every_chain_is_a_chain_for_its_degree():
    assert len(E.every_case()) >= 25
    for name, logn, L, k, alpha, mext in chains_in_use():
        assert len(mext) == L + k and len(set(mext)) == L + k, (name, L, k)
        for q in mext:
            assert P.is_prime(q) and M.log_modulus(q) <= 59 and M.max_logn(q) >= logn, (name, q)
        assert 1 <= alpha <= 8 and 1 <= k <= 8 and E.nd_of(L, alpha) <= 16 and L + k <= 32
    for name, logn, key_L0, L, k, alpha in E.AT_CASES:
        assert key_L0 == L + 2 and L % alpha != 0 and (L - 1) % alpha == 0            # partial last digit at L, full at L - 1
    # the chains keep what they are named for
    assert M.Q59 == E.chain_of("W59LAST", 4, 2)[3] and all(q.bit_length() == 40 for q in E.chain_of("W59LAST", 4, 2)[:3])
    assert M.FAMILIES[58]["high_mid"] in E.chain_of("WIDE58", 3, 2) and M.Q59 in E.chain_of("W59", 3, 2)
    assert min(E.chain_of(*E.NARROW_CASE[:1], *E.NARROW_CASE[2:4])).bit_length() == 20
    assert all(M.fold_consts(q)[2] > q >> 3 for q in E.chain_of("HIGHMID", 2, 3)[:1] + E.chain_of("HIGHMID", 2, 3)[2:4])   # high_mid: large delta
    assert M.level_a_chain(E.chain_of(*E.LEVEL_A_CASE[:1], *E.LEVEL_A_CASE[2:4]), E.LEVEL_A_CASE[1])
    assert not any(M.level_a_chain(mext, logn) for name, logn, L, k, alpha, mext in chains_in_use() if (name, logn) != E.LEVEL_A_CASE[:2])


def test_every_case_passes_the_premise_of_the_exact_models():
    for name, logn, L, k, alpha, mext in chains_in_use():
        assert E.premise(mext, L, logn), (name, logn, L, k, [q for q in mext if M.fold_bound(q, 2 * q, logn)[0]])
    for name, logn, L, k, alpha in E.PREMISE_FAILS:           # what is left out is left out for this reason
        assert not E.premise(E.chain_of(name, L, k), L, logn), name
        assert (name, logn, L, k, alpha) not in E.every_case()
    assert not E.premise(E.chain_of("LOWMID", 4, 2), 4, 5)   # (why the chains are swept at N = 16)


def test_the_transforms_are_the_true_ones_where_the_premise_holds(orc):
    """what the premise is for, observed: the round trip returns the strict row, and two representatives of the same residues (the
    model's strict words, the device's lazy ones) have congruent inverse transforms -- at every modulus of every (chain, degree) used"""
    seen = set()
    for name, logn, L, k, alpha, mext in chains_in_use():
        for j, q in enumerate(mext):
            if (q, logn, j >= L - 1) in seen:
                continue
            seen.add((q, logn, j >= L - 1))
            rng = SplitMix(q % 9973 + logn)
            n = 1 << logn
            for kind in ("strict", "max"):
                x = M.edge_words(rng, kind, q, n) % U(q)
                y = orc.ntt(logn, q, x)
                assert np.array_equal(orc.intt(logn, q, y) % U(q), x), (name, q, logn)
                if j >= L - 1:     # lazy words reach this modulus' inverse transform on the device
                    s = y % U(q)
                    lazy = s + U(q) * (np.arange(n) % 2).astype(U)
                    assert (lazy < U(2 * q)).all()
                    assert np.array_equal(orc.intt(logn, q, lazy) % U(q), orc.intt(logn, q, s) % U(q)), (name, q, logn)
                    assert np.array_equal(orc.intt(logn, q, s) % U(q), x), (name, q, logn)


def q_of(case):
    return E.chain_of(case[0], case[2], case[3])[:case[2]]


def test_every_case_that_ends_in_a_drop_passes_the_drop_premise():
    for c in E.RELIN_CASES + E.DOT_CASES + [E.DOT_MAX_CASE] + E.DECRYPT_CASES:
        assert E.drop_premise(q_of(c), c[1]), c
    for c in E.DROP_FAILS + E.DOT_WORD_CASES:                # what is left out of the model comparisons is left out for this reason
        assert not E.drop_premise(q_of(c), c[1]), c
        assert c not in E.RELIN_CASES + E.DOT_CASES + E.DECRYPT_CASES
    # WIDE58R is WIDE58 with the high_mid prime as q_last, where the drop centres and divides by it
    for shape in (E.FIRST, E.TILED, (5, 4, 2, 2)):
        wide, turned = E.chain_of("WIDE58", shape[1], shape[2]), E.chain_of("WIDE58R", shape[1], shape[2])
        assert sorted(wide[:shape[1]]) == sorted(turned[:shape[1]]) and wide[shape[1]:] == turned[shape[1]:]
        assert turned[shape[1] - 1] == M.FAMILIES[58]["high_mid"] == wide[0]
    assert M.Q59 == q_of(("W59LAST",) + E.FIRST)[-1]


def drop_inputs(c):
    q, n = q_of(c), 1 << c[1]
    rng = SplitMix(E.seed_of(c, 600))
    strict = rng.poly((2, len(q), n), q)
    return q, strict, strict + np.array(q, dtype=U)[:, None] * rng.words(strict.size, 2).reshape(strict.shape).astype(U)


@pytest.mark.parametrize("case", E.RELIN_CASES, ids=lambda c: "-".join(map(str, c)))
def test_hehubs_drop_is_the_exact_drop_where_the_drop_premise_holds(orc, case):
    """the model's last step (oracle.bgv_mod_drop) against Python integers, on canonical words and on lazy ones"""
    q, strict, lazy = drop_inputs(case)
    for t in E.plain_moduli(case)[:1 if case[1] > 6 else 3]:
        exact = E.exact_mod_drop(orc, case[1], q, t, strict)
        for words in (strict, lazy):
            got = orc.bgv_mod_drop(q, t, np.ascontiguousarray(words))
            assert (got < 2 * np.array(q[:-1], dtype=U)[:, None]).all()
            assert np.array_equal((got % np.array(q[:-1], dtype=U)[:, None]).astype(object), exact), (case, t)


def test_hehubs_drop_is_not_exact_at_a_high_mid_limb_below_the_last(orc):
    """why DROP_FAILS is left out: on HIGHMID at N = 2048 hehub's own mod switch of CANONICAL words misses (x - rem) / q_last on most
    coefficients of the high_mid limb, and only there"""
    case = ("HIGHMID",) + E.TILED
    q, strict, lazy = drop_inputs(case)
    exact = E.exact_mod_drop(orc, case[1], q, E.T0, strict)
    for words in (strict, lazy):
        got = orc.bgv_mod_drop(q, E.T0, np.ascontiguousarray(words))
        wrong = [[int(((got[h, m] % U(q[m])).astype(object) != exact[h, m]).sum()) for m in range(len(q) - 1)] for h in range(2)]
        print("HIGHMID N = 2048: residues of hehub's drop that are not the exact ones, per (polynomial, limb):", wrong)
        assert all(row[0] > 256 and row[1] == 0 for row in wrong)
    assert M.fold_consts(q[0])[2] > q[0] >> 3 and M.fold_consts(q[1])[2] < q[1] >> 16     # limb 0 is the high_mid one


def test_covers_holds_where_it_is_said_to_and_wherever_something_decrypts():
    for c in E.every_case():
        name, logn, L, k, alpha = c
        assert H.covers(E.chain_of(name, L, k), L, k, alpha) == (c not in E.UNCOVERED), c
    assert set(E.UNCOVERED) <= set(E.every_case())
    assert not set(E.DECRYPT_CASES) & set(E.UNCOVERED) and E.EDGE_T_CASE not in E.UNCOVERED
    for name, logn, key_L0, L, k, alpha in E.AT_CASES:
        mtop = E.at_chains(name, key_L0, k)
        for lv in (L, L - 1):
            assert H.covers(level_chain(mtop, key_L0, lv, k), lv, k, alpha) == ((name, logn, key_L0, L, k, alpha) not in E.UNCOVERED_AT)


def test_every_plain_modulus_is_below_every_modulus():
    for c in E.every_case():
        mext = E.chain_of(c[0], c[2], c[3])
        ts = (2,) if c == E.NARROW_CASE else E.plain_moduli(c)
        assert all(0 < t < min(mext) for t in ts), c
    assert min(E.chain_of("NARROW", 3, 2)) < max(B.PLAIN_MODULI)   # (why NARROW is not in the t-sweep: t < every modulus)
    mext = E.chain_of(E.EDGE_T_CASE[0], E.EDGE_T_CASE[2], E.EDGE_T_CASE[3])
    t = E.edge_t(mext)
    assert t % 2 == 1 and t == min(mext) - 2 and t.bit_length() == 58 and all(q % t for q in mext)
    for name, logn, key_L0, L, k, alpha in E.AT_CASES:
        assert E.T0 < min(E.at_chains(name, key_L0, k))


@pytest.mark.parametrize("case", E.PLANTED_CASES, ids=lambda c: c[0])
def test_the_planted_accumulators_hit_every_class(case):
    name, logn, L, k, alpha = case
    mext = E.chain_of(name, L, k)
    ts = E.plain_moduli(case) + ((E.edge_t(mext),) if case == E.EDGE_T_CASE else ())
    assert len(ts) >= 3
    for t in ts:
        w = E.planted(case, t)
        found = B.planted_classes(w, mext, L, k, t)
        assert len(found) == 12 and all(found.values()), (t, [c for c, ok in found.items() if not ok])
        assert all(0 <= x < B.prod(mext) for row in w for x in row)


@pytest.mark.parametrize("case", E.MAX_CASES, ids=lambda c: c[0])
def test_max_fill_sums_fit_the_accumulator(orc, case):
    """every ciphertext and key word 2q - 1: the digit loop's sum_d digit * key with Python integers, against the 128-bit register"""
    name, logn, L, k, alpha = case
    mext, worst = E.max_fill_sums(orc, case)
    room = E.report_max_fill(case, mext, worst)
    assert worst["inner"][0] < 1 << 128 and room > 0
    assert worst["word"][0] < 1 << 64
    # inside a digit the row is the caller's own word: (2q - 1)^2 is among the sums at every ciphertext modulus
    assert worst["inner"][0] >= max((2 * q - 1) ** 2 for q in mext[:L])


# ---- hks_bgv_model's identities on a wide chain ---------------------------------------------------------------------------------------
WIDE = E.EDGE_T_CASE          # WIDE58, (4, 4, 2, 2)


def wide_ts():
    mext = E.chain_of(WIDE[0], WIDE[2], WIDE[3])
    return B.PLAIN_MODULI + (E.edge_t(mext),)


@pytest.mark.parametrize("t", wide_ts())
def test_moddown_t_divides_exactly_and_keeps_the_value_mod_t_on_a_wide_chain(t):
    name, logn, L, k, alpha = WIDE
    mext = E.chain_of(name, L, k)
    Q, Pm = B.prod(mext[:L]), B.prod(mext[L:])
    rng = SplitMix(11 + t % 1000)
    xs = [x for row in E.planted(WIDE, t) for x in row] + [B.crt_all([int(rng.words(1, m)[0]) for m in mext], mext) for _ in range(64)]
    for x in xs:
        d = B.delta_of(x, t, Pm)
        y = B.mod_down_int(x, t, Pm)                    # (asserts that P divides x - delta)
        assert y * Pm + d == x and d % t == 0 and 2 * abs(d) <= t * (Pm + 1)
        assert (y * Pm - x) % t == 0                    # the quotient keeps x's value mod t (up to the unit P)
    assert max(2 * abs(B.delta_of(x, t, Pm)) for x in xs) == t * (Pm + 1)


@pytest.mark.parametrize("t", wide_ts())
def test_planted_key_and_model_agree_with_plain_arithmetic_on_a_wide_chain(orc, t):
    name, logn, L, k, alpha = WIDE
    mext = E.chain_of(name, L, k)
    w = E.planted(WIDE, t)
    key = B.planted_key(orc, logn, mext, L, k, alpha, w)
    got = B.model_switch_bgv(orc, logn, mext, L, k, alpha, t, B.planted_pt(L, 1 << logn), key)
    assert np.array_equal(got, B.planted_expected(orc, logn, mext, L, k, t, w))


@pytest.mark.parametrize("t", wide_ts())
def test_keygen_switch_and_decryption_return_the_message_on_a_wide_chain(orc, t):
    name, logn, L, k, alpha = WIDE
    mext, n = E.chain_of(name, L, k), 1 << logn
    q = mext[:L]
    rng = SplitMix(500 + t % 1000)
    s, s_old = B.ternary(rng, n), B.ternary(rng, n)
    msg = np.array([int(v) for v in rng.words(n, t)], dtype=object)
    ct = B.encrypt_bgv(orc, rng, q, t, s_old, msg)
    assert np.array_equal(B.decrypt_bgv(orc, q, t, s_old, ct), msg)
    key = B.keygen_bgv(orc, rng, logn, mext, L, k, alpha, t, s, s_old)
    sw = B.model_switch_bgv(orc, logn, mext, L, k, alpha, t, ct[1], key)
    for m in range(L):
        sw[0, m] = (sw[0, m] + ct[0, m].astype(object)) % q[m]
    assert np.array_equal(B.decrypt_bgv(orc, q, t, s, sw.astype(U)), msg)
    # and the multiplication: mult + relin + mod switch decrypts to the negacyclic product (on WIDE58R: the drop premise)
    mext = E.chain_of("WIDE58R", L, k)
    q = mext[:L]
    m2 = np.array([int(v) for v in rng.words(n, t)], dtype=object)
    ct1, ct2 = B.encrypt_bgv(orc, rng, q, t, s, msg), B.encrypt_bgv(orc, rng, q, t, s, m2)
    out = B.model_mult_bgv(orc, logn, mext, L, k, alpha, t, ct1, ct2, B.keygen_bgv(orc, rng, logn, mext, L, k, alpha, t, s, B.negacyclic(s, s)))
    assert np.array_equal(B.decrypt_bgv(orc, q[:-1], t, s, out.astype(U)), B.negacyclic(msg, m2, t))
