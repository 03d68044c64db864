"""The inputs of tests/test_gpu_hks_moduli.py held to their own conditions with the model alone (no GPU): the chains are usable, the
wide chain is what it claims to be, and for the extremal-row and accumulator-edge cases the sums that k_hks_inner_lintrans and
k_hks_bsgs_presum form (hp_hks.hip) are recomputed with Python integers from the words the device reads -- the caller's own words
inside a digit, the oracle's lazy transform of the lifted value elsewhere -- and asserted to fit their registers:
    the digit sum and the sum over the rotations / babies below 2^128, the word between them below 2^64.
Each case prints the measured figures next to hpi::hks_lintrans_max_rotations' premise (word w = 4 nd ceil(q^2 / 2^64) + 3q, sum w 2q R).

What the figures say (WIDE58, 16 digits, 32 rotations):
  * The premise "digit word below 2q" behind that w does NOT hold at level B: the lifted rows are hehub's lazy transform words, and at
    the 58-bit high_mid modulus they reach 2.73 q at N = 32 and 4.24 q at N = 1024 (moduli.fold_bound allows 3.25 q and 5.25 q).
  * The sums fit all the same: digit sum at most 2^123.97, word at most 2^60.85 (still under w = 2^61.32, because only the high_mid
    limbs have such rows and they are 0.8 * 2^59), sum over the rotations / babies at most 2^125.50 against the premise's 2^126.32 and the
    register's 2^128.  With fold_bound's largest word for any modulus the transforms accept (log_modulus <= 59, N <= 65536: 10.9 q
    at q = 2^58.5) the same arithmetic gives 2^125.4, 2^61.9 and 2^126.4: hks_lintrans_max_rotations needs no change.
  * The carry out of the middle carry-save column (hp_device.h: cx) fires in these cases and never on the table chains."""
import numpy as np
import pytest

import hks_edges as H
import moduli as M
import params as P
from hks_model import chain, crt, model_lintrans, model_rest, rotations_of
from oracle.pyoracle import SplitMix
from test_gpu_moduli import LEVEL_A_CHAINS

U = np.uint64
pytestmark = []          # (the module this one borrows LEVEL_A_CHAINS from is a GPU module; this one is not)


def shapes_in_use():
    out = [(name, logn, L, k, alpha) for name in H.MODEL_CHAINS for logn, L, k, alpha in H.MODEL_SHAPES]
    out += [(name,) + H.EXTREMAL_SHAPE for name in H.EXTREMAL_CHAINS] + [(name,) + H.ALL_MAX_SHAPE for name in H.EXTREMAL_CHAINS]
    out += [("WIDE58", logn) + H.EDGE_SHAPE for logn, _ in H.EDGE_CASES] + [("W59", logn, 3, 2, 2) for logn in H.CHUNK_LOGNS]
    out += [(name, 12) + shape for name, shape in H.LEVEL_B_ONLY_SHAPES.items()] + [(name, 11, 3, 2, 2) for name in H.CROSS_CHAINS]
    return out


def test_every_chain_is_a_chain():
    for name, logn, L, k, alpha in shapes_in_use():
        mext = H.chain_of(name, L, k)
        assert len(mext) == L + k and len(set(mext)) == L + k, (name, L, k)
        for q in mext:
            assert P.is_prime(q) and M.log_modulus(q) <= 59 and M.max_logn(q) >= logn, (name, q)
        assert (L + alpha - 1) // alpha <= 16 and L + k <= 32
    for name in H.MODEL_CHAINS[:-1]:            # the cut keeps what the chain is named for
        chain_ = M.CHAINS[name]
        for _, L, k, _ in H.MODEL_SHAPES:
            assert H.cut(name, L, k)[:min(L, len(chain_) - 1)] == chain_[:min(L, len(chain_) - 1)]
    assert M.LOWMID_Q in H.cut("LOWMID", 3, 2) and M.Q59 in H.cut("W59", 3, 2)


def test_level_a_follows_the_shapes_chosen():
    for name, (L, k, alpha) in H.LEVEL_A_SHAPES.items():
        c = LEVEL_A_CHAINS[name]
        mext = c[:L] + c[-k:]
        assert len(set(mext)) == L + k and M.level_a_chain(mext, 11), name
    for name, (L, k, alpha) in H.LEVEL_B_ONLY_SHAPES.items():
        assert not M.level_a_chain(H.cut(name, L, k), 12), name


@pytest.mark.parametrize("L,k,alpha", [(4, 2, 2), (5, 2, 2), (3, 2, 2), (2, 2, 2), (16, 2, 1)])
def test_wide58_is_wide_off_the_table_and_covered(L, k, alpha):
    mext = H.wide58(L, k)
    table = set(P.P40 + P.P50)
    assert len(set(mext)) == L + k and not table & set(mext)
    assert H.covers(mext, L, k, alpha)
    kinds = set()
    for q in mext:
        kb, fix, delta = M.fold_consts(q)
        assert q.bit_length() in (59, 60) and kb == 59 or (q.bit_length() in (58, 59) and kb == 58)
        kinds.add((kb, fix, delta > (1 << 50)))
    # just below and just above 2^58 and 2^59, and the 58-bit high_mid position (kb = 59, fix = 0, large delta)
    want = {(59, 1, False), (59, 0, True), (59, 0, False), (58, 1, False), (58, 0, False)}
    assert kinds <= want and (kinds == want or L + k < 5)
    assert M.FAMILIES[58]["high_mid"] in mext and (L + k < 5 or {M.FAMILIES[w][p] for w in (58, 59) for p in ("below", "above")} <= set(mext))


def fits(name, worst, mext, nd, R):
    """the registers' conditions; returns the host premise's (word, sum) for the caller's remarks"""
    w, s = H.report(name, worst, mext, nd, R)
    assert worst["inner"][0] < 1 << 128, (name, "digit sum", worst["inner"])
    assert worst["word"][0] < 1 << 64, (name, "word", worst["word"])
    assert worst["outer"][0] < 1 << 128, (name, "outer sum", worst["outer"])
    return w, s


# ---- case 2: extremal rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.EXTREMAL_CHAINS)
def test_extremal_rows_fit(orc, name):
    logn, L, k, alpha = H.EXTREMAL_SHAPE
    c = H.flat_inputs(name, logn, L, k, alpha, 1, 3, "kinds", 8200)
    fits(f"{name} kinds", H.flat_sums(orc, c), c["mext"], 2, 3)


@pytest.mark.parametrize("name", H.EXTREMAL_CHAINS)
def test_all_max_rows_reach_the_contracts_largest_digit_sum_and_fit(orc, name):
    """one digit: on a ciphertext modulus the digit sum is (2q - 1)^2, the largest product the contract allows, in every rotation"""
    for what, c, worst in (("flat", *(lambda c: (c, H.flat_sums(orc, c)))(H.all_max_flat(name))),
                           ("pre-sum", *(lambda c: (c, H.presum_sums(orc, c)))(H.all_max_bsgs(name)))):
        mext, L = c["mext"], c["L"]
        fits(f"{name} all max, {what}", worst, mext, 1, H.TABLE)
        assert worst["inner"][0] >= max((2 * q - 1) ** 2 for q in mext[:L])
        if name != "HIGHMID":                   # (41- to 51-bit moduli: below the width at which the carry can fire)
            assert worst["cx_outer"][0] >= 1, (name, what)


# ---- case 3: the accumulator edge -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,fill", H.EDGE_CASES)
def test_accumulator_edge_fits(orc, logn, fill):
    L, k, alpha = H.EDGE_SHAPE
    nd = L
    c = H.edge_flat(logn, fill)
    worst = H.flat_sums(orc, c)
    w, s = fits(f"WIDE58 logn {logn} {fill}, flat", worst, c["mext"], nd, H.TABLE)
    # the premise of the host formula's word: digit words below 2q.  It fails at the high_mid limbs; the word it bounds still holds.
    assert worst["ratio"][0] > 2 and M.fold_consts(c["mext"][worst["ratio"][1][0]])[2] > 1 << 50
    assert worst["word"][0] < w and worst["outer"][0] < s
    if logn <= 6:
        # (the digit sum's column carries at most twice over 16 digits of 60-bit words: it takes the all-max keys of "edge" to get there)
        assert worst["cx_outer"][0] >= 1 and (fill != "edge" or worst["cx_inner"][0] >= 1)
    cb = H.edge_bsgs(logn, fill)
    worst = H.presum_sums(orc, cb)
    w, s = fits(f"WIDE58 logn {logn} {fill}, pre-sum", worst, cb["mext"], nd, H.TABLE)
    assert worst["word"][0] < w and worst["outer"][0] < s
    if logn <= 6:
        assert worst["cx_outer"][0] >= 1


def test_the_table_chains_never_carry(orc):
    """the gap the wide chain closes: with 40- and 50-bit moduli no cross term reaches the carry (a word below 2^51 has a high half below 2^19: 16 digits or 32
    rotations of cross terms below 2^52 stay below 2^57), here at the full table"""
    logn, L, k, alpha, R = 4, 9, 2, 1, H.TABLE         # (nine digits: the table's 40-bit row is ten primes long)
    mext, n = chain(L, k), 1 << logn
    key, dg = H.max_rows((L, 2, L + k, n), mext), H.max_rows((L + k, n), mext)
    ct = H.max_rows((2, L, n), mext[:L])
    steps, conj = rotations_of(logn, R)
    worst = H.sums(orc, logn, mext, L, k, alpha, ct, [(key, s, c) for s, c in zip(steps, conj)], [[dg] * R])
    assert worst["cx_inner"][0] == 0 and worst["cx_outer"][0] == 0


# ---- the sampled model is the model -------------------------------------------------------------------------------------------------
def test_sampled_model_is_the_model(orc):
    logn, L, k, alpha, R = 5, 5, 2, 2, 5
    c = H.flat_inputs("WIDE58", logn, L, k, alpha, 1, R, "kinds", 8500)
    keys, diags = H.pick(c["kpool"], c["which"]), H.pick(c["dpool"], c["wd"])
    keys[0] = None                              # an identity term, as the BSGS call's identity baby
    full = model_lintrans(orc, logn, c["mext"], L, k, alpha, c["ct"][0], keys[1:], c["steps"][1:], c["conj"][1:], diags[1:])
    w = diags[0].astype(object)
    for h in range(2):
        for m in range(L):
            full[h, m] = (full[h, m] + w[m] * c["ct"][0][h, m].astype(object)) % c["mext"][m]
    sel = np.arange(1 << logn)
    assert np.array_equal(H.sampled_lintrans(orc, logn, c["mext"], L, k, alpha, c["ct"][0], keys, [0] + c["steps"][1:], c["conj"], diags, sel), full)
    sel = np.array([0, 3, 17, 31])
    got = H.sampled_lintrans(orc, logn, c["mext"], L, k, alpha, c["ct"][0], keys, [0] + c["steps"][1:], c["conj"], diags, sel)
    assert np.array_equal(got, full[:, :, sel])


# ---- ModDown is exact where hehub's transform words exceed 2q -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["HIGHMID", "WIDE58"])
def test_model_moddown_is_exact_at_high_mid_moduli(orc, name):
    """model_rest (the model every hybrid GPU test is held to) against ModDown written with Python integers alone:
        out_i = (x_i - [x]_P) * P^-1 mod q_i,   [x]_P the centred value of the special-prime part, coefficient by coefficient.
    At a high_mid modulus the lazy transform of the remainder has words of 2q and more; hehub's lazy subtraction takes its operand below
    2q and wraps on them (70 % of the words of such a limb at N = 2048), so the remainder's words are brought below 2q first
    (hks_model.below_2q; hp_lazy_below_2q on the device).  Without that this test fails on the high_mid limbs only."""
    logn, L, k = 11, 3, 2
    mext, n, E = H.chain_of(name, L, k), 1 << logn, L + k
    q, pm = mext[:L], mext[L:]
    A = SplitMix(8600).poly((2, E, n), mext)
    unit = np.zeros((2, 2, E, n), dtype=U)
    for m in range(E):
        unit[0, 0, m, :] = unit[1, 1, m, :] = (1 << 64) % mext[m]
    got = model_rest(orc, logn, mext, L, k, A, unit)
    pprod = pm[0] * pm[1]
    wide = False
    for h in range(2):
        coef = orc.poly_reduce_strict(mext, orc.poly_intt(mext, np.ascontiguousarray(A[h])))
        r = [(lambda y: y if y < pprod // 2 else y - pprod)(crt([coef[L + j][i] for j in range(k)], pm)[0]) for i in range(n)]
        for m in range(L):
            rem_words = orc.ntt(logn, q[m], np.array([x % q[m] for x in r], dtype=U))
            wide = wide or bool((rem_words >= U(2 * q[m])).any())
            pinv = pow(pprod % q[m], -1, q[m])
            want = orc.ntt(logn, q[m], np.array([(int(coef[m][i]) - r[i]) * pinv % q[m] for i in range(n)], dtype=U)) % U(q[m])
            assert (got[h, m] < U(2 * q[m])).all()
            assert np.array_equal(got[h, m] % U(q[m]), want), (name, h, m, M.fold_consts(q[m]))
    assert wide          # (the case is about such words)
