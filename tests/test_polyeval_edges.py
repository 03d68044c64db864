"""The cases of tests/test_gpu_polyeval_moduli.py held to their own conditions with the models alone (no GPU), so that a failure on the
GPU means the engine and not the case:
  * every chain is a chain for its degree, and every (case, logn, step level) that is held against polyeval_model.model_plan passes
    hks_bgv_edges.premise and drop_premise -- nothing is skipped at run time; the chains without such a model (polyeval_edges.DROP_FAILS,
    PREMISE_FAILS) do fail, for the reason written there;
  * every plan has 5 steps and 4 switches and no constant that rounds to 0 (printed: largest_constant_bits per case);
  * the planted lincomb residues are there, and every coefficient is a residue;
  * the accumulate maximum of section 3(b) is within the premise of hpi::lincomb_max_terms for its chain, in Python integers and through
    the host function itself (tests/cpp/lincomb_shim.cpp, the fixture of tests/test_lincomb_host.py);
  * the decryption error of the end-to-end case, measured in the model alone at both ring degrees: what polyeval_edges.DECRYPT_MEASURED
    records and the device test's threshold is 8 x of."""
import numpy as np
import pytest

import hks_bgv_edges as E
import hks_edges as H
import moduli as M
import params as P
import polyeval_edges as PE
from dot_model import strict_rows
from hks_levels import level_chain
from hks_model import centred, keygen
from oracle.pyoracle import SplitMix
from polyeval_model import POWER7, decrypt_error, encrypt_constant, model_plan
from test_lincomb_host import TABLE, lc  # noqa: F401  (the fixture around hpi::lincomb_max_terms)

U = np.uint64


def forms_of(plan):
    return [f for s in plan.steps for f in [g for xy in s.products for g in xy] + [s.z]]


def test_every_chain_is_a_chain_for_its_degree():
    chains = [(name, max(PE.LOGNS), PE.plan_chain(name)) for name in PE.PLAN_CASES]
    chains += [(name, max(PE.LOGNS), PE.top_chain(name, PE.PLAN_CASES[name][0] + 1)) for name in PE.TOP_KEY_PLANS]
    chains += [(name, 13 if name == PE.LINCOMB_FULL_TILES[0] else 11, PE.lincomb_chain(name)[0]) for name in PE.LINCOMB_CHAINS]
    chains += [(c[0], c[1], E.chain_of(c[0], PE.step_key_L0(c), c[3])) for c in PE.STEP_CASES]
    for name, logn, mext in chains:
        assert len(set(mext)) == len(mext) <= 32, name
        for q in mext:
            assert P.is_prime(q) and M.log_modulus(q) <= 59 and M.max_logn(q) >= logn, (name, q)
    widths = lambda name: [q.bit_length() for q in PE.plan_chain(name)]
    assert widths("W59") == [59] + [40] * 5 + [50] and widths("W59LAST") == [40] * 5 + [59, 50, 50]
    assert widths("ABOVE") == [45, 41, 42, 46, 37, 31, 50] and widths("PACKEDGE") == [59, 46, 47, 47, 48, 48, 50]
    assert all(w in (58, 59, 60) for w in widths("WIDE58R")) and PE.plan_chain("WIDE58R")[4] == M.FAMILIES[58]["high_mid"]
    assert all(q.bit_length() in (58, 59, 60) for q in PE.lincomb_chain("WIDE58")[0])
    top, L = PE.lincomb_chain("W59LAST")
    assert top[L - 1] == M.Q59
    for name in PE.LINCOMB_CHAINS:                          # operands with 0, 1 and 2 more limbs exist on every chain
        top, L = PE.lincomb_chain(name)
        assert L >= 2 and L + max(PE.LINCOMB_EXTRA) <= len(top), name
    for name in PE.TOP_KEY_PLANS:
        L, k = PE.PLAN_CASES[name][:2]
        assert level_chain(PE.top_chain(name, L + 1), L + 1, L, k) == PE.plan_chain(name)
    # the one (chain, degree) that level A serves: at every level of its plan below the top one (at level 6 the 31-bit limb takes
    # strict rows of the 50-bit prime, its fold may wrap, and the context keeps level B for that step: four of the five steps run at A)
    name, logn = PE.LEVEL_A_PLAN
    L, k = PE.PLAN_CASES[name][:2]
    assert PE.step_levels(name) == [3, 4, 5, 6]
    for lv in PE.step_levels(name):
        assert M.level_a_chain(level_chain(PE.plan_chain(name), L, lv, k), logn) == (lv < L), lv
    assert not any(M.level_a_chain(PE.plan_chain(other), 11) for other in PE.PLAN_CASES if other != name)


def test_every_modelled_level_passes_the_premises():
    cases = PE.modelled_levels()
    assert len(cases) >= 2 * 4 * len(PE.PLAN_CASES)
    for name, logn, lv, mext in cases:
        assert E.premise(mext, lv, logn), (name, logn, lv, [q for q in mext if M.fold_bound(q, 2 * q, logn)[0]])
        assert E.drop_premise(mext[:lv], logn), (name, logn, lv)
    for name in PE.TOP_KEY_PLANS:                           # the same levels read from the longer top chain
        L, k = PE.PLAN_CASES[name][:2]
        top = PE.top_chain(name, L + 1)
        for lv in PE.step_levels(name):
            assert level_chain(top, L + 1, lv, k) == level_chain(PE.plan_chain(name), L, lv, k)
    # the decryption case: another alpha on a chain already in the list
    assert PE.decrypt_chain() == PE.plan_chain(PE.DECRYPT["name"]) and H.covers(PE.decrypt_chain(), PE.DECRYPT["L"], 1, PE.DECRYPT["alpha"])
    assert not H.covers(PE.plan_chain("WIDE58R"), 5, 1, PE.PLAN_CASES["WIDE58R"][2])           # alpha = 2, k = 1: residues only
    # what has no model that ends in hehub's drop, and why
    for name in PE.DROP_FAILS:
        for logn, L, k, alpha in PE.STEP_SHAPES:
            q = E.chain_of(name, L, k)[:L]
            assert all(not E.drop_premise(q[:lv], logn) for lv in range(2, L + 1)), (name, logn)
        assert name not in PE.PLAN_CASES and name not in PE.Z_CHAINS and name in PE.STEP_CHAINS
    for name in PE.PREMISE_FAILS:
        assert E.premise(E.chain_of(name, 4, 2), 4, 4) and not any(E.premise(E.chain_of(name, 4, 2), 4, logn) for logn in (5, 11))
        assert name not in PE.PLAN_CASES and name not in PE.STEP_CHAINS and name in PE.LINCOMB_CHAINS


def test_every_plan_has_its_shape_and_no_constant_rounds_to_zero():
    for name in PE.PLAN_CASES:
        plan = PE.plan_of(name)
        L = PE.PLAN_CASES[name][0]
        assert len(plan.steps) == 5 and plan.switches == 4 and plan.in_limbs == L and plan.out_limbs >= 1, name
        consts = [c for f in forms_of(plan) for c in [c for _, c in f.terms] + [f.cst] if c is not None]
        assert consts and all(c != 0 for c in consts), name
        assert max(abs(c).bit_length() for c in consts) == plan.largest_constant_bits > 64, name
        print(f"{name}: {len(consts)} constants, largest_constant_bits = {plan.largest_constant_bits}")
    d = PE.decrypt_plan()
    assert len(d.steps) == 5 and d.switches == 4 and d.out_limbs == 1
    for name in PE.Z_CHAINS:
        L = PE.PLAN_CASES[name][0]
        two, top = PE.z_two_launch_plan(name, SplitMix(1)), PE.z_max_plan(name)
        assert two.steps[0].level == L - 1 and len(two.steps[0].z.terms) == PE.TABLE + 1 and two.steps[0].z.cst is not None
        assert top.steps[0].level == L and len(top.steps[0].z.terms) == PE.TABLE
        q = PE.plan_chain(name)[:L]
        assert all(c % m == m - 1 for _, c in top.steps[0].z.terms for m in q) and all(top.steps[0].z.cst % m == m - 1 for m in q)


def test_the_lincomb_inputs_hold_what_they_say():
    for name in PE.LINCOMB_CHAINS:
        for T in PE.LINCOMB_TERMS:
            q, cts, coefs, cst = PE.lincomb_inputs(name, 4, T)
            L = len(q)
            assert len(cts) == len(coefs) == T and [x.shape[2] - L for x in cts[:3]] == list(PE.LINCOMB_EXTRA[:T])
            assert all(0 <= c < m for row in coefs + [cst] for c, m in zip(row, q))
            assert cst[0] == q[0] - 1
            flat = [(c, m) for row in coefs + [cst] for c, m in zip(row, q)]
            if T > 1:
                assert any(c == 0 for c, m in flat) and any(c == 1 for c, m in flat) and any(c == m - 1 for c, m in flat), (name, T)
                assert any(c not in (0, 1, m - 1) for c, m in flat)
            for x in cts:                                     # moduli.lazy_rows: strict words, words in [q, 2q), some 2q - 1
                top = np.array(PE.lincomb_chain(name)[0][:x.shape[2]], dtype=U)[:, None]
                assert (x < 2 * top).all() and (x >= top).any() and (x == 2 * top - U(1)).any() and (x < top).any()
    vals = [PE.signed(SplitMix(7 + i)) for i in range(64)]
    assert min(vals) < -(1 << 96) and max(vals) > 1 << 96 and all(abs(v) <= 1 << 99 for v in vals)


def test_the_accumulate_maximum_is_within_the_range_function(lc):  # noqa: F811
    """3(b): 32 terms of (2q - 1)(q - 1), the constant q - 1 and an accumulated word below 2q -- the sum lincomb_max_terms budgets as
    T (q - 1)(2q - 1) + 3q -- at every modulus of the three chains, with the whole table allowed by the host function"""
    for name in PE.Z_CHAINS:
        L = PE.PLAN_CASES[name][0]
        q = PE.plan_chain(name)[:L]
        for lv in (L - 1, L):
            assert lc(q[:lv]) == TABLE == PE.TABLE, (name, lv)
        for m in q:
            assert PE.accumulate_max(m) <= TABLE * (m - 1) * (2 * m - 1) + 3 * m <= PE.montgomery_limit(m) < 1 << 128, (name, m)
        assert PE.report_accumulate_max(name) > 0
    for name in PE.LINCOMB_MAX_CHAINS:
        top = PE.lincomb_chain(name)[0]
        assert lc(top) == TABLE and all(PE.accumulate_max(m) <= PE.montgomery_limit(m) for m in top)
    assert M.log_modulus(max(PE.plan_chain("WIDE58R")[:5])) == 59    # 2^59 + small: the widest moduli the engine takes


@pytest.mark.parametrize("logn", PE.LOGNS)
def test_the_decryption_case_in_the_model_alone(orc, logn):
    """the end-to-end case of tests/test_gpu_polyeval_moduli.py with a model-made key and noise: the measurement that
    polyeval_edges.DECRYPT_MEASURED records (the threshold is 8 x it, here and on the device)"""
    d = PE.DECRYPT
    L, k, alpha, delta = d["L"], d["k"], d["alpha"], d["delta"]
    mext, n = PE.decrypt_chain(), 1 << logn
    q = mext[:L]
    plan = PE.decrypt_plan()
    rng = SplitMix(11900 + logn)
    s = rng.words(n, 3).astype(np.int64) - 1
    s_ntt = orc.poly_reduce_strict(q, orc.poly_ntt(q, np.stack([(s % m).astype(U) for m in q])))
    key = keygen(orc, rng, logn, mext, L, k, alpha, s, centred(orc, q, orc.poly_mul(q, s_ntt, s_ntt)))
    worst = 0
    for x in d["xs"]:
        v = int(round(x * delta))
        out = model_plan(orc, logn, mext, L, k, alpha, key, plan, encrypt_constant(orc, rng, q, s_ntt, v, n))
        worst = max(worst, decrypt_error(orc, q[:1], s_ntt, strict_rows(out, q[:1]), PE.exact_power(POWER7, v, delta)))
    lg = np.log2(max(worst, 1))
    print(f"power (4,2) on WIDE58R, logn {logn}: max |dec - Delta p(x)| = {worst} = 2^{lg:.2f} (2^{lg - 58:.1f} of Delta); recorded "
          f"{PE.DECRYPT_MEASURED[logn]}, threshold {PE.DECRYPT_THRESHOLD[logn]}")
    assert worst == PE.DECRYPT_MEASURED[logn]               # the model is deterministic: the record IS the measurement
    assert 0 < worst < PE.DECRYPT_THRESHOLD[logn]
