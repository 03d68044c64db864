"""hp_dev_ckks_lincomb (hp_lincomb.hip: k_ct_lincomb) and hp_dev_ckks_eval_plan_hks (hp_api_eval.cpp, hehub_amd/polyeval.py) on wide and
off-table moduli: the chains of tests/moduli.py, WIDE58 (tests/hks_edges.py: every modulus 58 or 59 bits), W59LAST and WIDE58R
(tests/hks_bgv_edges.py).  tests/test_gpu_lincomb.py and tests/test_gpu_polyeval.py hold the same calls exact on 40-bit limbs and 50-bit
special primes, and every exact plan or step with a Z form at batch 1.  Here
  * every ciphertext batch is 2, so the output of a linear form is addressed with the stride of what it is written into -- 2 polynomials
    for a ciphertext, 3 for the (d0, d1) of a quad -- against an exact model;
  * a Z form is added to the quad by accumulating launches: 33 terms (two launches) over an element with more limbs than the step's
    level, and 32 terms of all-(2q - 1) words times q - 1 plus the constant q - 1 on top of the tensor product's words -- the largest sum
    an accumulating launch forms (tests/test_polyeval_edges.py: 2^124.000 at 2^59 + small, 15.5 x below the Montgomery step's limit);
  * r64 / r64h / mqinv belong to primes off the table: 58- and 59-bit limbs, 2^k + small, high_mid limbs, 20-bit limbs;
  * a plan's levels have different widths (PACKEDGE: 59, 46, 47, 47, 48, 48), so the per-level range functions and the level chain's
    addressing change from step to step; the plans' largest constants have 81 to 115 bits and are reduced into 59-bit limbs;
  * a whole plan runs at parity level A on the one off-table chain level A serves (ABOVE at N = 2048, below its top level).
The cases and inputs are those of tests/polyeval_edges.py; tests/test_polyeval_edges.py holds them to their own conditions without a GPU.
The models are tests/polyeval_model.py: model_lincomb word for word (the output is canonical), model_plan on strict residues with every
word below 2q, at parity level B and in a level-A context; a model is computed once per module and held against both.

What is modelled and what is not: HIGHMID and WIDE58 keep a high_mid limb through every drop (hks_bgv_edges.drop_premise fails: hehub's
rescale is no function of the residues there) and LOWMID's fold may wrap from N = 32 on (hks_bgv_edges.premise fails).  They run in
section 1 (pure integer arithmetic: no premise) and, HIGHMID and WIDE58, in section 2 against the engine's own calls, word for word;
sections 3 to 5, which end in hehub's drop, hold chains that pass both premises at every step's level.  Section 5 decrypts: secret and
relinearisation key through hp_dev_hks_keygen on host-drawn rows, ciphertexts from the model's encryption (not the seeded device
encryption, whose off-table behaviour is a separate matter), threshold 8 x the CPU model's own measurement at the same case.

What these cases found: no defect of the engine -- all 107 cases pass at both parity levels, and the device's decryption errors (3 at
N = 16, 41 and 42 at N = 2048) sit on the model's own (3, 42).  What they see that the suite could not, tried on scratch builds with one
defect planted each (counts of the 101 cases before 3(b) got its second fill): with `out_polys` replaced by 2 in k_ct_lincomb's `dst`
every exact test of tests/test_gpu_polyeval.py and tests/test_gpu_lincomb.py still passes (only the end-to-end noise threshold notices)
and 28 cases of sections 3 to 5 fail here; `accumulate || t0 != 0` cut to `t0 != 0` fails 22 cases here (3(a), 4, 5) and 6 of
test_gpu_polyeval.py; `old + cst` dropped from the odd word fails 93 cases here and both older modules.  The all-(2q - 1) fill of 3(b) is
a test of the RANGE of the sum, not of the accumulated word: there the quad's (d0, d1) are the constants 1 and 2, which the rescale
rounds away, so it passes without the accumulation (the second defect) and fails only if the sum wraps.  That is why 3(b) runs the
same step on lazy rows as well: those six cases fail on the second defect."""
import time

import numpy as np
import pytest

import hks_bgv_edges as E
import hks_bgv_model as B
import hks_edges as H
import moduli as M
import polyeval_edges as PE
from dot_model import below_2q, strict_rows
from gpu_words import at_both_levels, case_id, dev_i64
from hehub_amd.polyeval import Form, Plan
from hks_levels import embed_key, level_chain, level_digits
from oracle.pyoracle import SplitMix
from polyeval_model import POWER7, decrypt_error, encrypt_constant, model_lincomb, model_plan
from test_gpu_hks_bgv_moduli import mismatch

pytestmark = pytest.mark.gpu
U = np.uint64
BATCH, E0 = PE.BATCH, PE.E0
SPENT = {"model": 0.0, "start": None}


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    SPENT["start"] = time.perf_counter()
    yield e
    e.close()
    wall = time.perf_counter() - SPENT["start"]
    print(f"\ntest_gpu_polyeval_moduli: {SPENT['model']:.1f} s in the CPU models, {wall - SPENT['model']:.1f} s elsewhere (GPU, transfers, inputs)")


class modelled:
    """with modelled(): ... -- the time the exact models take, summed for the module's closing line"""

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        SPENT["model"] += time.perf_counter() - self.t0


def one_step(q, level, products, z):
    plan = Plan(q, 1)
    plan.add(level, products, z, 1)
    return plan


def holds_the_model(got, exp, q):
    """got: {parity level: [BATCH][2][len(q)][n] words}; exp[b]: the model's words -- the same residues, every word below 2q"""
    for level, g in got.items():
        assert g.shape == (BATCH,) + exp[0].shape and below_2q(g, q), level
        for b in range(BATCH):
            want = strict_rows(exp[b], q)
            assert np.array_equal(strict_rows(g[b], q), want), (level, b, mismatch(g[b], want, q))


# ---- 1. hp_dev_ckks_lincomb: pure integer arithmetic on every chain -----------------------------------------------------------------------
def lincomb_is_the_model(eng, name, logn, T):
    q, cts, coefs, cst = PE.lincomb_inputs(name, logn, T)
    n = 1 << logn
    with modelled():
        exp = [model_lincomb(q, [x[p] for x in cts], coefs, cst) for p in range(BATCH)]
    d = [eng.to_device(x) for x in cts]
    for level, got in at_both_levels(eng, lambda: eng.to_host(eng.ckks_lincomb(q, d, coefs, cst))).items():
        assert got.shape == (BATCH, 2, len(q), n)
        assert (got < np.array(q, dtype=U)[:, None]).all(), level              # every word canonical
        for p in range(BATCH):
            assert np.array_equal(got[p].astype(object), exp[p]), (level, p, mismatch(got[p], exp[p], q))


@pytest.mark.parametrize("T", PE.LINCOMB_TERMS)
@pytest.mark.parametrize("logn", PE.LOGNS)
@pytest.mark.parametrize("name", PE.LINCOMB_CHAINS)
def test_lincomb_matches_the_integer_model_on_every_chain(eng, name, logn, T):
    """operands of moduli.lazy_rows stored with 0, 1 and 2 limbs beyond L, batch 2; coefficients and the constant signed integers up
    to 2^100 reduced per limb, the residues 0, 1 and q - 1 planted; one term, a full table, a second launch: WORD for word"""
    lincomb_is_the_model(eng, name, logn, T)


def test_lincomb_on_full_tiles(eng):
    """N = 8192: rows of whole 2048-word tiles, 33 terms"""
    lincomb_is_the_model(eng, PE.LINCOMB_FULL_TILES[0], PE.LINCOMB_FULL_TILES[1], PE.TABLE + 1)


@pytest.mark.parametrize("logn", PE.LOGNS)
@pytest.mark.parametrize("name", PE.LINCOMB_MAX_CHAINS)
def test_largest_sum_of_a_launch_on_wide_and_on_narrow_limbs(eng, name, logn):
    """tests/test_gpu_lincomb.py's test_largest_sum_the_range_function_allows where EVERY limb is 58 or 59 bits wide, and on 20- and
    30-bit limbs: 32 terms of all-(2q - 1) words times q - 1 plus the constant q - 1, then one more term in a second launch"""
    q, n = PE.lincomb_chain(name)[0], 1 << logn
    dx = eng.to_device(H.max_rows((BATCH, 2, len(q), n), q))
    top = [m - 1 for m in q]
    for terms in (PE.TABLE, PE.TABLE + 1):
        for level, got in at_both_levels(eng, lambda: eng.to_host(eng.ckks_lincomb(q, [dx] * terms, [top] * terms, top))).items():
            for i, m in enumerate(q):
                assert (got[:, 0, i] == U((terms * (2 * m - 1) * (m - 1) + m - 1) % m)).all(), (level, terms, i)
                assert (got[:, 1, i] == U((terms * (2 * m - 1) * (m - 1)) % m)).all(), (level, terms, i)


# ---- 2. a step is the calls it is composed of, word for word ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", PE.STEP_CASES, ids=case_id)
def test_a_step_is_the_calls_it_is_composed_of(eng, case):
    """one product of pass-through forms: ckks_mult_hks; three products with materialised X forms c_t E_0: ckks_dot_hks on ckks_lincomb
    outputs; no product: ckks_lincomb, then ckks_rescale -- the same WORDS, every word below 2q, on HIGHMID and WIDE58 too, where the
    drop has no model.  On W59 and WIDE58 the plan reads a top-level key for key_L0 = L + 1 (the level key planted into words of
    another stream) and the composed calls its compact sub-key."""
    name, logn, L, k, alpha = case
    key_L0, n = PE.step_key_L0(case), 1 << logn
    mtop = E.chain_of(name, key_L0, k)
    mext = level_chain(mtop, key_L0, L, k)
    q = mext[:L]
    rng, fill = SplitMix(E.seed_of(case, 700)), SplitMix(E.seed_of(case, 777))
    d_ct = eng.to_device(M.lazy_rows(rng, (BATCH, 2, L, n), q))
    level_key = E.key_rows(rng, "lazy", mext, level_digits(L, alpha), n)
    top_key = level_key
    if key_L0 > L:
        top_key = embed_key(H.lazy_uniform(fill, (level_digits(key_L0, alpha), 2, key_L0 + k, n), mtop), level_key, key_L0, L, k, alpha)
    d_top, d_level = eng.to_device(top_key), eng.to_device(level_key)
    cs = [PE.signed(rng) for _ in range(3)]
    c, cst = PE.signed(rng), PE.signed(rng)
    res = lambda v: [v % m for m in q]
    plans = [one_step(q, L, [(E0, E0)], Form()), one_step(q, L, [(Form([(0, v)]), E0) for v in cs], Form()),
             one_step(q, L, [], Form([(0, c)], cst))]

    def run():
        h = eng.to_host
        steps = [h(eng.ckks_poly_eval_hks(mext, k, alpha, d_ct, d_top, p, key_L0=key_L0)) for p in plans]
        xs = [eng.ckks_lincomb(q, [d_ct], [res(v)]) for v in cs]
        return steps, [h(eng.ckks_mult_hks(mext, k, alpha, d_ct, d_ct, d_level)),
                       h(eng.ckks_dot_hks(mext, k, alpha, xs, [d_ct] * 3, d_level)),
                       h(eng.ckks_rescale(q, eng.ckks_lincomb(q, [d_ct], [res(c)], res(cst))))]

    for level, (steps, calls) in at_both_levels(eng, run).items():
        for i, (got, want) in enumerate(zip(steps, calls)):
            assert got.shape == want.shape == (BATCH, 2, L - 1, n) and below_2q(got, q[:-1]), (level, i)
            assert np.array_equal(got, want), (level, i, mismatch(got[0], want[0] % np.array(q[:-1], dtype=U)[:, None], q[:-1]))


# ---- 3. Z added to the quad ---------------------------------------------------------------------------------------------------------------
def z_is_the_model(eng, orc, name, logn, plan, ct):
    L, k, alpha = PE.PLAN_CASES[name][:3]
    mext, lext, _, key = PE.plan_inputs(name, logn)
    level = plan.steps[0].level
    with modelled():
        same = all(np.array_equal(ct[0], ct[b]) for b in range(1, BATCH))
        first = model_plan(orc, logn, mext, L, k, alpha, key, plan, ct[0])
        exp = [first] + [first if same else model_plan(orc, logn, mext, L, k, alpha, key, plan, ct[b]) for b in range(1, BATCH)]
    d_ct, d_key = eng.to_device(ct), eng.to_device(key)
    got = at_both_levels(eng, lambda: eng.to_host(eng.ckks_poly_eval_hks(lext, k, alpha, d_ct, d_key, plan)))
    assert exp[0].shape == (2, level - 1, 1 << logn)
    holds_the_model(got, exp, mext[:level - 1])


@pytest.mark.parametrize("logn", PE.LOGNS)
@pytest.mark.parametrize("name", PE.Z_CHAINS)
def test_z_of_two_launches_is_added_to_the_quad(eng, orc, name, logn):
    """(a) one product plus a Z of 33 terms and a constant at level L - 1 of an L-limb input: two launches of k_ct_lincomb, both
    accumulating into the 3-polynomial quad of a batch of two"""
    plan = PE.z_two_launch_plan(name, SplitMix(12100 + logn))
    z_is_the_model(eng, orc, name, logn, plan, PE.plan_inputs(name, logn)[2])


@pytest.mark.parametrize("fill", ["max", "lazy"])
@pytest.mark.parametrize("logn", PE.LOGNS)
@pytest.mark.parametrize("name", PE.Z_CHAINS)
def test_z_at_the_range_maximum_of_an_accumulating_launch(eng, orc, name, logn, fill):
    """(b) every input word 2q - 1, the step [(E0, E0)] with Z = 32 x (E0, q - 1) + the constant q - 1: a full table, the constant and
    the quad's own word in one accumulator (tests/test_polyeval_edges.py holds the sum to lincomb_max_terms' premise).  There the quad's
    (d0, d1) are the constants 1 and 2, which the rescale rounds away: fill "lazy" runs the same step -- a FIRST launch of a full table
    that accumulates -- on two different ciphertexts of moduli.lazy_rows, where dropping the accumulated word changes every residue."""
    L = PE.PLAN_CASES[name][0]
    q = PE.plan_chain(name)[:L]
    ct = H.max_rows((BATCH, 2, L, 1 << logn), q) if fill == "max" else PE.plan_inputs(name, logn)[2]
    z_is_the_model(eng, orc, name, logn, PE.z_max_plan(name), ct)


# ---- 4. whole plans ---------------------------------------------------------------------------------------------------------------------------
def whole_plan_is_the_model(eng, orc, name, logn, key_L0):
    L, k, alpha = PE.PLAN_CASES[name][:3]
    mtop, lext, ct, key = PE.plan_inputs(name, logn, key_L0)
    plan = PE.plan_of(name)
    with modelled():
        exp = [model_plan(orc, logn, mtop, key_L0, k, alpha, key, plan, ct[b]) for b in range(BATCH)]
    d_ct, d_key = eng.to_device(ct), eng.to_device(key)
    seen = []

    def run():
        seen.append(eng.parity_level())
        return eng.to_host(eng.ckks_poly_eval_hks(lext, k, alpha, d_ct, d_key, plan, key_L0=key_L0))

    got = at_both_levels(eng, run)          # (its sync reports HP_ERANGE, should the range guard of level A fire)
    assert seen == ["B", "A"]               # the level-A case (polyeval_edges.LEVEL_A_PLAN) did run in a level-A context
    assert exp[0].shape == (2, plan.out_limbs, 1 << logn) and not np.array_equal(exp[0], exp[1])
    holds_the_model(got, exp, mtop[:plan.out_limbs])


@pytest.mark.parametrize("logn", PE.LOGNS)
@pytest.mark.parametrize("name", list(PE.PLAN_CASES))
def test_whole_plans_match_the_exact_model(eng, orc, name, logn):
    """the table of tests/polyeval_edges.py: 5 steps, 4 switches, two different ciphertexts; ABOVE at logn 11 is the level-A case (its
    steps below the top level run on the FP64 kernels: the same residues, the range guard quiet)"""
    whole_plan_is_the_model(eng, orc, name, logn, PE.PLAN_CASES[name][0])


@pytest.mark.parametrize("logn", PE.LOGNS)
@pytest.mark.parametrize("name", PE.TOP_KEY_PLANS)
def test_whole_plans_under_a_key_for_one_more_modulus(eng, orc, name, logn):
    whole_plan_is_the_model(eng, orc, name, logn, PE.PLAN_CASES[name][0] + 1)


# ---- 5. by decryption ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", PE.LOGNS)
def test_power_plan_on_58_bit_limbs_decrypts_to_the_polynomial(eng, orc, logn):
    """WIDE58R (5, 1), alpha = 1, Delta = 2^58: the key made by hp_dev_hks_keygen from host-drawn uniform rows and errors, the
    ciphertexts by the model's encryption; |dec - Delta p(x)| below 8 x the CPU model's own measurement at this ring degree
    (polyeval_edges.DECRYPT_MEASURED: 3 at N = 16, 42 at N = 2048)"""
    d = PE.DECRYPT
    L, k, alpha, delta = d["L"], d["k"], d["alpha"], d["delta"]
    mext, n = PE.decrypt_chain(), 1 << logn
    q, nd = mext[:L], E.nd_of(L, alpha)
    assert H.covers(mext, L, k, alpha)
    plan = PE.decrypt_plan()
    rng = SplitMix(12200 + logn)
    vs = [int(round(x * delta)) for x in d["xs"]]
    with modelled():
        s = B.ternary(rng, n)
        s_ntt = B.to_ntt(orc, q, s)
        s2 = B.negacyclic_ntt(orc, q[:2], s, s)
        ct = np.stack([encrypt_constant(orc, rng, q, s_ntt, v, n) for v in vs])
    rows = eng.poly_from_signed(mext, dev_i64(eng, np.stack([np.array([int(v) for v in x], dtype=np.int64) for x in (s, s2)])))
    uniform = eng.to_device(rng.poly((1, nd, L + k, n), mext))
    errors = dev_i64(eng, B.small_errors(rng, nd * n).reshape(1, nd, n))
    d_key = eng.hks_keygen(mext, k, alpha, rows[0], rows[1:], uniform, errors)[0]
    d_ct = eng.to_device(ct)
    got = at_both_levels(eng, lambda: eng.to_host(eng.ckks_poly_eval_hks(mext, k, alpha, d_ct, d_key, plan)))
    with modelled():
        for level, out in got.items():
            assert out.shape == (len(vs), 2, 1, n) and below_2q(out, q[:1]), level
            for b, v in enumerate(vs):
                err = decrypt_error(orc, q[:1], s_ntt, strict_rows(out[b], q[:1]), PE.exact_power(POWER7, v, delta))
                print(f"level {level}, x = {d['xs'][b]}: |dec - Delta p(x)| <= {err} (model: {PE.DECRYPT_MEASURED[logn]}, threshold "
                      f"{PE.DECRYPT_THRESHOLD[logn]})")
                assert err < PE.DECRYPT_THRESHOLD[logn], (level, b)
