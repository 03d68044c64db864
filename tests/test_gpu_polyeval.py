"""hp_dev_ckks_eval_plan_hks: straight-line plans of steps E_{s+1} = rescale(relin(sum_t X_t (x) Y_t) + Z) over the hybrid key switch.

Pinned four ways:
  * a step against the calls it is composed of, WORD for word: one product of pass-through forms is hp_dev_ckks_mult_relin_rescale_hks_at,
    several products are hp_dev_ckks_dot_relin_rescale_hks_at on the materialised forms, no product is hp_dev_ckks_lincomb followed by
    hp_dev_ckks_rescale;
  * whole plans of hehub_amd/polyeval.py against the exact model (tests/polyeval_model.py), on strict residues with every word below
    2q, at both parity levels;
  * end to end: secret, relinearisation key and ciphertexts from the seeded device calls, a Chebyshev polynomial of degree 15 on a
    batch of four values, decrypted exactly;
  * every refusal returns its code and leaves the output untouched."""
import ctypes as C

import numpy as np
import pytest
from numpy.polynomial import chebyshev as Ch

import moduli as M
import params as P
from dot_model import below_2q, strict_rows
from hehub_amd import capi
from hehub_amd.polyeval import Form, Plan, build_plan
from hks_model import chain
from oracle.pyoracle import SplitMix
from polyeval_model import CHEB15, DELTA, E2E, E2E_THRESHOLD, POWER7, decrypt_error, model_plan

pytestmark = pytest.mark.gpu
U = np.uint64
E0 = Form([(0, None)])   # the input, as it lies


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def setting(seed, logn, L, key_L0, k, alpha, B=1):
    """the top chain, an input batch [B][2][L][n] of lazy words and a top-shaped key of any words"""
    mext = chain(key_L0, k)
    n = 1 << logn
    rng = SplitMix(seed)
    ct = M.lazy_rows(rng, (B, 2, L, n), mext[:L])
    key = rng.poly(((key_L0 + alpha - 1) // alpha, 2, key_L0 + k, n), mext)
    return mext, mext[:L] + mext[key_L0:], ct, key, rng


def one_step(q, level, products, z):
    plan = Plan(q, 1)
    plan.add(level, products, z, 1)
    return plan


@pytest.mark.parametrize("logn,L,key_L0,k,alpha", [(4, 3, 3, 1, 1), (5, 4, 6, 2, 2), (11, 3, 4, 2, 2), (12, 4, 4, 1, 3)])
def test_one_product_of_pass_through_forms_is_the_fused_multiplication(eng, logn, L, key_L0, k, alpha):
    mext, lext, ct, key, _ = setting(9800 + logn, logn, L, key_L0, k, alpha, B=2)
    d_ct, d_key = eng.to_device(ct), eng.to_device(key)
    got = eng.to_host(eng.ckks_poly_eval_hks(lext, k, alpha, d_ct, d_key, one_step(mext[:L], L, [(E0, E0)], Form()), key_L0=key_L0))
    assert np.array_equal(got, eng.to_host(eng.ckks_mult_hks(lext, k, alpha, d_ct, d_ct, d_key, key_L0=key_L0)))


@pytest.mark.parametrize("logn,L,key_L0,k,alpha,T", [(5, 4, 5, 2, 2, 2), (11, 3, 3, 2, 2, 3), (11, 3, 4, 2, 2, 33)])
def test_several_products_are_the_lazy_dot_product(eng, logn, L, key_L0, k, alpha, T):
    """X_t = c_t E_0 (materialised by the lincomb kernel), Y_t = E_0 (by address): the words of ckks_dot_hks on those operands"""
    mext, lext, ct, key, rng = setting(9900 + logn + T, logn, L, key_L0, k, alpha)
    q = mext[:L]
    cs = [int(rng.words(1, 1 << 39)[0]) - (1 << 38) for _ in range(T)]          # integers of either sign
    d_ct, d_key = eng.to_device(ct), eng.to_device(key)
    plan = one_step(q, L, [(Form([(0, c)]), E0) for c in cs], Form())
    got = eng.to_host(eng.ckks_poly_eval_hks(lext, k, alpha, d_ct, d_key, plan, key_L0=key_L0))
    xs = [eng.ckks_lincomb(q, [d_ct], [[c % m for m in q]]) for c in cs]
    assert np.array_equal(got, eng.to_host(eng.ckks_dot_hks(lext, k, alpha, xs, [d_ct] * T, d_key, key_L0=key_L0)))


@pytest.mark.parametrize("logn,L,level", [(4, 3, 2), (11, 4, 4), (12, 5, 3)])
def test_a_step_without_a_product_is_lincomb_and_rescale(eng, logn, L, level):
    mext, lext, ct, key, rng = setting(10000 + logn, logn, L, L, 1, 1, B=2)
    q = mext[:level]
    c, cst = int(rng.words(1, 1 << 40)[0]), -int(rng.words(1, 1 << 60)[0])
    d_ct = eng.to_device(ct)
    got = eng.to_host(eng.ckks_poly_eval_hks(lext, 1, 1, d_ct, eng.to_device(key), one_step(mext[:L], level, [], Form([(0, c)], cst))))
    lin = eng.ckks_lincomb(q, [d_ct], [[c % m for m in q]], [cst % m for m in q])
    assert got.shape == (2, 2, level - 1, 1 << logn)
    assert np.array_equal(got, eng.to_host(eng.ckks_rescale(q, lin)))


def test_z_is_added_before_the_switch_and_final_drops_follow(eng, orc):
    """one step with a product AND a Z form over an operand of more limbs than the level, then two final drops: the model's residues"""
    logn, L, key_L0, k, alpha = 5, 5, 5, 2, 2
    mext, lext, ct, key, _ = setting(10100, logn, L, key_L0, k, alpha)
    plan = one_step(mext[:L], 4, [(Form([(0, 3)], 11), E0)], Form([(0, -5)], 1 << 70))
    plan.final_drops = 2
    got = eng.to_host(eng.ckks_poly_eval_hks(lext, k, alpha, eng.to_device(ct), eng.to_device(key), plan))
    exp = model_plan(orc, logn, mext, key_L0, k, alpha, key, plan, ct[0])
    assert got.shape == (1, 2, 1, 1 << logn) and below_2q(got, mext[:1])
    assert np.array_equal(strict_rows(got[0], mext[:1]), strict_rows(exp, mext[:1]))


COEFS = {"power": POWER7, "chebyshev": CHEB15}
WHOLE = {"power42": ("power", 7, 4, 4, 5, 5, 1, 1), "cheb44": ("chebyshev", 15, 4, 5, 7, 8, 2, 2), "cheb42": ("chebyshev", 7, 4, 11, 6, 6, 2, 2)}
_cache = {}


def whole_case(orc, name):
    """(mext, lext, ct, key, plan, the model's output) of a whole-plan case, computed once"""
    if name not in _cache:
        basis, degree, n1, logn, L, key_L0, k, alpha = WHOLE[name]
        mext, lext, ct, key, _ = setting(10200 + logn, logn, L, key_L0, k, alpha)
        plan = build_plan(COEFS[basis][:degree + 1], basis, mext[:L], DELTA, DELTA, n1=n1)
        _cache[name] = (mext, lext, ct, key, plan, model_plan(orc, logn, mext, key_L0, k, alpha, key, plan, ct[0]))
    return _cache[name]


def matches_model(got, case):
    mext, plan, exp = case[0], case[4], case[5]
    qo = mext[:plan.out_limbs]
    assert got.shape[1:] == exp.shape and below_2q(got, qo)
    assert np.array_equal(strict_rows(got[0], qo), strict_rows(exp, qo))


@pytest.mark.parametrize("name", list(WHOLE))
def test_whole_plans_match_the_exact_model(eng, orc, name):
    """power (4,2) at (logn 4, L 5, k 1, alpha 1); Chebyshev (4,4) at (5, 7, 2, 2) under a key for 8 moduli; Chebyshev (4,2) at
    (11, 6, 2, 2), where every step takes the merged ModDown + rescale"""
    case = whole_case(orc, name)
    k, alpha, key_L0 = WHOLE[name][6], WHOLE[name][7], WHOLE[name][5]
    got = eng.to_host(eng.ckks_poly_eval_hks(case[1], k, alpha, eng.to_device(case[2]), eng.to_device(case[3]), case[4], key_L0=key_L0))
    matches_model(got, case)


def test_whole_plan_at_parity_level_a(eng, orc):
    """the linear forms and the quadratic sums are integer arithmetic at both levels; the tails run on the FP64 kernels: the residues of
    the level-B model, every word below 2q, and the range guard stays quiet (sync would report HP_ERANGE)"""
    case = whole_case(orc, "cheb42")
    eng.set_parity_level("A")
    try:
        assert eng.parity_level() == "A"
        got = eng.to_host(eng.ckks_poly_eval_hks(case[1], 2, 2, eng.to_device(case[2]), eng.to_device(case[3]), case[4], key_L0=6))
        eng.sync()
    finally:
        eng.set_parity_level("B")
    matches_model(got, case)


def test_end_to_end_chebyshev_on_device_made_keys_and_ciphertexts(eng, orc):
    """logn 11, L 7, a key set for 8 moduli (polyeval_model.E2E): the secret (hp_dev_sample_small_ntt), the relinearisation key
    (hp_dev_hks_keygen_seeded with s_from = s^2) and the ciphertexts (hp_dev_rlwe_encrypt_seeded of the constants round(x_b Delta)) are
    made on the device; the degree-15 Chebyshev plan decrypts, exactly, to Delta p(x_b) within E2E_THRESHOLD = 920: 8 x the error the
    exact model measures for this plan at this ring degree and these values (tests/test_polyeval_model.py: 115).  Measured on the
    device: 57 .. 93."""
    logn, L, key_L0, k, alpha = (E2E[v] for v in ("logn", "L", "key_L0", "k", "alpha"))
    n, mext = 1 << logn, chain(key_L0, k)
    q, lext = mext[:L], mext[:L] + mext[key_L0:]
    seed = bytes(range(32))
    s = eng.sample_small_ntt(logn, mext, 2, seed, 1)                                   # ternary, [1][E][n]
    key = eng.hks_keygen_seeded(mext, k, alpha, s[0], eng.poly_mul(mext, s, s), seed, 100)[0]
    xs = list(E2E["xs"])
    ms = [int(round(x * DELTA)) for x in xs]
    pt = np.zeros((len(xs), L, n), dtype=U)
    for b, v in enumerate(ms):
        pt[b, :, 0] = [v % m for m in q]
    ct = eng.rlwe_encrypt_seeded(q, s[0, :L].contiguous(), eng.to_device(pt), seed, 1000)
    plan = build_plan(CHEB15, "chebyshev", q, DELTA, DELTA, n1=E2E["n1"])
    assert plan.out_limbs == 2 and plan.switches == 6
    out = eng.to_host(eng.ckks_poly_eval_hks(lext, k, alpha, ct, key, plan, key_L0=key_L0))
    qo, s_host = q[:2], eng.to_host(s)[0]
    for b, v in enumerate(ms):
        exp = int(round(float(Ch.chebval(v / DELTA, CHEB15)) * DELTA))
        err = decrypt_error(orc, qo, s_host, strict_rows(out[b], qo), exp)
        print(f"x = {xs[b]}: |dec - Delta p(x)| <= {err} = 2^{np.log2(max(err, 1)):.2f} (2^{np.log2(max(err, 1)) - 40:.1f} of Delta), threshold {E2E_THRESHOLD}")
        assert err < E2E_THRESHOLD


def test_refusals_enqueue_nothing(eng):
    logn, L, k, alpha = 4, 4, 1, 2
    mext, lext, ct, key, _ = setting(10300, logn, L, L, k, alpha)
    n, q = 1 << logn, mext[:L]
    d_ct, d_key = eng.to_device(ct), eng.to_device(key)
    out = eng.empty((1, 2, L - 1, n))
    out.fill_(7)
    mod = (capi.u64 * (L + k))(*lext)
    keep = []

    def call(plan, dst=None, ct_=None, key_=None, steps=None, final_drops=0, L_=L, key_L0=L, batch=1, alpha_=alpha, raw=None):
        arr, k2 = plan.marshal() if raw is None else (raw, None)
        keep.append((arr, k2))
        return eng.lib.hp_dev_ckks_eval_plan_hks(eng.h, logn, L_, key_L0, k, alpha_, mod, batch, len(plan.steps) if steps is None else steps, arr,
                                                 final_drops, C.c_void_p(d_ct.data_ptr() if ct_ is None else ct_),
                                                 C.c_void_p(d_key.data_ptr() if key_ is None else key_), C.c_void_p(out.data_ptr() if dst is None else dst))

    sq = lambda level=L: one_step(q, level, [(E0, E0)], Form())
    assert call(sq()) == capi.HP_OK                                           # the call as such is fine
    eng.sync()
    out.fill_(7)
    EINVAL = capi.HP_EINVAL
    assert call(sq(), dst=0) == EINVAL and call(sq(), ct_=0) == EINVAL and call(sq(), key_=0) == EINVAL
    assert call(sq(), dst=out.data_ptr() + 8) == EINVAL and call(sq(), ct_=d_ct.data_ptr() + 8) == EINVAL
    assert call(sq(), raw=None, steps=0) == EINVAL
    long = Plan(q, 1)
    long.steps, long.limbs = sq().steps * 65, [L] * 66
    assert call(long) == EINVAL                                               # more than 64 steps
    low = sq()
    low.steps[0].level = 1
    assert call(low) == EINVAL                                                # level < 2
    two = Plan(q, 1)
    two.add(L, [(E0, E0)], Form(), 1)
    two.add(L - 1, [(Form([(1, None)]), Form([(1, None)]))], Form(), 1)
    assert call(two, dst=out.data_ptr()) == capi.HP_OK                        # (L - 2 limbs: fits the sentinel buffer)
    eng.sync()
    out.fill_(7)
    two.steps[1].level = L                                                    # element 1 has L - 1 limbs
    assert call(two) == EINVAL
    two.steps[1].level = L - 1
    two.steps[0].products[0] = (Form([(1, None)]), E0)                        # a forward reference
    assert call(two) == EINVAL
    high = sq()
    high.steps[0].level = L + 1
    assert call(high) == EINVAL                                               # a level above the input's limb count
    empty = sq()
    empty.steps[0].products[0] = (Form(), E0)
    assert call(empty) == EINVAL                                              # an X form with no term
    idle = one_step(q, L, [], Form([(0, 3)]))
    idle.steps[0].z = Form()
    assert call(idle) == EINVAL                                               # neither a product nor a term

    class Residue(Plan):   # a plan whose constants are NOT reduced: a residue equal to its modulus reaches the call
        def marshal(self):
            arr, k2 = Plan.marshal(self)
            bad = (capi.u64 * L)(*q)
            if self.bad_cst:
                arr[0].z.cst = C.cast(bad, C.POINTER(capi.u64))
            else:
                arr[0].z.term[0].coef = C.cast(bad, C.POINTER(capi.u64))
            return arr, (k2, bad)

    for bad_cst in (False, True):
        r = Residue(q, 1)
        r.add(L, [(E0, E0)], Form([(0, 5)], 9), 1)
        r.bad_cst = bad_cst
        assert call(r) == EINVAL
    assert call(sq(), final_drops=L - 1) == EINVAL                            # leaves no limb
    assert call(sq(), dst=d_ct.data_ptr()) == EINVAL                          # the output is the input
    assert call(sq(), dst=d_ct.data_ptr() + (2 * L * n - 2) * 8) == EINVAL    # ... or begins in its last 16 bytes
    # what the _at calls refuse, with their code
    assert call(sq(), batch=0) == EINVAL and call(sq(), alpha_=0) == EINVAL and call(sq(), key_L0=L - 1) == EINVAL
    assert call(sq(), L_=0) == EINVAL and call(sq(), key_L0=32) == EINVAL
    leaf = one_step(q, L, [], Form([(0, 3)]))                                 # ... also where no step of the plan switches
    assert call(leaf, alpha_=0) == EINVAL and call(leaf, key_L0=L - 1) == EINVAL and call(leaf, key_L0=32) == EINVAL
    eng.sync()
    assert (eng.to_host(out) == 7).all()
    with pytest.raises(ValueError):                                           # the front end reports it as the reference's invalid_argument
        eng.ckks_poly_eval_hks(lext, k, alpha, d_ct, d_key, high)
