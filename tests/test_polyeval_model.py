"""tests/polyeval_model.py held to plain arithmetic, then a whole plan on real ciphertexts in the model alone (CPU tier).

The model is the reference of tests/test_gpu_polyeval.py: the device must reproduce its residues, so the model's decryption error IS
the device's.  A plan of hehub_amd/polyeval.py is run on encryptions of the constants round(x Delta) (keys: hks_model.keygen with a
ternary secret and s_from = s^2) and decrypted exactly (hks_model.centred):

  power basis, degree 7, (n1, n2) = (4, 2), logn 4, L 5, k 1, alpha 1, Delta = 2^40, x in (0.73, -0.5, 0.001):
      measured max |dec - Delta p(x)| over all coefficients = 2 (2^-39 of Delta)          POWER_MEASURED
      threshold = 8 x that                                                                 POWER_THRESHOLD = 16
  Chebyshev, degree 15, (4, 4), L 7, key_L0 8, k 2, alpha 2, at logn 4, x = 0.73:
      measured 5                                                                           CHEB16_MEASURED
      threshold = 8 x that                                                                 CHEB16_THRESHOLD = 40
  the same plan at logn 11 -- the shape AND the four values of the device's end-to-end test (polyeval_model.E2E):
      measured 115 (2^-33.2 of Delta)                                                      E2E_MEASURED
      threshold = 8 x that                                                                 E2E_THRESHOLD = 920
The device test uses E2E_THRESHOLD as it is: measured at its own ring degree, nothing is extrapolated.  (The error is the fresh
ciphertext's noise amplified by p', the roundings of the rescales and the switches' noise after ModDown; it grows about like sqrt(N).)
The constants live in tests/polyeval_model.py, which both test files import."""
import numpy as np
import pytest
from numpy.polynomial import chebyshev as Ch

import params as P
from dot_model import strict_rows
from hehub_amd.polyeval import build_plan
from hks_model import centred, chain, keygen
from oracle.pyoracle import SplitMix
from polyeval_model import (CHEB15, CHEB16_THRESHOLD, DELTA, E2E, E2E_THRESHOLD, POWER7, POWER_THRESHOLD, decrypt_error, encrypt_constant,
                            model_lincomb, model_plan)

U = np.uint64



def test_lincomb_model_is_schoolbook():
    q = P.P40[:2]
    rng = SplitMix(9500)
    a, b = rng.poly((2, 3, 4), P.P40[:3]), rng.poly((2, 2, 4), q)
    a[0, 0, 0] = 2 * q[0] - 1
    got = model_lincomb(q, [a, b], [[3, 5], None], [7, q[1] - 1])
    for h in range(2):
        for m in range(2):
            for i in range(4):
                exp = int(a[h, m, i]) * (3, 5)[m] + int(b[h, m, i]) + ((7, q[1] - 1)[m] if h == 0 else 0)
                assert got[h, m, i] == exp % q[m]
    neg = model_lincomb(q, [a], [-1], -1)     # integer constants of either sign, one for every limb
    assert neg[0, 1, 2] == (-int(a[0, 1, 2]) - 1) % q[1] and neg[1, 0, 1] == (-int(a[1, 0, 1])) % q[0]


def run_plan(orc, logn, L, key_L0, k, alpha, plan, xs, seed):
    """-> the worst decryption error over the (x, p) pairs of xs"""
    mext = chain(key_L0, k)
    n, q = 1 << logn, mext[:key_L0]
    rng = SplitMix(seed)
    s = rng.words(n, 3).astype(np.int64) - 1
    s_ntt = orc.poly_reduce_strict(q, orc.poly_ntt(q, np.stack([(s % m).astype(U) for m in q])))
    s2 = centred(orc, q, orc.poly_mul(q, s_ntt, s_ntt))
    key = keygen(orc, rng, logn, mext, key_L0, k, alpha, s, s2)
    worst = 0
    for x, exact in xs:
        ct = encrypt_constant(orc, rng, q[:L], np.ascontiguousarray(s_ntt[:L]), int(round(x * DELTA)), n)
        out = model_plan(orc, logn, mext, key_L0, k, alpha, key, plan, ct)
        qo = q[:plan.out_limbs]
        assert out.shape == (2, plan.out_limbs, n)
        worst = max(worst, decrypt_error(orc, qo, s_ntt, strict_rows(out, qo), int(round(exact(round(x * DELTA) / DELTA) * DELTA))))
    return worst


def test_power_plan_decrypts_to_the_polynomial(orc):
    logn, L, k, alpha = 4, 5, 1, 1
    plan = build_plan(POWER7, "power", P.P40[:L], DELTA, DELTA, n1=4)
    assert plan.out_limbs == 1 and plan.switches == 4
    worst = run_plan(orc, logn, L, L, k, alpha, plan, [(x, lambda v: float(np.polyval(POWER7[::-1], v))) for x in (0.73, -0.5, 0.001)], 9600)
    print(f"power (4,2) logn {logn}: max |dec - Delta p(x)| = {worst} = 2^{np.log2(max(worst, 1)):.2f}, threshold {POWER_THRESHOLD}")
    assert worst < POWER_THRESHOLD


def test_chebyshev_plan_of_the_device_test_decrypts(orc):
    logn, L, key_L0, k, alpha = 4, 7, 8, 2, 2
    plan = build_plan(CHEB15, "chebyshev", P.P40[:L], DELTA, DELTA, n1=4)
    assert plan.out_limbs == 2
    worst = run_plan(orc, logn, L, key_L0, k, alpha, plan, [(x, lambda v: float(Ch.chebval(v, CHEB15))) for x in (0.73,)], 9700)
    print(f"chebyshev (4,4) logn {logn}: max |dec - Delta p(x)| = {worst} = 2^{np.log2(max(worst, 1)):.2f}, threshold {CHEB16_THRESHOLD}")
    assert worst < CHEB16_THRESHOLD


def test_chebyshev_plan_at_the_ring_degree_of_the_device_test(orc):
    """the end-to-end case of tests/test_gpu_polyeval.py in the model alone: the same shape, plan and values, model-made key and noise"""
    c = E2E
    plan = build_plan(CHEB15, "chebyshev", P.P40[:c["L"]], DELTA, DELTA, n1=c["n1"])
    worst = run_plan(orc, c["logn"], c["L"], c["key_L0"], c["k"], c["alpha"], plan,
                     [(x, lambda v: float(Ch.chebval(v, CHEB15))) for x in c["xs"]], 9800)
    print(f"chebyshev (4,4) logn {c['logn']}: max |dec - Delta p(x)| = {worst} = 2^{np.log2(max(worst, 1)):.2f}, threshold {E2E_THRESHOLD}")
    assert worst < E2E_THRESHOLD
