"""What the comparisons of tests/test_gpu_hks_dot.py rest on (CPU tier): the device hands the hybrid switch a lazy representative of
sum d2 (words below 2q), the model a canonical one.  model_switch's strict residues do not depend on which: adding q_i to some input
words changes neither the coefficients it decomposes nor, modulo each modulus, the inner product, ModDown or the division by P."""
import numpy as np

import params as P
from dot_model import model_tensor_sum, strict_rows
from hks_model import model_switch
from oracle.pyoracle import SplitMix

U = np.uint64


def test_model_switch_residues_do_not_depend_on_the_representative(orc):
    logn, L, k, alpha = 4, 3, 2, 2
    mext = P.P40[:L] + P.P50[:k]
    n, q = 1 << logn, mext[:L]
    rng = SplitMix(8100)
    pt = rng.poly((L, n), q)
    key = rng.poly(((L + alpha - 1) // alpha, 2, L + k, n), mext)
    lazy = pt.copy()
    lazy[:, ::3] += np.array(q, dtype=U)[:, None]       # some words in [q, 2q), in every limb
    lazy[1] = pt[1] + U(q[1])                           # ... and a whole limb of them
    assert (lazy >= np.array(q, dtype=U)[:, None]).any() and np.array_equal(strict_rows(lazy, q), pt)
    a, b = model_switch(orc, logn, mext, L, k, alpha, pt, key), model_switch(orc, logn, mext, L, k, alpha, lazy, key)
    assert np.array_equal(strict_rows(a, q), strict_rows(b, q))


def test_model_tensor_sum_of_one_term_is_the_oracle_tensor_product(orc):
    L, n = 2, 8
    q = P.P40[:L]
    rng = SplitMix(8101)
    a, b = rng.poly((2, L, n), q), rng.poly((2, L, n), q)
    assert np.array_equal(model_tensor_sum(q, [a], [b]), strict_rows(orc.mult_low_level(q, a, b), q).astype(object))
