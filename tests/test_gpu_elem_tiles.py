"""Every path of the tile skeleton the coefficient-wise kernels share (hehub_amd/csrc/hp_elem.h), word for word against the oracle, at
the smallest shapes that reach it: the single-word tail (n = 1), one pair (n = 2), a partial chunk in two rounds of the pair loop
(n = 1024), exactly one full chunk (n = 2048) and two chunks per row (n = 4096), with L = 3 limbs and a batch of 2 so that both
row % L and row / L matter.  Then the two workgroup sizes of the tensor product, and the first and a middle case of the Garner
digits and of the 1..8 template dispatch (many -> one base transform on its CRT branch; hybrid ModUp / ModDown)."""
import numpy as np
import pytest

import params as P
from oracle.pyoracle import SplitMix

U = np.uint64
MODULI = P.P40[:3]
B = 2
SCALARS = [2**63 + 5, 3, P.P40[1] - 1]             # one per limb (RNS-scalar multiply)
NEGATE = [0, 1, 0, 1, 1]                           # the five-term fold: x0 - x1 + x2 - x3 - x4


def operands(n, terms=5):
    """terms polynomials [B][L][n] of words below 2q"""
    return SplitMix(4200 + n).poly((terms, B, len(MODULI), n), [2 * q for q in MODULI])


def cpu_results(o, x):
    """what the CPU library o gives for every polynomial operation of this file on the operands x (one polynomial at a time)"""
    a, b = x[0], x[1]
    per = lambda f: np.stack([f(i) for i in range(B)])
    fold = []
    for i in range(B):
        acc = x[0][i]
        for j in range(1, len(NEGATE)):
            acc = o.poly_sub(MODULI, acc, x[j][i]) if NEGATE[j] else o.poly_add(MODULI, acc, x[j][i])
        fold.append(acc)
    return {"add": per(lambda i: o.poly_add(MODULI, a[i], b[i])), "sub": per(lambda i: o.poly_sub(MODULI, a[i], b[i])),
            "mul": per(lambda i: o.poly_mul(MODULI, a[i], b[i])), "strict": per(lambda i: o.poly_reduce_strict(MODULI, a[i])),
            "scalar": per(lambda i: o.poly_scalar_mul(MODULI, a[i], SCALARS[0])),
            "rns_scalar": per(lambda i: o.poly_rns_scalar_mul(MODULI, a[i], SCALARS)), "fold": np.stack(fold)}


_EXPECTED = {}


def expected(orc, n):
    """(operands, the oracle's results) for rows of n words: computed once, shared by whatever asks for this n, never changed"""
    if n not in _EXPECTED:
        x = operands(n)
        exp = cpu_results(orc, x)
        for v in (x, *exp.values()):
            v.setflags(write=False)
        _EXPECTED[n] = (x, exp)
    return _EXPECTED[n]


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("n", [1, 2])
def test_oracle_and_reference_agree_on_the_shortest_rows(orc, ref, n):
    """CPU: the oracle's words at the two sizes no other test pins are the compiled reference's"""
    x = operands(n, terms=2)
    a, b = x[0], x[1]
    for i in range(B):
        assert np.array_equal(orc.poly_add(MODULI, a[i], b[i]), ref.poly_add(MODULI, a[i], b[i]))
        assert np.array_equal(orc.poly_sub(MODULI, a[i], b[i]), ref.poly_sub(MODULI, a[i], b[i]))
        assert np.array_equal(orc.poly_mul(MODULI, a[i], b[i]), ref.poly_mul(MODULI, a[i], b[i]))
        assert np.array_equal(orc.poly_reduce_strict(MODULI, a[i]), ref.poly_reduce_strict(MODULI, a[i]))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 1024, 2048, 4096])
def test_polynomial_operations_on_every_tile_path(eng, orc, n):
    x, exp = expected(orc, n)
    d = [eng.to_device(t.copy()) for t in x]
    # the fold takes its term rows by address, 16-byte aligned each (include/hehub_amd.h): at n = 1 the second polynomial of a
    # [B][L][n] tensor is not, so every term polynomial gets a tensor of its own, as an application's separate objects have
    rows = [[eng.to_device(t[p].copy()) for t in x] for p in range(B)]
    got = {"add": eng.poly_add(MODULI, d[0], d[1]), "sub": eng.poly_sub(MODULI, d[0], d[1]), "mul": eng.poly_mul(MODULI, d[0], d[1]),
           "scalar": eng.poly_scalar_mul(MODULI, d[0], SCALARS[0]), "rns_scalar": eng.poly_scalar_mul(MODULI, d[0], SCALARS),
           "strict": eng.poly_reduce_strict_(MODULI, d[0].clone()),
           "fold": eng.poly_fold_rows(MODULI, rows, NEGATE)}
    for name, t in got.items():
        assert np.array_equal(eng.to_host(t), exp[name]), (name, n)
    assert np.array_equal(eng.to_host(eng.copy(d[0])), x[0]), ("copy", n)      # hp_dev_copy of B * L * n words
    # in place, as operator+= uses the kernel (out == a)
    inplace = np.stack([orc.poly_add(MODULI, x[2][i], x[1][i]) for i in range(B)])
    assert np.array_equal(eng.to_host(eng.poly_add(MODULI, d[2], d[1], out=d[2])), inplace), ("add in place", n)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [2, 256])
def test_tensor_product_at_both_workgroup_sizes(eng, orc, batch):
    """logn 11, L = 4: 8 rows take the 512-word workgroups, 1024 rows the 2048-word ones (hp_ks.hip: tensor_chunk)"""
    moduli, n = P.P40[:4], 1 << 11
    rng = SplitMix(4300 + batch)
    ct1, ct2 = rng.poly((batch, 2, 4, n), moduli), rng.poly((batch, 2, 4, n), moduli)
    got = eng.to_host(eng.mult_low_level(moduli, eng.to_device(ct1), eng.to_device(ct2)))
    exp = np.stack([orc.mult_low_level(moduli, ct1[i], ct2[i]) for i in range(batch)])
    assert np.array_equal(got, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [2, 5])
def test_many_to_one_base_transform_on_the_crt_branch(eng, orc, L):
    """n = 8, coefficients not small: the Garner digits of 2 and of 5 limbs, and the value -new that comes out as new itself"""
    old, new, n = P.P40[:L], 65537, 8
    x = SplitMix(4400 + L).poly((B, L, n), old)
    x[1, :, 0] = [(q - new % q) % q for q in old]
    got = eng.to_host(eng.rns_base_to_single(old, new, eng.to_device(x)))
    exp = np.stack([orc.rns_base_to_single(old, new, x[i]) for i in range(B)])
    assert np.array_equal(got, exp) and got[1, 0] == new


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [1, 3])
def test_hybrid_modup_and_moddown_dispatch(eng, orc, alpha):
    """n = 8, L = 3, alpha limbs per digit and alpha special primes: k_hks_modup<alpha> and k_hks_moddown<alpha> against the
    exact integer model of tests/hks_model.py"""
    from hks_model import model_switch

    logn, L, k = 3, 3, alpha
    mext = P.P40[:L] + P.P50[:k]
    n, nd = 1 << logn, (L + alpha - 1) // alpha
    rng = SplitMix(4500 + alpha)
    pt = np.stack([rng.poly((L, n), mext[:L]) for _ in range(B)])
    key = rng.poly((nd, 2, L + k, n), mext)
    got = eng.to_host(eng.hks_switch(mext, k, alpha, eng.to_device(pt), eng.to_device(key)))
    for i in range(B):
        assert np.array_equal(got[i], model_switch(orc, logn, mext, L, k, alpha, pt[i], key)), (i, alpha)
