"""hp_dev_ckks_tensor_sum (hp_ks.hip: k_tensor_sum) against the exact model (tests/dot_model.py: Python integers modulo each q_i).
The contract is on residues with every output word below 2q.  The shapes are the smallest that reach each path of the kernel and of
the launch loop: the short row (a few lanes of one workgroup), the 512-word workgroup and the batch stride, a full argument table, two
and three launches (add_prev), squares and repeated addresses -- and the largest sum the range function (hpi::tensor_sum_max_terms,
tests/test_tensor_sum_host.py) is about, planted at a 59-bit modulus."""
import ctypes as C

import numpy as np
import pytest

import moduli as M
import params as P
from dot_model import below_2q, model_tensor_sum, strict_rows
from oracle.pyoracle import SplitMix

pytestmark = pytest.mark.gpu
U = np.uint64


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def check(eng, q, a_host, b_host, d_a, d_b):
    """a_host[t], b_host[t]: [B][2][L][n]; the device lists may share tensors"""
    got = eng.to_host(eng.ckks_tensor_sum(q, d_a, d_b))
    B = a_host[0].shape[0]
    assert got.shape == (B, 3) + a_host[0].shape[2:]
    assert below_2q(got, q)
    for p in range(B):
        exp = model_tensor_sum(q, [a[p] for a in a_host], [b[p] for b in b_host])
        assert np.array_equal(strict_rows(got[p], q).astype(object), exp), p
    return got


@pytest.mark.parametrize("logn,L,T,B", [
    (3, 2, 1, 1),      # a: a row shorter than one pair tile; one term
    (11, 3, 5, 2),     # b: the 512-word workgroup; the batch stride
    (13, 2, 32, 1),    # c: a full table
    (11, 2, 33, 1),    # d: two launches, add_prev
    (11, 2, 65, 1),    # e: three launches
], ids=list("abcde"))
def test_tensor_sum_matches_the_integer_model(eng, orc, logn, L, T, B):
    q, n = P.P40[:L], 1 << logn
    rng = SplitMix(8200 + logn + T)
    a = [M.lazy_rows(rng, (B, 2, L, n), q) for _ in range(T)]      # strict words, words in [q, 2q), some 2q - 1
    b = [M.lazy_rows(rng, (B, 2, L, n), q) for _ in range(T)]
    d_a, d_b = [eng.to_device(x) for x in a], [eng.to_device(x) for x in b]
    got = check(eng, q, a, b, d_a, d_b)
    if T == 1:   # the residues of hehub's tensor product, from the device and from the oracle
        low = eng.to_host(eng.mult_low_level(q, d_a[0], d_b[0]))
        assert np.array_equal(strict_rows(got, q), strict_rows(low, q))
        assert np.array_equal(strict_rows(got[0], q), strict_rows(orc.mult_low_level(q, a[0][0], b[0][0]), q))


def test_squares_and_repeated_addresses(eng):
    """f: a_list is b_list (a sum of squares), and one tensor standing for several terms"""
    logn, L = 12, 3
    q, n = P.P40[:L], 1 << logn
    rng = SplitMix(8260)
    x, y = M.lazy_rows(rng, (1, 2, L, n), q), M.lazy_rows(rng, (1, 2, L, n), q)
    dx, dy = eng.to_device(x), eng.to_device(y)
    d_list = [dx, dy, dx]
    check(eng, q, [x, y, x], [x, y, x], d_list, d_list)
    check(eng, q, [x, x, y], [y, x, x], [dx, dx, dy], [dy, dx, dx])


def planted(kind, rng, q, n):
    """one ciphertext batch [1][2][L][n] of moduli.edge_words rows, or every word 2q - 1 / every other word 2q - 1"""
    return np.stack([np.stack([M.edge_words(rng, kind, m, n) for m in q]) for _ in range(2)])[None]


@pytest.mark.parametrize("logn", [4, 11])
@pytest.mark.parametrize("kind", ["max", "alt"])
def test_planted_extremes_at_a_59_bit_modulus(eng, logn, kind):
    """g: the sum the range function is about, at its largest: a full table of 32 terms with EVERY operand word 2q - 1 ("max": each d1
    word is 2 * 32 * (2q - 1)^2) or alternating between 2q - 1 and 0 ("alt": both neighbours of a lane's pair differ), on W59[:3] --
    a 59-bit q0 next to 40-bit limbs.  The expected residues are Python integers."""
    q, n, T = M.W59[:3], 1 << logn, 32
    assert M.Q59 == q[0] and q[0].bit_length() == 59
    rng = SplitMix(8270 + logn)
    x = planted(kind, rng, q, n)
    dx = eng.to_device(x)
    got = eng.to_host(eng.ckks_tensor_sum(q, [dx] * T, [dx] * T))
    assert below_2q(got, q)
    w = [np.array([int(v) for v in M.edge_words(rng, kind, m, n)], dtype=object) for m in q]
    for i, m in enumerate(q):
        sq = w[i] * w[i] * T
        for c, exp in enumerate((sq % m, 2 * sq % m, sq % m)):
            assert np.array_equal((got[0, c, i] % U(m)).astype(object), exp), (i, c)
    if kind == "max":   # the largest sum a launch can see, against the host function's premise
        assert 2 * T * (2 * q[0] - 1) ** 2 <= ((1 << 64) - q[0]) * (1 << 64) - 1
    # different operands for a and b, mixed kinds: the cross terms of d1 are two different products
    y = planted("alt" if kind == "max" else "max", rng, q, n)
    dy = eng.to_device(y)
    check(eng, q, [x] * 16 + [y] * 16, [y] * 16 + [y] * 16, [dx] * 16 + [dy] * 16, [dy] * 32)


def test_refusals_enqueue_nothing(eng):
    """terms == 0, a NULL entry, a misaligned entry, an output that overlaps an operand: HP_EINVAL, and the output keeps its words"""
    from hehub_amd import capi

    logn, L = 4, 2
    q, n = P.P40[:L], 1 << logn
    rng = SplitMix(8290)
    x = eng.to_device(rng.poly((1, 2, L, n), q))
    big = eng.empty((5 * L * n,))                      # room for an operand [1][2][L][n] followed by an output [1][3][L][n]
    big.fill_(7)
    eng.copy(x.reshape(-1), out=big[:2 * L * n])
    out = eng.empty((1, 3, L, n))
    out.fill_(7)
    mod = (capi.u64 * L)(*q)

    def call(terms, a, b, dst):
        return eng.lib.hp_dev_ckks_tensor_sum(eng.h, logn, L, mod, 1, terms, (capi.P * len(a))(*a), (capi.P * len(b))(*b), C.c_void_p(dst))

    xp, op = x.data_ptr(), out.data_ptr()
    assert call(1, [xp], [xp], op) == capi.HP_OK       # the call as such is fine
    out.fill_(7)
    assert call(0, [xp], [xp], op) == capi.HP_EINVAL
    assert call(2, [xp, None], [xp, xp], op) == capi.HP_EINVAL
    assert call(2, [xp, xp], [None, xp], op) == capi.HP_EINVAL
    assert call(2, [xp, xp], [xp, xp + 8], op) == capi.HP_EINVAL
    assert call(1, [xp], [xp], op + 8) == capi.HP_EINVAL
    assert eng.lib.hp_dev_ckks_tensor_sum(eng.h, logn, L, mod, 1, 1, None, (capi.P * 1)(xp), C.c_void_p(op)) == capi.HP_EINVAL
    assert eng.lib.hp_dev_ckks_tensor_sum(eng.h, logn, L, mod, 0, 1, (capi.P * 1)(xp), (capi.P * 1)(xp), C.c_void_p(op)) == capi.HP_EINVAL
    assert eng.lib.hp_dev_ckks_tensor_sum(eng.h, logn, 0, mod, 1, 1, (capi.P * 1)(xp), (capi.P * 1)(xp), C.c_void_p(op)) == capi.HP_EINVAL
    assert eng.lib.hp_dev_ckks_tensor_sum(eng.h, logn, 33, mod, 1, 1, (capi.P * 1)(xp), (capi.P * 1)(xp), C.c_void_p(op)) == capi.HP_EINVAL
    # the output inside the operand, and starting in the operand's last 16 bytes
    bp = big.data_ptr()
    assert call(1, [bp], [xp], bp) == capi.HP_EINVAL
    assert call(1, [xp], [bp], bp + (2 * L * n - 2) * 8) == capi.HP_EINVAL
    assert call(1, [bp], [bp], bp + 2 * L * n * 8) == capi.HP_OK          # adjacent is not overlapping
    eng.sync()
    assert (eng.to_host(out) == 7).all()
    with pytest.raises(ValueError, match="overlaps an operand"):   # the front end reports it as the reference's invalid_argument
        eng.ckks_tensor_sum(q, [big[:2 * L * n].reshape(1, 2, L, n)], [x], out=big[:3 * L * n].reshape(1, 3, L, n))
