"""tests/bfv_model.py held to plain arithmetic, without a GPU: the residue mechanics of the scaling and of the decryption rounding
against floor((t x + h) / Q) on Python integers, the model's lift / tensor / scale against schoolbook negacyclic products at
N = 8 and 16, decryption of products at the (Q, B, t) sets of the issue, and the planted classes at every GPU shape."""
import numpy as np
import pytest

import bfv_model as F
import params as P
from oracle.pyoracle import SplitMix

U = np.uint64
M31 = 2147483647
SETS = [(P.P40[:2], P.P40[2:5], 65537), (P.P40[:3], P.P40[3:7], 65537), (P.P40[:4], P.P40[4:9], 65537), (P.P40[:1], P.P40[1:3], 2),
        (P.P40[:3], P.P50[:4], 2), (P.P40[:3], P.P50[:4] + P.P40[3:4], M31)]
IDS = ["L2", "L3", "L4", "L1-t2", "P50aux-t2", "t31"]


def ternary(rng, n):
    return [int(x) - 1 for x in rng.words(n, 3)]


@pytest.mark.parametrize("q,b,t", SETS, ids=IDS)
@pytest.mark.parametrize("n", [8, 16])
def test_the_base_size_rule_holds_at_the_sets(q, b, t, n):
    assert F.base_ok(q + b, len(q), t, n)
    Q, B = F.prod(q), F.prod(b)
    bound = F.tensor_bound(Q, n)
    assert t * bound + (Q - 1) // 2 < Q * B // 2 and abs(F.scale_int(bound, t, Q)) < B // 2 and abs(F.scale_int(-bound, t, Q)) < B // 2


@pytest.mark.parametrize("q,b,t", SETS, ids=IDS)
def test_residue_mechanics_are_the_rounded_division(q, b, t):
    """planted and random x over the whole allowed range: the mechanics give floor((t x + h) / Q) exactly"""
    n, L = 16, len(q)
    Q = F.prod(q)
    vals = F.scale_planted(SplitMix(100 + t % 97), q + b, L, t, n, 64)
    assert all(F.scale_classes(vals, q + b, L, t, n).values())
    for x in vals:
        assert F.scale_residues([x % m for m in q], [x % m for m in b], q, b, t) == F.scale_int(x, t, Q), x


@pytest.mark.parametrize("q,b,t", SETS, ids=IDS)
def test_decryption_rule_is_the_rounding(q, b, t):
    Q = F.prod(q)
    vals = F.decrypt_planted(SplitMix(200 + t % 97), q, t, 64)
    assert all(F.decrypt_classes(vals, q, t).values())
    for x in vals:
        assert F.decrypt_residues([x % m for m in q], q, t) == F.decrypt_int(x, t, Q), x
    got = F.decrypt_round(q, t, F.residue_rows(vals, q))
    assert got.tolist() == [F.decrypt_int(x, t, Q) for x in vals]


@pytest.mark.parametrize("logn", [3, 4])
def test_lift_tensor_and_scale_match_schoolbook_products(orc, logn):
    """the model's quadratic ciphertext = the rounded t / Q multiples of the schoolbook tensor of the centred polynomials"""
    q, b, t = SETS[0]
    n, L, qb = 1 << logn, len(q), q + b
    Q = F.prod(q)
    rng = SplitMix(300 + logn)
    ct1, ct2 = rng.poly((2, L, n), q), rng.poly((2, L, n), q)
    c = [[[F.centre(v, Q) for v in F.ints_of(F.coeff_rows(orc, q, ct[h]), q)] for h in range(2)] for ct in (ct1, ct2)]
    for h in range(2):   # the lift keeps the Q rows and carries the centred integer
        up = F.lift(orc, logn, qb, L, ct1[h])
        assert np.array_equal(up[:L], ct1[h])
        assert [F.centre(v, Q * F.prod(b)) for v in F.ints_of(F.coeff_rows(orc, qb, up), qb)] == c[0][h]
    cross = [x + y for x, y in zip(F.negacyclic(c[0][0], c[1][1]), F.negacyclic(c[0][1], c[1][0]))]
    tensor = [F.negacyclic(c[0][0], c[1][0]), cross, F.negacyclic(c[0][1], c[1][1])]
    assert all(abs(x) <= 2 * F.tensor_bound(Q, n) for row in tensor for x in row)
    got = F.mult_low_level(orc, logn, qb, L, t, ct1, ct2)
    for j in range(3):
        want = [F.scale_int(x, t, Q) for x in tensor[j]]
        assert np.array_equal(got[j], F.ntt_rows(orc, logn, q, want)), j


@pytest.mark.parametrize("q,b,t", SETS, ids=IDS)
@pytest.mark.parametrize("logn", [3, 4])
def test_products_decrypt(orc, q, b, t, logn):
    n = 1 << logn
    rng = SplitMix(400 + logn + t % 89)
    s = ternary(rng, n)
    m1, m2 = [int(x) for x in rng.words(n, t)], [int(x) for x in rng.words(n, t)]
    ct1, ct2 = F.encrypt(orc, rng, logn, q, t, s, m1), F.encrypt(orc, rng, logn, q, t, s, m2)
    quad = F.mult_low_level(orc, logn, q + b, len(q), t, ct1, ct2)
    assert F.decrypt_quadratic(orc, q, t, s, quad) == [x % t for x in F.negacyclic(m1, m2)]


@pytest.mark.parametrize("shape", F.GPU_SHAPES, ids=str)
def test_gpu_shapes_satisfy_the_rule_and_fill_every_planted_class(shape):
    logn, L, M, k, alpha = shape
    mext, aux = F.shape_moduli(shape)
    n, q = 1 << logn, mext[:L]
    qb = q + aux
    assert len(aux) == M and len(mext) == L + k and len(set(qb)) == L + M and not set(q) & set(mext[L:])
    assert all(P.is_prime(m) and m % (2 * n) == 1 for m in qb + mext[L:])
    ts = F.shape_plain_moduli(shape)
    assert F.T0 in ts and all(F.base_ok(qb, L, t, n) for t in ts)
    if shape == F.GPU_SHAPES[0]:
        assert ts == F.PLAIN_MODULI
    slots = 2 * n   # batch 2
    assert all(F.lift_classes(F.lift_planted(SplitMix(1), qb, L, slots), qb, L).values())
    for t in ts:
        assert all(F.scale_classes(F.scale_planted(SplitMix(2), qb, L, t, n, slots), qb, L, t, n).values()), t
        assert all(F.decrypt_classes(F.decrypt_planted(SplitMix(3), q, t, slots), q, t).values()), t
