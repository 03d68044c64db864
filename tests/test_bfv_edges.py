"""The conditions of tests/bfv_edges.py, without a GPU: every modulus a prime = 1 (mod 2N) (one declared decryption set aside), the
bases distinct and disjoint, the base-size rule and t below every modulus at every (shape, t), no wrap of hehub's fold on words below
2q, every planted class present at 2N slots, the model's residue mechanics equal to floor((t x + h) / Q) at the new widths, and the
Garner widths the tables reach -- computed from the tables, so that a shape taken out of them fails here."""
import math

import pytest

import bfv_edges as E
import bfv_model as F
import moduli as MD
import params as P
from oracle.pyoracle import SplitMix

PAIRS = [(s, t) for s in E.SHAPES for t in s.ts]
DEC_PAIRS = [(d, t) for d in E.DECRYPT_SETS for t in d.ts]
CHECKED = 64   # values per (shape, t) held to plain arithmetic: the planted ones come first


def test_the_tables_hold_every_listed_shape():
    """every listed shape is there with its plain moduli: none may be filtered out at run time"""
    assert [(s.name, s.logn, s.L, s.M, len(s.ts)) for s in E.SHAPES] == [
        ("w5", 4, 5, 6, 3), ("w6", 4, 6, 7, 2), ("w7", 4, 7, 8, 2), ("w9", 4, 9, 10, 1), ("w12", 4, 12, 13, 2), ("w16", 5, 16, 16, 2),
        ("w16x59", 5, 16, 16, 2), ("b59", 4, 3, 3, 2), ("q59", 4, 3, 4, 2), ("w59q", 4, 6, 6, 2), ("narrow", 4, 5, 5, 3),
        ("chunks12", 12, 2, 3, 1)]
    assert [s.name for s in E.MULT_SHAPES] == ["w5", "w6", "w7", "w12", "w16", "q59"]
    assert len(E.DECRYPT_SETS) == 16 + 4 + len(E.SHAPES) and len(PAIRS) == 24
    assert [d.name for d in E.DECRYPT_SETS if not d.prime] == ["not-prime"]
    assert all(len(s.ts) == len(set(s.ts)) for s in E.SHAPES + E.DECRYPT_SETS)


def test_every_new_width_is_reached():
    """from the tables: k_bfv_scale and k_bfv_decrypt_round run at width L, k_bfv_lift at L (Q -> B) and at M (B -> Q)"""
    assert E.scale_widths() >= {5, 6, 7, 9, 12, 16}
    assert E.decrypt_widths() >= {5, 6, 7, 9, 12, 16} and E.decrypt_widths() >= set(range(1, 17))
    assert E.lift_widths() >= {6, 7, 10, 12, 13, 16}
    # the widths a shape of the table is the only one to bring (bfv_model.GPU_SHAPES has none of them): taking it out fails
    for name, widths in (("w7", {7, 8}), ("w9", {9, 10}), ("w12", {12, 13})):
        rest = [s for s in E.SHAPES if s.name != name]
        assert not widths <= {s.L for s in rest} | {s.M for s in rest}, name
    assert sum(s.L == 16 and s.M == 16 for s in E.SHAPES) == 2 and sum(s.L == 5 for s in E.SHAPES) == 2 and sum(s.L == 6 for s in E.SHAPES) == 2
    assert max(s.L + s.M for s in E.SHAPES) == 32
    assert {s.n // 2048 for s in E.CHUNK_SHAPES} == {2} and {d.n // 2048 for d in E.DECRYPT_SETS} >= {0, 2, 4}
    # (not the wide chain tests/test_gpu_bfv.py already runs)
    assert not {tuple(s.q) for s in E.SHAPES} & {tuple(F.shape_moduli(g)[0][:g[1]]) for g in F.GPU_SHAPES if g[1] > 4}


@pytest.mark.parametrize("shape", E.SHAPES, ids=str)
def test_moduli_of_a_shape(shape):
    q, b, qb, n = shape.q, shape.b, shape.qb, shape.n
    assert len(set(qb)) == len(qb) and not set(q) & set(b)
    assert all(P.is_prime(m) and m % (2 * n) == 1 and m < (1 << 59) for m in qb)
    for m in qb:   # the transforms see words below 2q (the calls' promise) and strict rows
        assert not MD.fold_bound(m, 2 * m, shape.logn)[0], m
    assert not set(qb) & {MD.NARROW[1], MD.NARROW[3]}
    slots = E.BATCH * n
    assert all(F.lift_classes(F.lift_planted(SplitMix(1), qb, shape.L, slots), qb, shape.L).values())


def test_widths_of_the_named_shapes():
    bits = lambda xs: sorted({m.bit_length() for m in xs})
    by = {s.name: s for s in E.SHAPES}
    for name in ("w5", "w6", "w7", "w9", "w12"):
        assert bits(by[name].qb) == [40]
    assert (bits(by["w16"].q), bits(by["w16"].b)) == ([40], [50]) and (bits(by["w16x59"].q), bits(by["w16x59"].b)) == ([36], [59])
    assert all(m % (1 << 16) == 1 for m in by["w16x59"].b)
    assert (bits(by["b59"].q), bits(by["b59"].b)) == ([40], [59]) and bits(by["q59"].qb) == [59]
    assert bits(by["w59q"].q) == [40, 59] and bits(by["w59q"].b) == [46, 47, 48, 49]   # (2^k + small has k + 1 bits)
    assert bits(by["narrow"].q) == [20, 30, 59] and all(m < (1 << MD.log_modulus(m)) for m in by["narrow"].q)
    assert all(MD.fold_consts(m)[1] == 1 for m in by["narrow"].b)
    # close to the base-size rule: B / (4 t N Q) is 2 to within 2^-15, and one prime less in B breaks the rule
    s = by["w59q"]
    need = 4 * E.T0 * s.n * F.prod(s.q)
    assert need <= F.prod(s.b) < 2 * need + (need >> 15) and not F.base_ok(s.qb[:-1], s.L, E.T0, s.n)
    assert by["b59"].ts[1] % 2 == 0 and by["b59"].ts[1].bit_length() == 40


@pytest.mark.parametrize("shape,t", PAIRS, ids=str)
def test_a_shape_and_plain_modulus(shape, t):
    q, qb, L, n = shape.q, shape.qb, shape.L, shape.n
    Q = F.prod(q)
    assert 2 <= t < min(qb) and math.gcd(t, Q) == 1
    assert F.base_ok(qb, L, t, n)
    slots = E.BATCH * n
    vals = F.scale_planted(SplitMix(2), qb, L, t, n, slots)
    assert all(F.scale_classes(vals, qb, L, t, n).values())
    for x in vals[:CHECKED]:
        assert F.scale_residues([x % m for m in q], [x % m for m in shape.b], q, shape.b, t) == F.scale_int(x, t, Q), x


@pytest.mark.parametrize("dset,t", DEC_PAIRS, ids=str)
def test_a_decryption_set_and_plain_modulus(dset, t):
    q, n = dset.q, dset.n
    Q = F.prod(q)
    assert len(set(q)) == len(q) and all(m % 2 == 1 and m >= 3 for m in q)
    assert all(P.is_prime(m) for m in q) == dset.prime
    assert all(math.gcd(a, c) == 1 for i, a in enumerate(q) for c in q[:i])
    assert 2 <= t < min(q) and math.gcd(t, Q) == 1
    assert n >= 8 and n & (n - 1) == 0 and n <= 8192
    vals = F.decrypt_planted(SplitMix(3), q, t, E.BATCH * n)
    assert all(F.decrypt_classes(vals, q, t).values())
    for x in vals[:CHECKED]:
        assert F.decrypt_residues([x % m for m in q], q, t) == F.decrypt_int(x, t, Q) < t, x


def test_the_decryption_sets_hold_what_they_name():
    by = {d.name: d for d in E.DECRYPT_SETS}
    for L in range(1, 17):
        d = by["p59-L%d" % L]
        assert len(d.q) == L and all(m.bit_length() == 59 for m in d.q) and d.ts == (2, E.T0, 1 << 58, min(d.q) - 1)
    assert by["narrow-chain"].q == MD.NARROW and by["narrow-chain"].ts[2] == min(MD.NARROW) - 1
    assert by["chunks4"].n == 4 * 2048 and by["chunks4"].q == P.P40[:2]
    for s in E.SHAPES:
        assert (by["Q-of-" + s.name].q, by["Q-of-" + s.name].n, by["Q-of-" + s.name].ts) == (s.q, s.n, s.ts)


def test_the_hybrid_shape():
    logn, L, M, k, alpha = E.HYBRID
    n, mext, aux, t = 1 << logn, E.HYBRID_MEXT, E.HYBRID_AUX, E.HYBRID_T
    assert (len(mext), len(aux)) == (L + k, M) and len(set(mext + aux)) == L + k + M
    assert all(P.is_prime(m) and m % (2 * n) == 1 for m in mext + aux)
    assert F.base_ok(mext[:L] + aux, L, t, n) and t < min(mext + aux)
    assert L not in {g[1] for g in F.GPU_SHAPES} and L > 4   # a width no earlier end-to-end test runs, compiled with the fences
    assert all(not MD.fold_bound(m, 2 * m, logn)[0] for m in mext + aux)


def test_values_that_need_the_garner_steps_strict_reduction():
    """bfv_digit reduces digit b modulo x_A lazily and then strictly before u + x_A - v_b.  With moduli of one width the lazy word is
    already below x_A; a 59-bit digit in front of a 40-bit modulus can leave x_A + s for small s, and u < s would wrap.  Uniform
    inputs do not get there: w59q plants it (lift, scaling and decryption rounding)."""
    by = {s.name: s for s in E.SHAPES}
    assert [s.name for s in E.SHAPES if E.digit_wrap_values(s.q)] == ["w59q"]
    assert [d.name for d in E.DECRYPT_SETS if E.digit_wrap_values(d.q)] == ["wide-first", "Q-of-w59q"]   # (a 59-bit digit into 20 bits too)
    for d in E.DECRYPT_SETS:
        for t in d.ts:
            xs = E.digit_wrap_inputs(d.q, t)
            assert all(F.decrypt_classes(E.plant_last(F.decrypt_planted(SplitMix(3), d.q, t, 32), xs), d.q, t).values())
    q = by["w59q"].q
    Q, h = F.prod(q), (F.prod(q) - 1) // 2
    wrap = E.digit_wrap_values(q)
    assert len(wrap) == 2
    for w in wrap:
        vb = E.barrett_lazy(w % q[0], q[1])
        assert 0 <= w < Q and q[1] <= vb < 2 * q[1] and vb % q[1] == (w % q[0]) % q[1]
        assert w % q[1] + q[1] - vb < 0                 # a negative word without the strict reduction
        assert w % q[1] + q[1] - vb % q[1] >= 0
    assert vb - q[1] == 1 << 19                  # s < 2^19 + 1 of a 40-bit modulus: two uniform residues meet there once in 2^43
    for t in by["w59q"].ts:
        xs = E.digit_wrap_inputs(q, t)
        assert [(t * x + h) % Q for x in xs] == wrap and all(0 <= x < Q for x in xs)
        n, slots = by["w59q"].n, E.BATCH * by["w59q"].n
        assert all(F.scale_classes(E.plant_last(F.scale_planted(SplitMix(2), by["w59q"].qb, 6, t, n, slots), xs), by["w59q"].qb, 6, t, n).values())
        assert all(F.decrypt_classes(E.plant_last(F.decrypt_planted(SplitMix(3), q, t, slots), xs), q, t).values())
    assert all(F.lift_classes(E.plant_last(F.lift_planted(SplitMix(1), by["w59q"].qb, 6, slots), wrap), by["w59q"].qb, 6).values())
    # one width: the lazy word of a digit is the digit
    p = by["w5"].q
    assert all(E.barrett_lazy(x, p[1]) == x for x in (0, 1, p[1] - 1)) and not E.digit_wrap_values(p) and not E.digit_wrap_values(E.P59)


def test_edge_rows_hold_the_largest_word():
    import numpy as np

    for s in (E.SHAPES[0], E.SHAPES[6], E.SHAPES[10]):
        x = E.edge_rows(SplitMix(4), (E.BATCH, len(s.qb), s.n), s.qb)
        qa = np.array(s.qb, dtype=E.U)[:, None]
        assert x.shape == (E.BATCH, len(s.qb), s.n) and (x.max(axis=-1) == 2 * qa[:, 0] - 1).all()
        y = E.lazy(SplitMix(5), x % qa, s.qb)
        assert (y % qa == x % qa).all() and (y >= qa).any() and (y < 2 * qa).all()
