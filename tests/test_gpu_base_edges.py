"""The RNS base transforms (hp_edge.hip) on planted inputs (tests/base_edges.py): the old modulus' half and its neighbours, strict and
lazy, into narrower and wider new moduli; coefficients of magnitude min(q) / 2 - 1, min(q) / 2, min(q) / 2 + 1 at the small-coefficient
check's boundary; CRT values at floor(Q / 2) - 1, floor(Q / 2), floor(Q / 2) + 1, Q - 1 and the multiples of the new modulus below Q,
where the lexicographic comparison of the mixed-radix digits changes sides.  Every output against the oracle (which
tests/test_drop_edges.py holds to the reference at these inputs); the many -> many conversion against Python integers."""
import numpy as np
import pytest

import base_edges as BE

pytestmark = pytest.mark.gpu
U = np.uint64
SIZES = [8, 4096, 32768]


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.release_workspace()
    e.close()


@pytest.mark.parametrize("n", SIZES)
def test_from_single_at_the_half_strict_and_lazy(eng, orc, n):
    for old, new, x in BE.from_single_cases(n):
        rows = np.stack([x, x[::-1], np.roll(x, 3)])
        got = eng.to_host(eng.rns_base_from_single(old, new, eng.to_device(rows)))
        exp = np.stack([orc.rns_base_from_single(old, new, np.ascontiguousarray(r)) for r in rows])
        assert np.array_equal(got, exp), (old, new)


@pytest.mark.parametrize("n", SIZES)
def test_to_single_at_the_small_coefficient_boundary(eng, orc, n):
    for name, old, new, x in BE.small_cases(n):
        out, flags = eng.rns_base_to_single_small(old, new, eng.to_device(x))
        out, flags = eng.to_host(out), flags.cpu().numpy()
        for p in range(x.shape[0]):
            ok, exp = orc.rns_base_to_single_small(old, new, x[p])
            assert (flags[p] == 0) == ok, (name, p)
            if ok:
                assert np.array_equal(out[p], exp), (name, p)
        got = eng.to_host(eng.rns_base_to_single(old, new, eng.to_device(x)))
        exp = np.stack([orc.rns_base_to_single(old, new, x[p]) for p in range(x.shape[0])])
        assert np.array_equal(got, exp), name


def test_seventeen_old_moduli_are_refused(eng):
    """HP_CRT_MAX_LIMBS = 16: one more is a status, and nothing is written"""
    from hehub_amd import capi
    from hehub_amd.engine import HpError

    old, n = BE.CHAIN17, 8
    x = eng.to_device(np.zeros((1, len(old), n), dtype=U))
    out = eng.empty((1, n))
    out.fill_(-1)
    with pytest.raises(HpError) as err:
        eng.rns_base_to_single(old, BE.T17, x)
    assert err.value.code == capi.HP_EUNSUPPORTED
    with pytest.raises(HpError) as err:
        eng.rns_base_many_to_many(old, [BE.T17], x)
    assert err.value.code == capi.HP_EUNSUPPORTED
    rc = eng.lib.hp_dev_rns_base_to_single(eng.h, n, len(old), (capi.u64 * len(old))(*old), BE.T17, 1, eng._ptr(x), eng._ptr(out))
    assert rc == capi.HP_EUNSUPPORTED and (eng.to_host(out) == U((1 << 64) - 1)).all()


@pytest.mark.parametrize("n", SIZES)
def test_crt_branch_around_half_q(eng, orc, n):
    for name, old, new, x, want in BE.crt_cases(n):
        got = eng.to_host(eng.rns_base_to_single(old, new, eng.to_device(x)))
        exp = np.stack([orc.rns_base_to_single(old, new, x[p]) for p in range(2)])
        assert np.array_equal(got, exp), name
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want), name


@pytest.mark.parametrize("n", SIZES)
def test_many_to_many_around_half_q(eng, n):
    """the same values into several new moduli at once, against Python integers"""
    for name, old, t, x, _ in BE.crt_cases(n):
        new = [t, BE.Q20, 257, BE.P.P50[3]]
        Q, vals = BE.product(old), BE.crt_values(old, t)
        got = eng.to_host(eng.rns_base_many_to_many(old, new, eng.to_device(x)))
        for k, m in enumerate(new):
            want = np.array([BE.single_of(v, Q, m) for v in vals], dtype=U)[np.arange(n) % len(vals)]
            assert np.array_equal(got[0, k], want) and np.array_equal(got[1, k], want), (name, m)
