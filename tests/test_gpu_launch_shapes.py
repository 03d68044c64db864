"""The launch shapes at which the work-item numbering has a tail, on the tiled kernels (every engine here is created with
HP_SPLIT_MAX_ITEMS=0, so N >= 4096 does not take hp_ntt_split.hip): polynomial counts around the LPW = 8 / 4 / 2 limbs per workgroup
of the inverse kernels at N = 2^11 / 2^12 / 2^13, item counts around the eight XCDs of hp_xcd_remap, and the digit-spread and drop
groups (HP_SPREAD_GROUP, HP_DROP_GROUP) against limb counts they do and do not divide -- up to the special prime standing alone in the
last group.  tests/test_host_ntt_items.py proves the numbering itself on the CPU; here the kernels have to use it correctly.

Whole output tensors, bit-exact against the oracle.  One wide (50-bit) limb and narrow (40-bit) ones under a 50-bit special prime, so
packed and plain digit rows mix; the largest canonical and the largest lazy word planted in the first coefficients.  Digit rows and
drop rows live in the context's workspace, where a row a launch fails to write may still hold the right words of an earlier call
on the same input: before every compared call the same call runs once on ANOTHER input of the same shape."""
import numpy as np
import pytest

import params as P
from oracle.pyoracle import SplitMix

pytestmark = pytest.mark.gpu
U = np.uint64
T = 65537
LPW = {11: 8, 12: 4, 13: 2}   # hp_ntt_tile.h: InvGeo


def chain(L):
    return [P.P50[1]] + P.P40[:L - 1] + [P.P50[0]]


def canon(a, mext):
    return a % np.array(mext[:a.shape[-2]], dtype=U)[:, None]


def plant(a, moduli):
    """q - 1 in the first words of the first polynomial, 2q - 1 in the next words of the last one (the same one in a batch of one)"""
    qv = np.array(moduli, dtype=U)[:, None]
    polys = a.reshape(-1, *a.shape[-2:])
    assert np.shares_memory(polys, a)
    polys[0][:, :5] = qv - U(1)
    polys[-1][:, 5:10] = U(2) * qv - U(1)
    return a


@pytest.fixture(scope="module")
def tiled_env():
    """the knob every engine of this file is created under (read once at hp_ctx_create)"""
    mp = pytest.MonkeyPatch()
    for k in ("HP_SPREAD_GROUP", "HP_DROP_GROUP", "HP_PARITY_LEVEL"):
        mp.delenv(k, raising=False)
    mp.setenv("HP_SPLIT_MAX_ITEMS", "0")
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def eng(tiled_env):
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.release_workspace()
    e.close()


# ---- transforms ----------------------------------------------------------------------------------------------------------------------
def _batches(logn):
    w = LPW[logn]
    return sorted({1, w - 1, w, w + 1, 2 * w + 1})


# N <= 8192: polynomial counts around the inverse kernels' group; N >= 16384 (one limb per workgroup): item counts around the XCD remap
# -- identity (W < 8), exact, with a tail, two rounds with a tail
TRANSFORMS = [(logn, L, B) for logn in (11, 12, 13) for L in (1, 3) for B in _batches(logn)] + \
             [(logn, 1, B) for logn in (14, 15) for B in (7, 8, 9, 17)]


@pytest.mark.parametrize("logn,L,B", TRANSFORMS)
def test_transforms_at_the_group_and_remap_edges(orc, eng, logn, L, B):
    n, Q = 1 << logn, chain(L)[:L]
    rng = SplitMix(7100 + 100 * logn + 10 * L + B)
    x = plant(rng.poly((B, L, n), Q), Q)
    other = rng.poly((B, L, n), Q)
    each = lambda f: np.stack([f(i) for i in range(B)])
    fwd = each(lambda i: orc.poly_ntt(Q, x[i]))
    inv = each(lambda i: orc.poly_intt(Q, fwd[i]))
    inv_strict = each(lambda i: orc.poly_reduce_strict(Q, inv[i]))
    dev, host = eng.to_device, eng.to_host

    def run(call, a):
        call(dev(other))
        return host(call(dev(a)))

    assert np.array_equal(run(lambda d: eng.ntt_(Q, d), x), fwd)
    assert np.array_equal(run(lambda d: eng.intt_(Q, d), fwd), inv)
    assert np.array_equal(run(lambda d: eng.intt_(Q, d, strict=True), fwd), inv_strict)
    assert np.array_equal(run(lambda d: eng.ntt_residues_(Q, d), x), canon(fwd, Q))
    assert np.array_equal(run(lambda d: eng.intt_residues_(Q, d), canon(fwd, Q)), inv_strict)


@pytest.mark.parametrize("logn,B", [(logn, B) for logn in (11, 12, 13) for B in _batches(logn)])
def test_drops_at_the_group_edges(orc, eng, logn, B):
    """the one-modulus inverse launch of 2B polynomials (strict epilogue; post-scalar epilogue for BGV), then the grouped drop launch"""
    n, L = 1 << logn, 3
    Q = chain(L)[:L]
    rng = SplitMix(7300 + 100 * logn + B)
    ct = plant(rng.poly((B, 2, L, n), Q), Q)
    other = rng.poly((B, 2, L, n), Q)
    each = lambda f: np.stack([f(i) for i in range(B)])
    rescale = each(lambda i: orc.ckks_rescale(Q, ct[i]))
    mod_switch = each(lambda i: orc.bgv_mod_drop(Q, T, ct[i]))
    dev, host = eng.to_device, eng.to_host
    for level, words in (("B", lambda w: w), ("A", lambda w: canon(w, Q))):
        eng.set_parity_level(level)
        try:
            eng.ckks_rescale(Q, dev(other))
            assert np.array_equal(host(eng.ckks_rescale(Q, dev(ct))), words(rescale)), level
            eng.bgv_mod_switch(Q, T, dev(other))
            assert np.array_equal(host(eng.bgv_mod_switch(Q, T, dev(ct))), words(mod_switch)), level
        finally:
            eng.set_parity_level("B")


# ---- group numbering -----------------------------------------------------------------------------------------------------------------
GROUP_LOGN = 11
GROUP_L = [2, 3, 4, 5, 7, 8, 9]   # with the default group of 4: a remainder, exactly one group, the special prime alone, ...
GROUP_B = [1, 3]
GROUPS = ["0", "1", "2", "3", None, "8", "32"]   # None: unset, the default of 4


@pytest.fixture(scope="module")
def group_cases(orc):
    """inputs, the other inputs run first, and the oracle's words: once per (L, B), shared by every setting, read-only"""
    n, out = 1 << GROUP_LOGN, {}
    for L in GROUP_L:
        mext = chain(L)
        Q = mext[:L]
        for B in GROUP_B:
            rng = SplitMix(7500 + 10 * L + B)
            ct1, ct2 = plant(rng.poly((B, 2, L, n), Q), Q), plant(rng.poly((B, 2, L, n), Q), Q)
            key = rng.poly((L, 2, L + 1, n), mext)
            o1, o2 = rng.poly((B, 2, L, n), Q), rng.poly((B, 2, L, n), Q)
            each = lambda f: np.stack([f(i) for i in range(B)])
            exp = {"ckks": each(lambda i: orc.ckks_mult(mext, ct1[i], ct2[i], key)),
                   "bgv": each(lambda i: orc.bgv_mult(mext, P.C5_T, ct1[i], ct2[i], key)),
                   "rot": each(lambda i: orc.ckks_rotate(mext, ct1[i], key, 3))}
            for v in exp.values():
                v.setflags(write=False)
            out[L, B] = (mext, ct1, ct2, key, o1, o2, exp)
    return out


@pytest.mark.parametrize("L", GROUP_L)
@pytest.mark.parametrize("group", GROUPS, ids=lambda g: "default" if g is None else f"G{g}")
def test_spread_and_drop_groups_at_every_remainder(group_cases, tiled_env, group, L):
    from hehub_amd.engine import Engine

    with tiled_env.context() as mp:
        if group is not None:
            mp.setenv("HP_SPREAD_GROUP", group)
            mp.setenv("HP_DROP_GROUP", group)
        e = Engine(0)      # the knobs are read here
    try:
        dev, host = e.to_device, e.to_host
        for B in GROUP_B:
            mext, ct1, ct2, key, o1, o2, exp = group_cases[L, B]
            d1, d2, dk, s1, s2 = dev(ct1), dev(ct2), dev(key), dev(o1), dev(o2)
            # level A: the canonical residues of the oracle's words after a drop, its residue in a lazy word after the rotation
            for level, fin in (("B", lambda w: w), ("A", lambda w: canon(w, mext))):
                e.set_parity_level(level)
                assert e.parity_level() == level
                e.ckks_mult(mext, s1, s2, dk)
                assert np.array_equal(host(e.ckks_mult(mext, d1, d2, dk)), fin(exp["ckks"])), (group, L, B, level)
                e.bgv_mult(mext, P.C5_T, s1, s2, dk)
                assert np.array_equal(host(e.bgv_mult(mext, P.C5_T, d1, d2, dk)), fin(exp["bgv"])), (group, L, B, level)
                e.ckks_rotate(mext, s1, dk, 3)
                rot = host(e.ckks_rotate(mext, d1, dk, 3))
                if level == "A":
                    assert (rot < U(2) * np.array(mext[:L], dtype=U)[:, None]).all(), (group, L, B)
                    rot = canon(rot, mext)
                assert np.array_equal(rot, fin(exp["rot"])), (group, L, B, level)
    finally:
        e.release_workspace()
        e.close()
