"""The level-aware hybrid entry points at the C boundary (CPU tier: nothing is launched): include/hehub_amd.h declares an _at form of
every hybrid call that takes a key -- the plain call's parameters with key_L0 after L -- hehub_amd/capi.py carries them as the plain
call's with a size_t after L, and the Engine methods take key_L0 (exported, typed as the header types them, refusing a NULL
context: every call, tests/test_capi_symbols.py).  Then the claim
the feature rests on, in plain integers: the digits of a level are contained in the top-level digits of the same index, and the row
map of tests/hks_levels.py selects exactly the level's rows.  What the calls compute: tests/test_gpu_hks_levels.py."""
import inspect

import numpy as np

import abi
from hks_levels import level_chain, level_rows, sub_diag, sub_key, top_chain
from hks_model import digits_of

PLAIN = ("hp_dev_hks_switch", "hp_dev_ckks_rotate_hks", "hp_dev_ckks_conjugate_hks", "hp_dev_ckks_rotate_hoisted_hks",
         "hp_dev_ckks_lintrans_hks", "hp_dev_ckks_lintrans_bsgs_hks", "hp_dev_ckks_mult_relin_rescale_hks",
         "hp_dev_ckks_relin_rescale_hks", "hp_dev_ckks_dot_relin_rescale_hks")
CALLS = tuple(name + "_at" for name in PLAIN)
METHODS = ("hks_switch", "ckks_rotate_hks", "ckks_conjugate_hks", "ckks_rotate_hoisted_hks", "ckks_lintrans_hks",
           "ckks_lintrans_bsgs_hks", "ckks_mult_hks", "ckks_relin_rescale_hks", "ckks_dot_hks")


def test_header_declares_the_calls_with_key_L0_after_L():
    for name in PLAIN:
        plain, at = abi.parameter_names(name), abi.parameter_names(name + "_at")
        assert len(at) == len(plain) + 1, name
        i = plain.index("L")
        assert at == plain[:i + 1] + ["key_L0"] + plain[i + 1:], name


def test_ctypes_table_has_the_header_argument_counts():
    from hehub_amd import capi

    for name in PLAIN:
        res, args = capi.SIGNATURES[name + "_at"]
        plain_args = capi.SIGNATURES[name][1]
        assert res is capi.INT and len(args) == len(abi.parameter_names(name + "_at")) == len(plain_args) + 1 and args[0] is capi.P, name
        assert args == plain_args[:3] + [capi.szt] + plain_args[3:], name   # (ctx, logn, L, key_L0, ...)


def test_engine_methods_take_key_L0():
    from hehub_amd.engine import Engine

    for method in METHODS:
        p = inspect.signature(getattr(Engine, method)).parameters.get("key_L0")
        assert p is not None and p.default is None, method


SHAPES = [(key_L0, L, alpha) for key_L0 in range(1, 13) for L in range(1, key_L0 + 1) for alpha in range(1, 5)]


def test_level_digits_lie_inside_the_top_digits():
    for key_L0, L, alpha in SHAPES:
        top, level = digits_of(key_L0, alpha), digits_of(L, alpha)
        assert len(level) == (L + alpha - 1) // alpha <= (key_L0 + alpha - 1) // alpha == len(top)
        for d, limbs in enumerate(level):
            assert limbs and set(limbs) <= set(top[d]), (key_L0, L, alpha, d)
            assert limbs == [m for m in top[d] if m < L]        # exactly the top digit's limbs below L, in order
        assert sorted(m for limbs in level for m in limbs) == list(range(L))


def test_sub_key_selects_exactly_the_level_rows():
    """a top key whose word (d, h, m) names itself: the sub-key holds the words of digits d < ceil(L/alpha), of rows 0..L-1 and
    key_L0..key_L0+k-1, in that order -- and the chain of those rows is the level's chain"""
    n = 2
    for key_L0, L, alpha in SHAPES:
        for k in (1, 3):
            KE, ndt, nd = key_L0 + k, (key_L0 + alpha - 1) // alpha, (L + alpha - 1) // alpha
            d, h, m, i = np.meshgrid(np.arange(ndt), np.arange(2), np.arange(KE), np.arange(n), indexing="ij")
            top = (((d * 2 + h) * KE + m) * n + i).astype(np.uint64)
            sub = sub_key(top, key_L0, L, k, alpha)
            assert sub.shape == (nd, 2, L + k, n)
            rows = list(range(L)) + list(range(key_L0, key_L0 + k))
            assert level_rows(key_L0, L, k) == rows
            for dd in range(nd):
                for hh in range(2):
                    for j, mm in enumerate(rows):
                        assert list(sub[dd, hh, j]) == [((dd * 2 + hh) * KE + mm) * n + ii for ii in range(n)]
            diag = np.arange(KE * n, dtype=np.uint64).reshape(KE, n)
            assert [int(w) for w in sub_diag(diag, key_L0, L, k)[:, 0]] == [mm * n for mm in rows]
            assert sub_diag(None, key_L0, L, k) is None
            mext = list(range(100, 100 + KE))                   # (stand-ins: the prime table ends before key_L0 = 12)
            assert level_chain(mext, key_L0, L, k) == mext[:L] + mext[key_L0:]
    # at the top the map is the identity
    top = np.arange(3 * 2 * 7 * n, dtype=np.uint64).reshape(3, 2, 7, n)
    assert np.array_equal(sub_key(top, 5, 5, 2, 2), top)
    # the top chains of the GPU tier: distinct primes, the existing tests' chain at the top
    for key_L0, k in ((4, 2), (5, 2), (6, 3), (7, 1), (8, 2), (5, 9)):
        mext = top_chain(key_L0, k)
        assert len(mext) == len(set(mext)) == key_L0 + k
