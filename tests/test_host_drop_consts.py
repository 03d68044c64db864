"""Host-side logic without a GPU: the constants of the fused drop launches, hehub_amd/csrc/hp_drop.cpp.

Every word the builders produce is compared with a big-integer model written here: inverses are inverses, a Harvey word is
floor(v 2^64 / q), a level-A pair is the doubles (v, v / q), and the products A, m, m2, B, K of the two-drop flavour follow the
DropPre2A comment of hp_ntt_a.hip -- so a wrong constant is caught here, before any GPU run."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "cpp", "libdrop_shim.so")
CSRC = os.path.join(ROOT, "hehub_amd", "csrc")
HEAD = ["q_last", "half_q_last", "bgv", "small_rem", "raw_input", "out_stride", "fin_on", "comb_half", "q2_last", "half_q2_last", "L",
        "add_poly_stride", "add_ct_stride", "add_mask", "x", "addend", "out", "comb"]
ROWS = ["r", "inv", "inv_h", "t", "t_h", "qlt", "qlt_h", "fin", "fin_h", "comb_r", "comb_mul", "comb_mul_h"]
ML = 32   # HP_MAX_LIMBS

EXTRA40 = P.ntt_primes(ML - 14, 11, 40, exclude=P.P40)
CHAINS = {
    "one_limb_remains": P.P40[:2],
    "mixed": [P.P50[1]] + P.P40[:4] + [P.P50[0]],     # the last modulus exceeds 2 q_k for the 40-bit limbs
    "all40": P.P40[:5],
    "array_bound": P.P40 + EXTRA40 + P.P50,           # HP_MAX_LIMBS moduli
}
SMALL_REM = {"one_limb_remains": 1, "mixed": 0, "all40": 1, "array_bound": 0}
SCHEMES = [(0, 0), (1, 65537), (1, 2), (1, 1)]   # (bgv, t)
HKS = {(4, 2, 2): [P.P50[1]] + P.P40[:3] + P.P50[2:4], (3, 1, 1): P.P40[:3] + [P.P50[0]], (2, 9, 1): P.P40[:2] + P.P40[2:10] + [P.P50[0]]}


@pytest.fixture(scope="module")
def ds():
    src = [os.path.join(ROOT, "tests", "cpp", "drop_shim.cpp"), os.path.join(CSRC, "hp_drop.cpp"), os.path.join(CSRC, "hp_tables.cpp")]
    dep = src + [os.path.join(CSRC, "hp_drop.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in dep):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO] + src, check=True)
    lib = C.CDLL(SO)
    u, z, i, p = C.c_uint64, C.c_size_t, C.c_int, C.c_void_p
    lib.ds_a_pair.argtypes = [u, u, p]
    lib.ds_drop_args.argtypes = [u, z, u, z, z, C.c_uint, z, u, z, p]
    lib.ds_drop.argtypes = [p, z, z, z, i, u, i, p]
    lib.ds_post_scalar.argtypes = [u, u, i, p]
    lib.ds_two_drop.argtypes = [p, z, i, u, u, p, p]
    lib.ds_hks_limbs.argtypes = [p, z, z, p]
    lib.ds_hks_down.argtypes = [p, z, z, z, z, i, p]
    lib.ds_hks_down_rescale.argtypes = [p, z, z, u, i, p]
    lib.ds_flavours.argtypes = [i, i, i, i, C.c_uint, i, i, p]
    assert lib.ds_max_limbs() == ML
    return lib


# ---- the model -----------------------------------------------------------------------------------------------------------------
def harvey(v, q):
    return (v << 64) // q


def f64(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def a_pair(v, q):
    return f64(v), struct.unpack("<Q", struct.pack("<d", float(v) / float(q)))[0]


def inverse(v, q):
    w = pow(v % q, -1, q)
    assert w * v % q == 1
    return w


def blank():
    d = {h: 0 for h in HEAD}
    d.update({r: [0] * ML for r in ROWS})
    return d


def put(d, name, i, pair):
    d[name][i], d[name + "_h"][i] = pair


def model_drop(chain, k0, k1, bgv, t, level_a):
    """drop_consts + drop_small_rem [+ drop_consts_to_a] for the limbs [k0, k1) of chain[:-1]"""
    ql, d = chain[-1], blank()
    pair = a_pair if level_a else (lambda v, q: (v, harvey(v, q)))
    d["q_last"], d["half_q_last"] = (f64(ql), f64(ql // 2)) if level_a else (ql, ql // 2)
    d["bgv"] = bgv
    d["small_rem"] = int(all(ql <= 2 * q for q in chain[k0:k1]))
    for i, q in enumerate(chain[k0:k1]):
        d["r"][i] = ql % q
        put(d, "inv", i, pair(inverse(ql, q), q))
        put(d, "t", i, pair(t % q if bgv else 0, q))
        put(d, "qlt", i, pair((ql % t) % q if bgv else 0, q))
    return d


def two_drop_products(q, p, q2, bgv, t1, t2):
    """hp_ntt_a.hip, DropPre2A: A = p^-1 [(p mod t1)], m = A [t1], m2 = 1 [t2], B = q'^-1 [(q' mod t2)]   (bracketed: BGV)"""
    A = inverse(p, q) * ((p % t1) if bgv else 1) % q
    m = A * (t1 if bgv else 1) % q
    m2 = (t2 if bgv else 1) % q
    B = inverse(q2, q) * ((q2 % t2) if bgv else 1) % q if q != q2 else None
    return A, m, m2, B


def model_two_drop(ext, bgv, t1, t2):
    L, p, q2, d = len(ext) - 1, ext[-1], ext[-2], blank()
    d["bgv"] = bgv
    d["q_last"], d["half_q_last"], d["q2_last"], d["half_q2_last"] = f64(p), f64(p // 2), f64(q2), f64(q2 // 2)
    for k, q in enumerate(ext[:L - 1]):
        A, m, m2, B = two_drop_products(q, p, q2, bgv, t1, t2)
        put(d, "inv", k, a_pair(A, q)); put(d, "t", k, a_pair(m, q)); put(d, "comb_mul", k, a_pair(m2, q)); put(d, "qlt", k, a_pair(B, q))
    A, K, _, _ = two_drop_products(q2, p, q2, bgv, t1, t2)   # the combined limb: K = m of that limb
    return d, list(a_pair(A, q2) + a_pair(K, q2)) + [f64(p), f64(p // 2)]


def model_hks_limbs(mext, L, k):
    Pp = math.prod(mext[L:L + k])
    pinv = [inverse(Pp, q) for q in mext[:L]]
    pmq = [Pp % q for q in mext[:L]]
    return pinv, [harvey(v, q) for v, q in zip(pinv, mext)], pmq, [harvey(v, q) for v, q in zip(pmq, mext)]


def raw_rows_a(d):
    d["raw_input"], d["bgv"], d["q_last"], d["half_q_last"] = 0, 0, f64(0), f64(2 ** 62)


def model_hks_down(mext, L, k, i0, cnt, level_a):
    pinv, pinv_h, _, _ = model_hks_limbs(mext, L, k)
    d = blank()
    d["raw_input"] = 1
    for i in range(cnt):
        put(d, "inv", i, (pinv[i0 + i], pinv_h[i0 + i]))
    if level_a:
        raw_rows_a(d)
        for i in range(cnt):
            put(d, "inv", i, a_pair(pinv[i0 + i], mext[i0 + i]))
    return d


def model_hks_down_rescale(mext, L, k, comb, level_a):
    pinv, _, pmq, pmq_h = model_hks_limbs(mext, L, k)
    ql = mext[L - 1]
    d = model_hks_down(mext, L, k, 0, L - 1, False)
    d["fin_on"], d["comb"], d["comb_half"] = 1, comb, (ql // 2 if comb else 0)
    for i, q in enumerate(mext[:L - 1]):
        put(d, "comb_mul", i, (pmq[i], pmq_h[i]))
        d["comb_r"][i] = ql % q
        put(d, "fin", i, (inverse(ql, q), harvey(inverse(ql, q), q)))
    if level_a:   # the two-drop flavour: A = m = P^-1, m2 = 1, B = q_last^-1
        raw_rows_a(d)
        d["fin_on"], d["q2_last"], d["half_q2_last"] = 0, f64(ql), f64(ql // 2)
        for i, q in enumerate(mext[:L - 1]):
            put(d, "inv", i, a_pair(pinv[i], q)); put(d, "t", i, a_pair(pinv[i], q))
            put(d, "comb_mul", i, a_pair(1, q)); put(d, "qlt", i, a_pair(inverse(ql, q), q))
    return d


# ---- the builders ----------------------------------------------------------------------------------------------------------------
def arr(v):
    return np.array(v, dtype=np.uint64)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def parse(words):
    d = {h: int(words[i]) for i, h in enumerate(HEAD)}
    for i, r in enumerate(ROWS):
        d[r] = [int(x) for x in words[18 + i * ML: 18 + (i + 1) * ML]]
    return d


def call(fn, *args):
    out = np.full(18 + 12 * ML, 0xDEAD, dtype=np.uint64)
    fn(*args, ptr(out))
    return parse(out)


def same(got, exp):
    for key in HEAD + ROWS:
        assert got[key] == exp[key], key


def test_level_a_pair_and_common_fields(ds):
    for v, q in [(0, P.P40[0]), (1, P.P40[0]), (P.P40[0] - 1, P.P40[0]), (P.P50[0] - 1, P.P50[0]), (12345678901, P.P50[1])]:
        out = np.zeros(2, dtype=np.uint64)
        ds.ds_a_pair(v, q, ptr(out))
        assert (int(out[0]), int(out[1])) == a_pair(v, q)
    exp = blank()
    exp.update(x=0x1000, L=7, addend=0x2000 + 5 * 8, add_poly_stride=6, add_ct_stride=18, add_mask=3, out=0x3000, out_stride=5)
    same(call(ds.ds_drop_args, 0x1000, 7, 0x2000, 6, 18, 3, 5, 0x3000, 5), exp)
    exp = blank()   # no rows: no addend, whatever the mask says
    exp.update(x=0x1000, L=7, out=0x3000, out_stride=5)
    same(call(ds.ds_drop_args, 0x1000, 7, 0, 6, 18, 3, 5, 0x3000, 5), exp)


@pytest.mark.parametrize("name", list(CHAINS))
def test_one_drop(ds, name):
    chain = CHAINS[name]
    L = len(chain)
    for bgv, t in SCHEMES:
        for level_a in (0, 1):
            got = call(ds.ds_drop, ptr(arr(chain)), L, 0, L - 1, bgv, t, level_a)
            same(got, model_drop(chain, 0, L - 1, bgv, t, level_a))
            assert got["small_rem"] == SMALL_REM[name]


def test_one_drop_of_a_limb_range_starts_at_index_zero(ds):
    chain = [P.P50[1]] + P.P40[:3] + [P.P50[0]]
    for bgv, t in SCHEMES:
        for level_a in (0, 1):
            got = call(ds.ds_drop, ptr(arr(chain)), 5, 1, 3, bgv, t, level_a)
            same(got, model_drop(chain, 1, 3, bgv, t, level_a))
            whole = model_drop(chain, 0, 4, bgv, t, level_a)
            assert got["inv"][:2] == whole["inv"][1:3] and got["r"][:2] == whole["r"][1:3] and got["inv"][2] == 0
    # 40-bit limbs under a 50-bit last modulus; the 50-bit limb alone is within a factor of two
    assert call(ds.ds_drop, ptr(arr(chain)), 5, 1, 3, 0, 0, 0)["small_rem"] == 0
    assert call(ds.ds_drop, ptr(arr(chain)), 5, 0, 1, 0, 0, 0)["small_rem"] == 1


def test_post_scalar(ds):
    for q in (P.P40[1], P.P50[0]):
        for t in (65537, 2, 1):
            s = inverse(t, q)
            for level_a, exp in ((0, (s, harvey(s, q))), (1, a_pair(s, q))):
                out = np.zeros(2, dtype=np.uint64)
                ds.ds_post_scalar(t, q, level_a, ptr(out))
                assert (int(out[0]), int(out[1])) == exp


TWO_DROP_CHAINS = {
    "one_limb_remains": [P.P50[1], P.P40[0], P.P50[0]],   # L = 2
    "mixed": CHAINS["mixed"],
    "all40": CHAINS["all40"],
    "array_bound": CHAINS["array_bound"],                 # L + 1 = HP_MAX_LIMBS
}


@pytest.mark.parametrize("name", list(TWO_DROP_CHAINS))
def test_two_drops(ds, name):
    ext = TWO_DROP_CHAINS[name]
    # CKKS; BGV with the reference's relinearise quirk (inner t = 1) and t in {65537, 2, 1}; BGV with the true t in both drops
    for bgv, t1, t2 in [(0, 0, 0), (1, 1, 65537), (1, 1, 2), (1, 1, 1), (1, 65537, 65537)]:
        out = np.full(18 + 12 * ML, 0xDEAD, dtype=np.uint64)
        mx = np.zeros(6, dtype=np.uint64)
        ds.ds_two_drop(ptr(arr(ext)), len(ext) - 1, bgv, t1, t2, ptr(out), ptr(mx))
        exp, exp_mx = model_two_drop(ext, bgv, t1, t2)
        same(parse(out), exp)
        assert [int(v) for v in mx] == exp_mx


@pytest.mark.parametrize("shape", list(HKS))
def test_hybrid(ds, shape):
    (L, k, _alpha), mext = shape, HKS[shape]
    assert len(mext) == L + k
    m = arr(mext)
    out = np.zeros(4 * L, dtype=np.uint64)
    assert ds.ds_hks_limbs(ptr(m), L, k, ptr(out)) == 1
    assert [int(v) for v in out] == sum(model_hks_limbs(mext, L, k), [])
    for level_a in (0, 1):
        same(call(ds.ds_hks_down, ptr(m), L, k, 0, L, level_a), model_hks_down(mext, L, k, 0, L, level_a))
        same(call(ds.ds_hks_down, ptr(m), L, k, L - 1, 1, level_a), model_hks_down(mext, L, k, L - 1, 1, level_a))
        same(call(ds.ds_hks_down_rescale, ptr(m), L, k, 0x4000, level_a), model_hks_down_rescale(mext, L, k, 0x4000, level_a))
    same(call(ds.ds_hks_down_rescale, ptr(m), L, k, 0, 0), model_hks_down_rescale(mext, L, k, 0, 0))   # the combination as its own kernel


def test_hybrid_rejects_a_special_prime_that_is_a_ciphertext_modulus(ds):
    out = np.zeros(8, dtype=np.uint64)
    assert ds.ds_hks_limbs(ptr(arr([P.P40[0], P.P40[1], P.P40[0]])), 2, 1, ptr(out)) == 0


# ---- which compiled flavour a launch takes (hp_drop_flavour_b / hp_drop_flavour_a) -----------------------------------------------
# level B, without fin_on / raw_input / comb: by (addend in effect, add_mask, bgv); everything else is the run-time flavour 0
FLAV_B = {("none", 0): 1, ("none", 1): 3,      # no addend (no rows, or mask 0): rescale / mod_switch
          (3, 0): 2, (3, 1): 4,                # both polynomials: relinearize
          (1, 0): 5, (1, 1): 0,                # polynomial 0 only: rotation (CKKS); BGV has no such kernel
          (2, 0): 0, (2, 1): 0}                # polynomial 1 only: no such kernel
# level A: no kernel at all for fin_on / raw_input, nor for comb without an addend on both polynomials
FLAV_A = {("none", 0): 1, ("none", 1): 3, (3, 0): 2, (3, 1): 4, (1, 0): 5, (1, 1): -1, (2, 0): -1, (2, 1): -1}
FLAV_A_TWO = {0: 6, 1: 7}                      # comb and addend on both polynomials: two drops in one transform, CKKS / BGV


def test_flavour_tables(ds):
    seen_b, seen_a = set(), set()
    for fin_on in (0, 1):
        for raw_input in (0, 1):
            for comb in (0, 1):
                for addend in (0, 1):
                    for mask in (0, 1, 2, 3):
                        for bgv in (0, 1):
                            for small_rem in (0, 1):
                                out = np.zeros(2, dtype=np.int32)
                                fa = ds.ds_flavours(fin_on, raw_input, comb, addend, mask, bgv, small_rem, ptr(out))
                                fb, small = int(out[0]), int(out[1])
                                add = mask if addend and mask else "none"
                                exp_b = 0 if fin_on or raw_input or comb else FLAV_B[(add, bgv)]
                                if fin_on or raw_input:
                                    exp_a = -1
                                elif comb:
                                    exp_a = FLAV_A_TWO[bgv] if add == 3 else -1
                                else:
                                    exp_a = FLAV_A[(add, bgv)]
                                case = (fin_on, raw_input, comb, addend, mask, bgv, small_rem)
                                assert fb == exp_b and small == int(exp_b != 0 and small_rem == 1), case
                                assert fa == exp_a if exp_a > 0 else fa < 0, case
                                seen_b.add((fb, small)); seen_a.add(max(fa, -1))
    assert seen_b == {(0, 0)} | {(f, s) for f in range(1, 6) for s in (0, 1)} and seen_a == {-1, 1, 2, 3, 4, 5, 6, 7}
    # spelled out: the launches that fall to flavour 0 at level B although nothing run-time-only is asked for
    for mask, bgv in ((2, 0), (2, 1), (1, 1)):
        out = np.zeros(2, dtype=np.int32)
        assert ds.ds_flavours(0, 0, 0, 1, mask, bgv, 1, ptr(out)) < 0 and (int(out[0]), int(out[1])) == (0, 0)
