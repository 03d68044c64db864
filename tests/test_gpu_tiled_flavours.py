"""The tiled transforms (hp_ntt_fast.hip, hp_ntt_a.hip over hp_ntt_tile.h) reached on purpose: small batches go through
hp_ntt_split.hip, so every case here opens its own engine with HP_SPLIT_MAX_ITEMS=0 and runs each compiled flavour of the fused drop
and both parity levels at the ring degrees whose code paths differ:
    N = 2048, 4096, 8192   eight / four / two limbs per workgroup in the inverse kernels, stream epilogue
    N = 16384        one limb per workgroup, layout-A store with passenger bits
    N = 32768        lane-pair loads / stores, padded exchange buffer
One wide (50-bit) and two narrow (40-bit) limbs under a 50-bit special prime; the largest canonical and the largest lazy word planted
in the first coefficients.  Level B gives hehub's raw words (ntt.cpp:155-223, rescaling.cpp:46-75, mod_switch.cpp:45-77,
rgsw.cpp:98-153), level A their residues: canonical after a drop, in a lazy word after the key switch and the rotation.
Flavour 0 (hybrid key switch: raw_input, comb) is tests/test_hks.py's."""
import numpy as np
import pytest

import params as P
from oracle.pyoracle import SplitMix

pytestmark = pytest.mark.gpu
U = np.uint64
MEXT = [P.P50[1], P.P40[0], P.P40[1], P.P50[0]]
L, B, T = 3, 2, 65537
Q = MEXT[:L]
LOGNS = [11, 12, 13, 14, 15]
_expected = {}


def canon(a):
    return a % np.array(MEXT[:a.shape[-2]], dtype=U)[:, None]


def expected(orc, logn):
    """inputs and the oracle's words, computed once per ring degree and shared by both levels"""
    if logn in _expected:
        return _expected[logn]
    n = 1 << logn
    rng = SplitMix(6600 + logn)
    qv = np.array(Q, dtype=U)[:, None]
    x = rng.poly((B, L, n), Q)
    x[0, :, :5] = qv - U(1)
    x[1, :, :5] = U(2) * qv - U(1)
    ct1, ct2 = rng.poly((B, 2, L, n), Q), rng.poly((B, 2, L, n), Q)
    key = rng.poly((L, 2, L + 1, n), MEXT)
    ct1[0, 0, :, :7] = qv - U(1)
    ct2[0, 1, :, :5] = U(2) * qv - U(1)
    each = lambda f: np.stack([f(i) for i in range(B)])
    quad = each(lambda i: orc.mult_low_level(Q, ct1[i], ct2[i]))
    fwd = each(lambda i: orc.poly_ntt(Q, x[i]))
    inv = each(lambda i: orc.poly_intt(Q, fwd[i]))
    e = {"x": x, "ct1": ct1, "ct2": ct2, "key": key, "quad": quad, "fwd": fwd, "inv": inv,
         "inv_strict": each(lambda i: orc.poly_reduce_strict(Q, inv[i])),
         "rescale": each(lambda i: orc.ckks_rescale(Q, ct1[i])),                       # flavour 1
         "relin": each(lambda i: orc.ckks_relinearize(MEXT, quad[i], key)),            # flavour 2
         "mod_switch": each(lambda i: orc.bgv_mod_drop(Q, T, ct2[i])),                 # flavour 3
         "bgv_relin": each(lambda i: orc.bgv_relinearize(MEXT, quad[i], key)),         # flavour 4
         "rotate": each(lambda i: orc.ckks_rotate(MEXT, ct1[i], key, 3)),              # flavour 5
         "ckks_mult": each(lambda i: orc.ckks_mult(MEXT, ct1[i], ct2[i], key)),        # level A: flavour 6, k_ntt_inv_mix_a
         "bgv_mult": each(lambda i: orc.bgv_mult(MEXT, T, ct1[i], ct2[i], key)),       # level A: flavour 7
         "ext": each(lambda i: orc.ext_prod(MEXT, quad[i, 2], key))}                   # spread, packed rows
    for name, v in e.items():
        if name not in ("x", "ct1", "ct2", "key", "quad", "fwd"):      # (what goes to the device is copied there; torch wants it writable)
            v.setflags(write=False)
    _expected[logn] = e
    return e


@pytest.mark.parametrize("level", ["B", "A"])
@pytest.mark.parametrize("logn", LOGNS)
def test_tiled_kernels_give_the_oracle_words(orc, monkeypatch, logn, level):
    from hehub_amd.engine import Engine

    e = expected(orc, logn)
    monkeypatch.setenv("HP_SPLIT_MAX_ITEMS", "0")
    eng = Engine(0)      # the knob is read here
    try:
        eng.set_parity_level(level)
        assert eng.parity_level() == level
        a = level == "A"
        words = canon if a else (lambda w: w)      # what a call that ends in a drop returns
        dev, host = eng.to_device, eng.to_host
        if a:   # hp_dev_ntt / hp_dev_intt stay at level B whatever the context's level: the FP64 transforms have their own entry points
            assert np.array_equal(host(eng.ntt_residues_(Q, dev(e["x"]))), canon(e["fwd"]))
            assert np.array_equal(host(eng.intt_residues_(Q, dev(e["fwd"]))), e["inv_strict"])
            assert np.array_equal(e["inv_strict"], canon(e["inv"]))
        y = eng.ntt_(Q, dev(e["x"]))
        assert np.array_equal(host(y), e["fwd"])
        assert np.array_equal(host(eng.intt_(Q, y)), e["inv"])
        assert np.array_equal(host(eng.intt_(Q, dev(e["fwd"]), strict=True)), e["inv_strict"])
        d1, d2, dk, dq = dev(e["ct1"]), dev(e["ct2"]), dev(e["key"]), dev(e["quad"])
        assert np.array_equal(host(eng.ckks_rescale(Q, d1)), words(e["rescale"]))
        assert np.array_equal(host(eng.ckks_relinearize(MEXT, dq, dk)), words(e["relin"]))
        assert np.array_equal(host(eng.bgv_mod_switch(Q, T, d2)), words(e["mod_switch"]))
        assert np.array_equal(host(eng.bgv_relinearize(MEXT, dq, dk)), words(e["bgv_relin"]))
        assert np.array_equal(host(eng.ckks_mult(MEXT, d1, d2, dk)), words(e["ckks_mult"]))
        assert np.array_equal(host(eng.bgv_mult(MEXT, T, d1, d2, dk)), words(e["bgv_mult"]))
        rot = host(eng.ckks_rotate(MEXT, d1, dk, 3))
        ext = host(eng.ext_prod(MEXT, dq[:, 2].contiguous(), dk))
        if a:   # hehub's residue in a lazy word
            assert np.array_equal(canon(rot), canon(e["rotate"])) and np.array_equal(canon(ext), canon(e["ext"]))
            assert (rot < U(2) * np.array(Q, dtype=U)[:, None]).all() and (ext < U(2) * np.array(MEXT, dtype=U)[:, None]).all()
        else:
            assert np.array_equal(rot, e["rotate"]) and np.array_equal(ext, e["ext"])
    finally:
        eng.release_workspace()
        eng.close()
