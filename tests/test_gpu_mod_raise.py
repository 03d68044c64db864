"""hp_dev_ckks_mod_raise (hp_ntt_raise.hip: k_ntt_raise, and the composed form of the other ring degrees, of launches of few
transforms and of parity level A) against the three calls it replaces -- hp_dev_intt (strict) on limb row 0,
hp_dev_rns_base_from_single, hp_dev_ntt -- residue for residue in every modulus, and against the integer model
(tests/bootstrap_model.py), which does not share the engine's lift.  Words are below 2q, row 0 is canonical.

The input is built in the COEFFICIENT domain: uniform coefficients modulo q_0 with 0, 1, half - 1, half, half + 1, q_0 - 1 planted
(half = q_0 // 2, where the centring changes sides), transformed on the host, and handed in as words in [q_0, 2 q_0).  Operands
are stored with in_limbs limbs of which only row 0 may be read: the other rows hold words that would change the answer.

Shapes: the ring degrees without tiled kernels (3, 10, 16), every tiled degree, L - 1 below, at and above the group of moduli the
launch numbers its items by, more than one polynomial per group.  Launches of at most 128 transforms at N >= 4096 take the split-limb
path (the composed form), so every tiled shape runs a second time on an engine with that path switched off: the fused kernel."""
import numpy as np
import pytest

import params as P
from bootstrap_model import model_mod_raise, planted_coefficients
from oracle.pyoracle import SplitMix

pytestmark = pytest.mark.gpu
U = np.uint64
SHAPES = [(3, 2, 1, 1), (10, 3, 2, 1), (11, 2, 1, 1), (11, 13, 3, 3), (12, 5, 2, 1), (13, 4, 1, 2), (15, 3, 1, 1), (16, 2, 1, 1)]
TILED = [s for s in SHAPES if 11 <= s[0] <= 15] + [(14, 6, 1, 1)]


def chain(logn, L, bits0=50, bits=40):
    """q_0 of bits0 bits over L - 1 moduli of `bits` bits, all = 1 (mod 2N), off the prime table"""
    q0 = P.ntt_primes(1, logn, bits0)[0]
    return [q0] + P.ntt_primes(L - 1, logn, bits, exclude=(q0,))


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture
def eng_tiled(monkeypatch):
    """an engine whose transform launches never take the split-limb path: the knob is read when the context is created"""
    from hehub_amd.engine import Engine

    monkeypatch.setenv("HP_SPLIT_MAX_ITEMS", "0")
    e = Engine(0)
    yield e
    e.close()


_inputs = {}


def inputs(orc, logn, q, batch, in_limbs):
    """(ct u64[batch][2][in_limbs][N], model rows u64[batch][2][L][N]) for a chain, computed once and left unchanged"""
    key = (logn, tuple(q), batch, in_limbs)
    if key not in _inputs:
        n, q0 = 1 << logn, q[0]
        rng = SplitMix(7700 + 31 * logn + len(q) + batch)
        ct = np.empty((batch, 2, in_limbs, n), dtype=U)
        want = np.empty((batch, 2, len(q), n), dtype=U)
        for b in range(batch):
            for h in range(2):
                words = orc.ntt(logn, q0, planted_coefficients(rng, n, q0)) % U(q0)
                ct[b, h, 0] = words + U(q0)                       # every word in [q_0, 2 q_0)
                for r in range(1, in_limbs):
                    ct[b, h, r] = rng.words(n, 1 << 62)           # never read
                want[b, h], _ = model_mod_raise(orc, logn, q, ct[b, h, 0])
        ct.setflags(write=False)
        want.setflags(write=False)
        _inputs[key] = (ct, want)
    return _inputs[key]


def three_calls(e, q, ct):
    """the composition the call replaces, on the device: residues u64[batch][2][L][N]"""
    batch, _, _, n = ct.shape
    x = e.to_device(np.ascontiguousarray(ct[:, :, :1, :]).reshape(2 * batch, 1, n))
    e.intt_([q[0]], x, strict=True)
    lifted = e.rns_base_from_single(q[0], q, x.reshape(2 * batch, n))
    return e.to_host(e.ntt_(q, lifted)).reshape(batch, 2, len(q), n) % np.array(q, dtype=U)[:, None]


def check(e, orc, logn, q, batch, in_limbs, canonical=False):
    ct, want = inputs(orc, logn, q, batch, in_limbs)
    qv = np.array(q, dtype=U)[:, None]
    got = e.to_host(e.ckks_mod_raise(q, e.to_device(ct.copy())))
    assert got.shape == want.shape
    assert (got < U(2) * qv).all()
    assert (got[:, :, 0] < U(q[0])).all() and np.array_equal(got[:, :, 0], ct[:, :, 0] - U(q[0]))     # a strict copy
    if canonical:
        assert (got < qv).all()
    assert np.array_equal(got % qv, three_calls(e, q, ct))
    assert np.array_equal(got % qv, want)


@pytest.mark.parametrize("logn,L,batch,in_limbs", SHAPES)
def test_residues_equal_the_three_calls(eng, orc, logn, L, batch, in_limbs):
    check(eng, orc, logn, chain(logn, L), batch, in_limbs)


@pytest.mark.parametrize("logn,L,batch,in_limbs", TILED)
def test_the_fused_launch(eng_tiled, orc, logn, L, batch, in_limbs):
    """(14, 6): five moduli per polynomial = one full group of four and a remainder"""
    check(eng_tiled, orc, logn, chain(logn, L), batch, in_limbs)


@pytest.mark.parametrize("bits0,bits", [(59, 30), (30, 59)])
@pytest.mark.parametrize("logn,L,batch,in_limbs", [(3, 2, 1, 1), (11, 13, 3, 3), (13, 4, 1, 2)])
def test_wide_and_narrow_chains(eng, eng_tiled, orc, logn, L, batch, in_limbs, bits0, bits):
    """a 59-bit q_0 over 30-bit moduli (floor(q_0 / q) is 29 bits wide), a 30-bit q_0 under 59-bit moduli (every lift is below q)"""
    q = chain(logn, L, bits0, bits)
    assert q[0].bit_length() == bits0 and all(m.bit_length() == bits for m in q[1:])
    check(eng, orc, logn, q, batch, in_limbs)
    if logn >= 12:
        check(eng_tiled, orc, logn, q, batch, in_limbs)


@pytest.mark.parametrize("logn,L,batch,in_limbs", [(10, 3, 2, 1), (11, 13, 3, 3), (15, 3, 1, 1)])
def test_parity_level_a(orc, logn, L, batch, in_limbs):
    """a 50-bit q_0 over 40-bit moduli at level A: every word canonical (N = 1024 has no level-A transforms: level B's words)"""
    from hehub_amd.engine import Engine

    e = Engine(0)
    try:
        e.set_parity_level("A")
        check(e, orc, logn, chain(logn, L), batch, in_limbs, canonical=logn >= 11)
    finally:
        e.close()


def test_refusals_leave_the_output_untouched(eng):
    from hehub_amd import capi

    logn, L, in_limbs, batch = 4, 3, 2, 1
    n = 1 << logn
    q = chain(logn, L)
    x = eng.to_device(SplitMix(7800).poly((batch, 2, in_limbs, n), q[:in_limbs]))
    out = eng.empty((batch, 2, L, n))
    out.fill_(7)
    xp, op = x.data_ptr(), out.data_ptr()

    def call(logn_=logn, L_=L, mods=q, in_limbs_=in_limbs, batch_=batch, src=xp, dst=op):
        m = None if mods is None else (capi.u64 * len(mods))(*mods)
        return eng.lib.hp_dev_ckks_mod_raise(eng.h, logn_, L_, m, in_limbs_, batch_, capi.P(src), capi.P(dst))

    assert call() == capi.HP_OK             # the call as such is fine
    eng.sync()
    out.fill_(7)
    E = capi.HP_EINVAL
    assert call(L_=1) == E and call(L_=33, mods=q + [q[0]] * 30) == E
    assert call(in_limbs_=0) == E and call(in_limbs_=33) == E
    assert call(batch_=0) == E
    assert call(mods=None) == E and call(src=None) == E and call(dst=None) == E
    assert call(src=xp + 8) == E and call(dst=op + 8) == E
    assert call(dst=xp) == E                                                    # the output is the input
    assert call(dst=xp + (2 * in_limbs * n - 2) * 8) == E                       # ... or begins in its last words
    assert call(src=op + (2 * L * n - 2) * 8) == E                              # the input begins in the output's last words
    assert call(mods=[q[0], q[1], q[0]]) == E and call(mods=[q[0], q[1], q[1]]) == E
    assert call(mods=[q[0], q[1], q[2] + 2]) == E                               # 2N does not divide q - 1
    U_ = capi.HP_EUNSUPPORTED
    assert call(mods=[q[0], q[1], P.ntt_primes(1, logn, 61)[0]]) == U_          # beyond the transforms' 59 bits
    assert call(mods=[P.ntt_primes(1, logn, 61)[0], q[1], q[2]]) == U_
    assert call(logn_=17) == U_
    eng.sync()
    assert (eng.to_host(out) == 7).all()
