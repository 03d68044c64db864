"""What the seeded-ciphertext tests share (tests/test_rlwe_seeded_model.py on the CPU, tests/test_gpu_rlwe_seeded.py on the device):
chains, shapes, inputs, and the model references of tests/rlwe_seeded_model.py, computed once and left unchanged.

Shapes.  logn 3: one block per row -- L = 3, batch = 3 is a 9-thread launch with a tail; logn 5; logn 11: the first tiled transform
size, full workgroups (256 blocks per row).  L in {1, 3}, batch in {1, 3}, error_scale in {1, 65537}, each value with each ring
degree.  TABLE is a chain of tests/params.py; HEAVY holds two moduli of sample_cases.HEAVY just above a power of two, where every
other uniform word is redrawn, so the redraw loop runs inside the fused kernel (tests/test_rlwe_seeded_model.py checks that both
chains admit every ring degree used).  The HEAVY cases keep error_scale = 1: hp_dev_rlwe_encrypt_core, one of the references, lifts
its noise without a division and is defined for |noise| < q only, and 65537 is one of the moduli."""
import numpy as np

import moduli as M
import params as P
import rlwe_seeded_model as R
import sample_cases as K
import sample_model as S
from oracle.pyoracle import SplitMix

TABLE = P.P40[:2] + P.P50[:1]
HEAVY = [P.P40[0], M.PACK40EDGE[1], 65537]
assert M.PACK40EDGE[1] in K.HEAVY and 65537 in K.HEAVY

# id: (logn, moduli, batch, error_scale, stream)
CASES = {
    "n8_L3_B3": (3, TABLE, 3, 1, 3000),
    "n8_L1_B1_t": (3, TABLE[:1], 1, 65537, 3010),
    "n32_L3_B1_t": (5, TABLE, 1, 65537, 3020),
    "n32_L1_B3": (5, TABLE[:1], 3, 1, (1 << 32) - 2),     # (the ids carry into word 15)
    "n2048_L3_B3_t": (11, TABLE, 3, 65537, 3040),
    "n2048_L1_B1": (11, TABLE[:1], 1, 1, 3050),
    "heavy_n32_L3_B3": (5, HEAVY, 3, 1, 3060),
    "heavy_n2048_L3_B1": (11, HEAVY, 1, 1, 3070),
}
SECRET_STREAM, PK_STREAM, PK_ENC_OFFSET = 500, 7000, 100000
SMALL_SCALES = (1, 65537, (1 << 58) - 1)

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def secret(logn):
    """the ternary coefficients of the secret"""
    return _once(("s", logn), lambda: S.ternary_row(logn, K.SEED2, SECRET_STREAM))


def secret_ntt(orc, logn, moduli):
    return _once(("sn", logn, tuple(moduli)), lambda: R.small_ntt(orc, logn, moduli, S.TERNARY, K.SEED2, SECRET_STREAM)[0])


def plaintext(name):
    logn, moduli, batch, _, stream = CASES[name]
    return _once(("pt", name), lambda: SplitMix(stream).poly((batch, len(moduli), 1 << logn), moduli))


def model_ct(orc, name):
    logn, moduli, batch, scale, stream = CASES[name]
    return _once(("ct", name), lambda: R.encrypt_seeded(orc, logn, moduli, secret_ntt(orc, logn, moduli), plaintext(name), K.SEED, stream, scale))


def model_pk(orc, name):
    """pk = (e - a s, a): the zero-plaintext ciphertext of the id PK_STREAM under the case's error_scale"""
    logn, moduli, _, scale, _ = CASES[name]
    return _once(("pk", name), lambda: R.encrypt_seeded(orc, logn, moduli, secret_ntt(orc, logn, moduli), None, K.SEED2, PK_STREAM, scale)[0])


def model_pk_ct(orc, name):
    logn, moduli, batch, scale, stream = CASES[name]
    return _once(("pkct", name), lambda: R.encrypt_pk_seeded(orc, logn, moduli, model_pk(orc, name), plaintext(name), K.SEED,
                                                              stream + PK_ENC_OFFSET, scale))
