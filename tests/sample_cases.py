"""What the sampling tests share: the fixed seeds, the shapes the GPU tests run (tests/test_gpu_sample.py) -- which the host
implementation is held to as well (tests/test_sample_host.py) -- their model references, computed once and left unchanged, and the
planted candidate sequences of the uniform word rule."""
import functools

import numpy as np

import moduli as M
import params as P
import sample_model as S

SEED = bytes((7 * i + 1) & 255 for i in range(32))
SEED2 = bytes((11 * i + 3) & 255 for i in range(32))
HEAVY = [M.PACK40EDGE[1], 65537, P.P50[0], M.Q59]   # two moduli just above a power of two (every other word redrawn), a wide word
FIVE = P.P40[:3] + P.P50[:2]

# id: (logn, moduli, batch, stream, limb_ids)
UNIFORM_CASES = {
    "one_block": (3, P.P40[:1], 1, 5, None),
    "table": (5, P.P40[:2] + P.P50[:1], 1, 6, None),
    "heavy_rejection": (6, HEAVY, 1, 7, None),
    "largest_block_index": (16, P.P40[:1], 1, 8, None),
    "carry_into_word_15": (5, P.P40[:2], 2, (1 << 32) - 1, None),
    "carry_into_bit_63": (3, P.P40[:1], 2, (1 << 64) - 1, None),   # (the id wraps: 64-bit arithmetic)
    "limb_ids": (5, [FIVE[0], FIVE[1], FIVE[4]], 1, 9, [0, 1, 4]),
}
STRIDE_CASE = (12, P.P40[:1] + P.P50[:1], 3, 10)   # logn, moduli, batch, stream; stride = L * N + 64
SIGNED_LOGN = (3, 5, 11)
SIGNED_BATCH, SIGNED_STREAM = 2, 21
KEYGEN_CASES = [(5, 4, 2, 2, 1), (6, 5, 2, 3, 3), (11, 3, 2, 2, 2)]   # logn, L, k, alpha, keys
KEYGEN_STREAM = 1000


@functools.lru_cache(maxsize=None)
def _uniform(logn, moduli, seed, stream, ids, batch):
    out = S.sample_uniform(logn, list(moduli), seed, stream, None if ids is None else list(ids), batch)
    out.setflags(write=False)
    return out


def model_uniform(logn, moduli, stream, ids=None, batch=1, seed=SEED):
    return _uniform(logn, tuple(moduli), seed, stream, None if ids is None else tuple(ids), batch)


@functools.lru_cache(maxsize=None)
def model_signed(kind, logn, stream=SIGNED_STREAM, batch=SIGNED_BATCH, seed=SEED):
    out = (S.sample_ternary if kind == S.TERNARY else S.sample_cbd)(logn, seed, stream, batch)
    out.setflags(write=False)
    return out


PLANT_MODULI = [2, 3, 65537, M.PACK40EDGE[1], P.P50[0], M.Q59, (1 << 63) - 1]


def planted_sequences(q):
    """[(64 candidates, the word, candidates used)]: accepted at attempt 0, 1 and 63, and all 64 rejected.  Junk above the mask shows
    that the mask is applied."""
    bits = q.bit_length()
    mask = (1 << bits) - 1
    junk = (0xA5A5A5A5A5A5A5A5 << bits) & S.M64
    rej = [junk | (q + (i % (mask - q + 1))) for i in range(S.ATTEMPTS)]   # every masked value in q .. mask
    assert all(q <= (v & mask) <= mask for v in rej)
    last = rej[-1] & mask
    return [
        ([junk | (q - 1)] + rej[1:], q - 1, 1),
        ([rej[0], junk | 0] + rej[2:], 0, 2),
        (rej[:63] + [junk | (q // 2)], q // 2, 64),
        (rej, last - q, 64),
    ]
