"""The device samplers' model (include/hehub_amd.h: hp_dev_sample_*; hehub_amd/csrc/hp_sample.h has the same layout in C++): a
counter-based ChaCha20 keystream (RFC 8439 section 2.3, 20 rounds) and three rules over it, in Python integers for single words and
numpy for whole rows.  Everything is a function of (seed, stream).

State words: 0-3 the ChaCha constants; 4-11 the 32 seed bytes as little-endian u32; 12 the block index j; 13 = attempt (bits 0-15) |
kind << 16 | limb_id << 24; 14, 15 the low / high half of the 64-bit polynomial id `stream`.  Block j serves coefficients 8j .. 8j+7;
coefficient 8j + c owns the candidate v_c = o[2c] | o[2c+1] << 32 of the block's 16 output words."""
import numpy as np

UNIFORM, TERNARY, CBD = 1, 2, 3
ATTEMPTS = 64
ETA = 21
CONSTANTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
U32, U64 = np.uint32, np.uint64


def word13(attempt, kind, limb_id):
    return (attempt & 0xFFFF) | (kind << 16) | (limb_id << 24)


def seed_words(seed):
    assert len(seed) == 32
    return [int.from_bytes(seed[4 * i:4 * i + 4], "little") for i in range(8)]


def states(seed, j, w13, stream):
    """[len(j)][16] u32: the states of the blocks j (array) under word 13 = w13 (scalar or array)"""
    j = np.asarray(j, dtype=U32)
    s = np.empty((len(j), 16), dtype=U32)
    s[:, 0:4] = CONSTANTS
    s[:, 4:12] = seed_words(seed)
    s[:, 12] = j
    s[:, 13] = w13
    s[:, 14] = stream & M32
    s[:, 15] = (stream >> 32) & M32
    return s


def _rotl(x, n):
    return (x << U32(n)) | (x >> U32(32 - n))


def _quarter(x, a, b, c, d):
    x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)


def chacha20_blocks(state):
    """state [B][16] u32 -> the output words [B][16] u32 of every block"""
    state = np.ascontiguousarray(state, dtype=U32)
    x = [state[:, i].copy() for i in range(16)]
    for _ in range(10):
        _quarter(x, 0, 4, 8, 12); _quarter(x, 1, 5, 9, 13); _quarter(x, 2, 6, 10, 14); _quarter(x, 3, 7, 11, 15)
        _quarter(x, 0, 5, 10, 15); _quarter(x, 1, 6, 11, 12); _quarter(x, 2, 7, 8, 13); _quarter(x, 3, 4, 9, 14)
    return np.stack(x, axis=1) + state


def candidates(out):
    """[B][16] u32 -> [B][8] u64: v_c = o[2c] | o[2c+1] << 32, the keystream bytes 8c .. 8c+7 little-endian"""
    out = out.astype(U64)
    return out[:, 0::2] | (out[:, 1::2] << U64(32))


# ---- the three rules on single words (Python integers) ---------------------------------------------------------------------------------
def uniform_word(q, cands):
    """the word of a candidate sequence (attempt 0, 1, ...): the first w = v & (2^bit_length(q) - 1) below q; after 64 rejected
    attempts w - q of the last candidate"""
    assert 2 <= q < 1 << 63
    mask = (1 << q.bit_length()) - 1
    it = iter(cands)
    for _ in range(ATTEMPTS):
        w = next(it) & mask
        if w < q:
            return w
    return w - q


def ternary_word(v):
    for f in range(32):
        field = (v >> (2 * f)) & 3
        if field != 3:
            return field - 1
    return 0


def cbd_word(v):
    m = (1 << ETA) - 1
    return bin(v & m).count("1") - bin((v >> ETA) & m).count("1")


# ---- whole rows ----------------------------------------------------------------------------------------------------------------------
def uniform_row(n, q, seed, stream, limb_id):
    """-> (row [n] u64, redraws [n]: how many candidates every word rejected)"""
    assert n >= 8 and n % 8 == 0 and 2 <= q < 1 << 63 and 0 <= limb_id < 256
    mask = U64((1 << q.bit_length()) - 1)
    row = (candidates(chacha20_blocks(states(seed, np.arange(n // 8), word13(0, UNIFORM, limb_id), stream))) & mask).reshape(n)
    redraws = np.zeros(n, dtype=np.int64)
    pending = np.nonzero(row >= U64(q))[0]
    for attempt in range(1, ATTEMPTS):
        if len(pending) == 0:
            break
        redraws[pending] += 1
        out = chacha20_blocks(states(seed, pending // 8, word13(attempt, UNIFORM, limb_id), stream))
        row[pending] = candidates(out)[np.arange(len(pending)), pending % 8] & mask
        pending = pending[row[pending] >= U64(q)]
    row[pending] -= U64(q)   # 64 rejected candidates
    return row, redraws


def sample_uniform(logn, moduli, seed, stream, limb_ids=None, batch=1):
    """-> u64 [batch][L][n]: polynomial b has the id stream + b (64-bit), row m the label limb_ids[m] (default m)"""
    n = 1 << logn
    ids = list(range(len(moduli))) if limb_ids is None else limb_ids
    return np.stack([np.stack([uniform_row(n, q, seed, (stream + b) & M64, i)[0] for q, i in zip(moduli, ids)]) for b in range(batch)])


def _signed_candidates(kind, logn, seed, stream):
    n = 1 << logn
    assert n >= 8
    return candidates(chacha20_blocks(states(seed, np.arange(n // 8), word13(0, kind, 0), stream))).reshape(n)


def ternary_row(logn, seed, stream):
    v = _signed_candidates(TERNARY, logn, seed, stream)
    res = np.zeros(len(v), dtype=np.int64)
    for f in range(31, -1, -1):   # the lowest field that is not 3 wins: written last
        field = ((v >> U64(2 * f)) & U64(3)).astype(np.int64)
        res = np.where(field != 3, field - 1, res)
    return res


def _popcount(x):
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8).reshape(len(x), 8), axis=1).sum(axis=1).astype(np.int64)


def cbd_row(logn, seed, stream):
    v = _signed_candidates(CBD, logn, seed, stream)
    m = U64((1 << ETA) - 1)
    return _popcount(v & m) - _popcount((v >> U64(ETA)) & m)


def sample_ternary(logn, seed, stream, batch=1):
    return np.stack([ternary_row(logn, seed, (stream + b) & M64) for b in range(batch)])


def sample_cbd(logn, seed, stream, batch=1):
    return np.stack([cbd_row(logn, seed, (stream + b) & M64) for b in range(batch)])


def keystream_bytes(seed, w13, stream, blocks):
    """the raw keystream of the blocks 0 .. blocks-1, as `openssl enc -chacha20` produces it over zero bytes"""
    return chacha20_blocks(states(seed, np.arange(blocks), w13, stream)).astype("<u4").tobytes()


def openssl_iv(w13, stream):
    """the 16-byte -iv that puts block index 0, word 13 and the stream id into state words 12 .. 15"""
    return (0).to_bytes(4, "little") + w13.to_bytes(4, "little") + stream.to_bytes(8, "little")
