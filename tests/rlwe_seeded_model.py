"""The exact model of the seeded ciphertext calls (include/hehub_amd.h: hp_dev_sample_small_ntt, hp_dev_rlwe_encrypt_seeded,
hp_dev_rlwe_encrypt_pk_seeded) in Python integers: the draws of tests/sample_model.py, the oracle's forward transform followed by
poly_reduce_strict, and plain % arithmetic.  Every word of the three calls is pinned by it (tests/test_gpu_rlwe_seeded.py); what the
model itself computes is checked on the CPU by tests/test_rlwe_seeded_model.py.

Ids: small_ntt and encrypt_seeded use stream + b for polynomial / ciphertext b; encrypt_pk_seeded uses stream + 2b (u_b: ternary, e0_b:
centred binomial -- the kind tag keeps them apart) and stream + 2b + 1 (e1_b)."""
import numpy as np

import sample_model as S

U = np.uint64


def ids_used(call, stream, batch):
    """the polynomial ids a call draws from, as the header documents them"""
    count = 2 * batch if call == "encrypt_pk_seeded" else batch
    return [(stream + i) & S.M64 for i in range(count)]


def chain_supports(orc, logn, moduli):
    """the chain admits the ring degree (distinct primes = 1 mod 2N) and the oracle's forward transform leaves words below 2q on it, so
    that poly_reduce_strict of them is the canonical residue"""
    import params as P

    n = 1 << logn
    if len(set(moduli)) != len(moduli) or not all(P.is_prime(q) and q % (2 * n) == 1 for q in moduli):
        return False
    edge = np.stack([np.full(n, q - 1, dtype=U) for q in moduli])
    edge[:, ::3] = 1
    w = orc.poly_ntt(moduli, edge)
    return bool((w < 2 * np.array(moduli, dtype=U)[:, None]).all())


def residues(moduli, values):
    """signed Python integers [n] -> u64 [L][n], plain %"""
    return np.array([[int(v) % q for v in values] for q in moduli], dtype=U)


def forward(orc, moduli, rows):
    """coefficient rows [L][n] -> the canonical words of their forward transform"""
    w = orc.poly_ntt(moduli, np.ascontiguousarray(rows, dtype=U))
    assert bool((w < 2 * np.array(moduli, dtype=U)[:, None]).all())
    return orc.poly_reduce_strict(moduli, w)


def small_row(kind, logn, seed, stream):
    return (S.ternary_row if kind == S.TERNARY else S.cbd_row)(logn, seed, stream & S.M64)


def small_ntt(orc, logn, moduli, kind, seed, stream, scale=1, batch=1):
    """-> u64 [batch][L][n]: NTT(scale * the sample of id stream + b), canonical"""
    return np.stack([forward(orc, moduli, residues(moduli, [scale * int(v) for v in small_row(kind, logn, seed, stream + b)]))
                     for b in range(batch)])


def _obj(a):
    return np.asarray(a).astype(object)


def _mod(rows, moduli):
    return np.array([[int(v) % q for v in row] for row, q in zip(rows, moduli)], dtype=U)


def encrypt_seeded(orc, logn, moduli, s_ntt, pt, seed, stream, scale=1, with_c1=True, batch=None):
    """s_ntt [L][n] (NTT form, any representative), pt [B][L][n] coefficient rows or None (zero; `batch` ciphertexts)
    -> [B][2][L][n] = (NTT(scale e) + NTT(pt) - a s, a), or [B][L][n] = c0 alone"""
    B = len(pt) if pt is not None else (batch or 1)
    out = []
    for b in range(B):
        a = S.sample_uniform(logn, moduli, seed, (stream + b) & S.M64)[0]
        c0 = _obj(small_ntt(orc, logn, moduli, S.CBD, seed, stream + b, scale)[0]) - _obj(a) * _obj(s_ntt)
        if pt is not None:
            c0 = c0 + _obj(forward(orc, moduli, pt[b]))
        c0 = _mod(c0, moduli)
        out.append(np.stack([c0, a]) if with_c1 else c0)
    return np.stack(out)


def encrypt_pk_seeded(orc, logn, moduli, pk, pt, seed, stream, scale=1, batch=None):
    """pk [2][L][n] (NTT form), pt [B][L][n] coefficient rows or None -> [B][2][L][n] = (pk0 u + e0 + pt, pk1 u + e1)"""
    B = len(pt) if pt is not None else (batch or 1)
    out = []
    for b in range(B):
        u = _obj(small_ntt(orc, logn, moduli, S.TERNARY, seed, stream + 2 * b)[0])
        e0 = _obj(small_ntt(orc, logn, moduli, S.CBD, seed, stream + 2 * b, scale)[0])
        e1 = _obj(small_ntt(orc, logn, moduli, S.CBD, seed, stream + 2 * b + 1, scale)[0])
        c0 = _obj(pk[0]) * u + e0
        if pt is not None:
            c0 = c0 + _obj(forward(orc, moduli, pt[b]))
        out.append(np.stack([_mod(c0, moduli), _mod(_obj(pk[1]) * u + e1, moduli)]))
    return np.stack(out)


# ---- what a ciphertext decrypts to (Python integers) ---------------------------------------------------------------------------------
def centred(x, q):
    x = int(x) % q
    return x - q if x > q // 2 else x


def decrypt_coefficients(orc, moduli, ct, s_ntt):
    """ct [2][L][n], s_ntt [L][n] -> the coefficients of c0 + c1 s, u64 [L][n] below q"""
    lhs = _mod(_obj(ct[0]) + _obj(ct[1]) * _obj(s_ntt), moduli)
    return _mod(orc.poly_intt(moduli, lhs), moduli)


def negacyclic(a, b):
    """schoolbook product of two integer polynomials modulo x^n + 1"""
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        x = int(x)
        if x == 0:
            continue
        for j, y in enumerate(b):
            k = i + j
            if k < n:
                out[k] += x * int(y)
            else:
                out[k - n] -= x * int(y)
    return out
