"""The discrete Gaussian sampler's model (include/hehub_amd.h: hp_dev_sample_gauss, kind 4; hehub_amd/csrc/hp_sample.h has the same
rule in C++), over the keystream of tests/sample_model.py.

sigma = 16/5 exactly.  rho(k) = exp(-25 k^2 / 512), S = the sum of rho over all integers; a magnitude m has P(0) = rho(0) / S and
P(m) = 2 rho(m) / S.  The table: C[m] = floor(2^63 * (P(0) + ... + P(m))), m = 0 .. 29.  The word of a candidate v: sign = v & 1,
u = v >> 1 (63 bits), m = #{i : u >= C[i]}; -m where sign = 1 and m != 0, else m.  Kind tag 4 in word 13, attempt 0, limb id 0.

The table is computed here, in decimal arithmetic of PRECISION digits (far more than the 200 bits asked for); the C++ literals are
held to it by tests/test_gauss_host.py."""
import functools
from decimal import Decimal, localcontext

import numpy as np

import sample_model as S

GAUSS = 4
ENTRIES = 30
PRECISION = 120      # decimal digits: about 400 bits
TAIL = 200           # rho(200) = exp(-1953) is far below 10^-PRECISION
U64 = np.uint64


def _rho(k):
    return (Decimal(-25 * k * k) / Decimal(512)).exp()


@functools.lru_cache(maxsize=None)
def probabilities(count=64):
    """exact P(m), m = 0 .. count-1, as Decimals (PRECISION digits)"""
    with localcontext() as ctx:
        ctx.prec = PRECISION
        total = _rho(0) + 2 * sum(_rho(k) for k in range(1, TAIL))
        return tuple((_rho(m) if m == 0 else 2 * _rho(m)) / total for m in range(count))


@functools.lru_cache(maxsize=None)
def scaled_cumulatives(count):
    """2^63 * (P(0) + .. + P(m)) for m = 0 .. count-1, as Decimals"""
    with localcontext() as ctx:
        ctx.prec = PRECISION
        out, acc = [], Decimal(0)
        for p in probabilities(max(count, 64))[:count]:
            acc += p
            out.append(acc * (1 << 63))
        return tuple(out)


def table(count=ENTRIES):
    return [int(x) for x in scaled_cumulatives(count)]   # (int() of a positive Decimal truncates: the floor)


def variance():
    with localcontext() as ctx:
        ctx.prec = PRECISION
        total = _rho(0) + 2 * sum(_rho(k) for k in range(1, TAIL))
        return 2 * sum(k * k * _rho(k) for k in range(1, TAIL)) / total


TABLE = table()


def gauss_word(v):
    u = v >> 1
    m = sum(1 for c in TABLE if u >= c)
    return -m if (v & 1) and m else m


def gauss_row(logn, seed, stream):
    v = S._signed_candidates(GAUSS, logn, seed, stream & S.M64)
    m = np.searchsorted(np.array(TABLE, dtype=U64), v >> U64(1), side="right").astype(np.int64)   # entries <= u
    return np.where((v & U64(1)) == U64(1), -m, m)


def sample_gauss(logn, seed, stream, batch=1):
    return np.stack([gauss_row(logn, seed, (stream + b) & S.M64) for b in range(batch)])


def residues(moduli, row, scale=1):
    """signed coefficients [n] -> u64 [L][n]: scale * row modulo every modulus, plain %"""
    return np.array([[scale * int(v) % q for v in row] for q in moduli], dtype=U64)


def sample_small(logn, moduli, seed, stream, scale=1, batch=1, id_step=1):
    """-> u64 [batch][L][n]: the coefficient rows k_gauss_spread writes"""
    return np.stack([residues(moduli, gauss_row(logn, seed, stream + b * id_step), scale) for b in range(batch)])
