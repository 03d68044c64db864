"""The exact model of lazy relinearisation (hp_dev_ckks_tensor_sum, hp_dev_ckks_dot_relin_rescale_hks): the quadratic sum in Python
integers modulo each q_i, then the pieces every hybrid multiplication is already held to -- model_switch of tests/hks_model.py, the
oracle's poly_add and ckks_rescale.  The device and the model may hand the switch DIFFERENT representatives of sum d2 (the model's are
canonical), so every comparison built on this is on strict residues plus "every word below 2q" (tests/test_dot_model.py shows that
model_switch's residues do not depend on the representative).  No test, no fixture; needs no GPU."""
import numpy as np

from hks_model import model_switch

U = np.uint64


def model_tensor_sum(q, a_list, b_list):
    """a_list[t], b_list[t]: one ciphertext [2][L][n] each (any u64 words) -> the canonical residues of
    (sum a0 b0, sum (a0 b1 + a1 b0), sum a1 b1), [3][L][n] (dtype object)"""
    L, n = a_list[0].shape[1:]
    out = np.zeros((3, L, n), dtype=object)
    for a, b in zip(a_list, b_list):
        ao, bo = a.astype(object), b.astype(object)
        out[0] += ao[0] * bo[0]
        out[1] += ao[0] * bo[1] + ao[1] * bo[0]
        out[2] += ao[1] * bo[1]
    for i, m in enumerate(q):
        out[:, i] %= m
    return out


def model_dot(orc, logn, mext, L, k, alpha, a_list, b_list, key):
    """one ciphertext per term -> rescale(sum (d0, d1) + switch(sum d2)), [2][L-1][n] words (compare on strict residues)"""
    q = mext[:L]
    quad = model_tensor_sum(q, a_list, b_list).astype(U)
    sw = model_switch(orc, logn, mext, L, k, alpha, np.ascontiguousarray(quad[2]), key)
    lin = np.stack([orc.poly_add(q, sw[0], np.ascontiguousarray(quad[0])), orc.poly_add(q, sw[1], np.ascontiguousarray(quad[1]))])
    return orc.ckks_rescale(q, lin)


def strict_rows(rows, moduli):
    """[..., L, n] u64 words -> their canonical residues"""
    return rows % np.array(moduli, dtype=U)[:, None]


def below_2q(rows, moduli):
    return bool((rows < 2 * np.array(moduli, dtype=U)[:, None]).all())
