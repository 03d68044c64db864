"""One top-level hybrid key set at every level (the _at entry points, include/hehub_amd.h): the row map between a key generated for
key_L0 ciphertext moduli and the key of a level L <= key_L0, in plain numpy.  A hybrid key is [ceil(key_L0/alpha)][2][key_L0+k][n] and
a diagonal [key_L0+k][n]; level L reads digits d < ceil(L/alpha) and rows 0..L-1 (its ciphertext moduli) and key_L0..key_L0+k-1 (the
special primes).  No test, no fixture: tests/test_hks_levels_api.py and tests/test_gpu_hks_levels.py import from here."""
import numpy as np

from hks_model import chain


def top_chain(key_L0, k):
    """the chain the other hybrid tests use, at the top: 40-bit ciphertext moduli, then the special primes"""
    return chain(key_L0, k)


def level_rows(key_L0, L, k):
    """the rows of a top-level key digit (or diagonal) that level L reads, in the order of the level's chain"""
    assert 1 <= L <= key_L0
    return list(range(L)) + list(range(key_L0, key_L0 + k))


def level_chain(mext_top, key_L0, L, k):
    assert len(mext_top) == key_L0 + k
    return [mext_top[m] for m in level_rows(key_L0, L, k)]


def level_digits(L, alpha):
    return (L + alpha - 1) // alpha


def sub_key(key, key_L0, L, k, alpha):
    """[ceil(key_L0/alpha)][2][key_L0+k][n] -> the level's key [ceil(L/alpha)][2][L+k][n], a compact copy"""
    assert key.shape[:3] == (level_digits(key_L0, alpha), 2, key_L0 + k), key.shape
    return np.ascontiguousarray(key[:level_digits(L, alpha)][:, :, level_rows(key_L0, L, k)])


def sub_diag(diag, key_L0, L, k):
    """[key_L0+k][n] -> [L+k][n]; None (the constant 1, or an absent term) stays None"""
    if diag is None:
        return None
    assert diag.shape[0] == key_L0 + k, diag.shape
    return np.ascontiguousarray(diag[level_rows(key_L0, L, k)])


def embed_key(fill, key, key_L0, L, k, alpha):
    """the level key `key` planted into `fill`, a top-shaped key whose words come from another random stream (valid residues of the
    top chain's moduli): what the level does not read differs from anything a run at the level alone would hold, so a kernel that
    reads row m where it should read row km gets wrong words, not shifted ones"""
    top = fill.copy()
    rows = level_rows(key_L0, L, k)
    for d in range(level_digits(L, alpha)):
        top[d][:, rows] = key[d]
    assert np.array_equal(sub_key(top, key_L0, L, k, alpha), key)
    return top


def embed_diag(fill, diag, key_L0, L, k):
    top = fill.copy()
    top[level_rows(key_L0, L, k)] = diag
    return top
