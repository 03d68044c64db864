"""Helpers the GPU test files share word for word.  A helper whose body or contract differs from these stays in its own file
(test_gpu_hks_levels.at_both_levels, test_gpu_bfv.at_levels, test_gpu_gauss.strict, the canon()s, the eng fixtures)."""
import numpy as np

U = np.uint64


def dev_i64(eng, x):
    return eng.torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to(f"cuda:{eng.device}")


def residues(x, q):
    return x % np.array(q, dtype=U)[:, None]


def strict(moduli, a):
    """reduce_strict per limb (mod_arith.h:58-72): a [..., L, n] of lazy words below 2q"""
    q = np.array(moduli, dtype=U)[:, None]
    return np.where(a >= q, a - q, a)


def case_id(c):
    return "-".join(str(x) for x in c)


def at_both_levels(eng, run):
    """{level: run()} at parity level B and in a level-A context (which keeps level B where the chain is not eligible)"""
    got = {}
    for level in ("B", "A"):
        eng.set_parity_level(level)
        try:
            got[level] = run()
            eng.sync()
        finally:
            eng.set_parity_level("B")
    return got
