"""Timing of the double-hoisted diagonal transform against the path it replaces (`pytest -m perf`, on an MI355X; not part of the
correctness tiers: tests/conftest.py).  Baseline: one hp_dev_ckks_rotate_hoisted_hks, the products of its R results with the
diagonals (one hp_dev_poly_mul per rotation over both polynomials) and their sum (one hp_dev_poly_fold_rows).  Candidate: one
hp_dev_ckks_lintrans_hks.  The one assertion is the condition for the feature to exist: the candidate is not slower.  By transform
count the ratio would be near (56 + 28) / (56 + 16 * 28) = 0.167; the measured value and the per-family times are printed (`-s`) and
recorded in DESIGN.md 4.7a."""
import statistics

import pytest

import params as P

pytestmark = pytest.mark.perf


def test_one_lintrans_call_is_not_slower_than_hoisted_rotations_and_the_weighted_sum():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from hehub_amd.engine import Engine

    logn, L, k, alpha, R = 15, 10, 4, 3, 16
    n, nd = 1 << logn, (L + alpha - 1) // alpha
    mext = P.P40[:L] + P.P50[:k]
    q = mext[:L]
    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.use_stream(stream)
    try:
        with torch.cuda.stream(stream):
            gen = torch.Generator(device="cuda").manual_seed(17)
            rand = lambda *shape: torch.randint(0, 1 << 40, shape, dtype=torch.int64, device="cuda", generator=gen)   # level B takes any words
            ct = rand(1, 2, L, n)
            keys = [rand(nd, 2, L + k, n) for _ in range(R)]
            diags = [rand(L + k, n) for _ in range(R)]
            steps = list(range(1, R + 1))
            # the baseline's operands, laid out once: the ciphertext part of every diagonal, for both polynomials; its buffers
            diags_q = [d[:L].unsqueeze(0).expand(2, L, n).contiguous() for d in diags]
            prods = [eng.empty((2, L, n)) for _ in range(R)]
            total = eng.empty((2, L, n))

            def lintrans():
                return eng.ckks_lintrans_hks(mext, k, alpha, ct, keys, steps, diags)

            def hoisted_then_sum():
                rot = eng.ckks_rotate_hoisted_hks(mext, k, alpha, ct, keys, steps)[0]          # [R][2][L][n]
                for r in range(R):
                    eng.poly_mul(q, rot[r], diags_q[r], out=prods[r])
                return eng.poly_fold_rows(q, [[prods[r][h] for r in range(R)] for h in range(2)], [False] * R, out=total)

            def median_ms(f, reps=5):
                f(); f()                                   # warmed: workspace, tables, maps, allocator
                times = []
                for _ in range(reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    f()
                    b.record(stream)
                    b.synchronize()
                    times.append(a.elapsed_time(b))
                return statistics.median(times)

            def families(f):
                eng.prof_begin("*")
                f()
                return eng.prof_end_families()

            t_base, t_lin = median_ms(hoisted_then_sum), median_ms(lintrans)
            print(f"\nN=2^{logn} L={L} k={k} alpha={alpha} batch 1, {R} rotations: hoisted + {R} products + sum {t_base:.3f} ms, "
                  f"lintrans {t_lin:.3f} ms, ratio {t_lin / t_base:.3f}")
            for name, f in (("hoisted + products + sum", hoisted_then_sum), ("lintrans", lintrans)):
                print(name, {fam: (cnt, round(ms, 3)) for fam, (cnt, ms) in families(f).items()})
            assert t_lin / t_base < 1.0, (t_lin, t_base)
    finally:
        eng.close()
