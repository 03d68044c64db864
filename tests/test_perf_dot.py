"""Timing of lazy relinearisation against the path it replaces (`pytest -m perf`, on an MI355X; not part of the correctness tiers:
tests/conftest.py).  N = 32768, L = 10, k = 4, alpha = 3, T = 8 terms, batch 1 and batch 32.
  * the call: T hp_dev_ckks_mult_relin_rescale_hks and one hp_dev_poly_fold_rows over their results, against ONE
    hp_dev_ckks_dot_relin_rescale_hks.  The one assertion is the condition for the feature to exist: ratio < 1.  By transform count it
    would be near 1 / T; no figure is fixed in advance.
  * the kernel alone: T hp_dev_mult_low_level and a fold of their quads, against one hp_dev_ckks_tensor_sum, asserted only to be not
    slower; its rate on 32 T + 24 bytes per output word is printed, to be set next to the coeffwise.mul and hbm_copy figures of a
    `bench.py --full` run of the same session.
The measured values and the per-family times of both sides are printed (`-s`) and recorded in DESIGN.md 4.7d."""
import statistics

import pytest

import params as P

pytestmark = pytest.mark.perf


@pytest.mark.parametrize("B", [1, 32])
def test_one_dot_call_is_not_slower_than_the_products_and_their_sum(B):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from hehub_amd.engine import Engine

    logn, L, k, alpha, T = 15, 10, 4, 3, 8
    n, nd = 1 << logn, (L + alpha - 1) // alpha
    mext = P.P40[:L] + P.P50[:k]
    q = mext[:L]
    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.use_stream(stream)
    try:
        with torch.cuda.stream(stream):
            gen = torch.Generator(device="cuda").manual_seed(23)
            rand = lambda *shape: torch.randint(0, 1 << 40, shape, dtype=torch.int64, device="cuda", generator=gen)   # words below q
            a = [rand(B, 2, L, n) for _ in range(T)]
            b = [rand(B, 2, L, n) for _ in range(T)]
            key = rand(nd, 2, L + k, n)
            prods = [eng.empty((B, 2, L - 1, n)) for _ in range(T)]
            total, total_dot = eng.empty((B, 2, L - 1, n)), eng.empty((B, 2, L - 1, n))
            quad_sum, quad_fold = eng.empty((B, 3, L, n)), eng.empty((B, 3, L, n))

            def dot():
                return eng.ckks_dot_hks(mext, k, alpha, a, b, key, out=total_dot)

            def products_then_sum():
                for t in range(T):
                    eng.ckks_mult_hks(mext, k, alpha, a[t], b[t], key, out=prods[t])
                chains = [[prods[t][p][h] for t in range(T)] for p in range(B) for h in range(2)]
                return eng.poly_fold_rows(q[:-1], chains, [False] * T, out=total.view(2 * B, L - 1, n))

            def tensor_sum():
                return eng.ckks_tensor_sum(q, a, b, out=quad_sum)

            def tensors_then_fold():
                quads = [eng.mult_low_level(q, a[t], b[t]) for t in range(T)]
                chains = [[quads[t][p][c] for t in range(T)] for p in range(B) for c in range(3)]
                return eng.poly_fold_rows(q, chains, [False] * T, out=quad_fold.view(3 * B, L, n))

            def median_ms(f, reps=5):
                f(); f()                                   # warmed: workspace, tables, allocator
                times = []
                for _ in range(reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    f()
                    e1.record(stream)
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1))
                return statistics.median(times)

            def families(f):
                eng.prof_begin("*")
                f()
                return eng.prof_end_families()

            t_base, t_dot = median_ms(products_then_sum), median_ms(dot)
            print(f"\nN=2^{logn} L={L} k={k} alpha={alpha} batch {B}, {T} terms: {T} mult_hks + sum {t_base:.3f} ms, dot {t_dot:.3f} ms, "
                  f"ratio {t_dot / t_base:.3f}")
            for name, f in ((f"{T} mult_hks + sum", products_then_sum), ("dot", dot)):
                print(name, {fam: (cnt, round(ms, 3)) for fam, (cnt, ms) in families(f).items()})
            t_fold, t_sum = median_ms(tensors_then_fold), median_ms(tensor_sum)
            gbytes = (32 * T + 24) * B * L * n / 1e9
            print(f"kernel alone, batch {B}: {T} mult_low_level + fold {t_fold:.3f} ms, tensor_sum {t_sum:.3f} ms, ratio {t_sum / t_fold:.3f}, "
                  f"{gbytes / (t_sum * 1e-3):.0f} GB/s on 32 T + 24 bytes per word")
            # (the two sides are not the same words, nor the same residues: T switches and T roundings against one of each)
            assert t_dot / t_base < 1.0, (t_dot, t_base)
            assert t_sum <= t_fold, (t_sum, t_fold)
    finally:
        eng.close()
