"""Timing of the baby-step giant-step diagonal transform against the flat call (`pytest -m perf`, on an MI355X; not part of the
correctness tiers: tests/conftest.py).  Baseline: one hp_dev_ckks_lintrans_hks with R keys and R diagonals.  Candidate: one
hp_dev_ckks_lintrans_bsgs_hks with sqrt(R) x sqrt(R) entries and R diagonals.  Every rotation has its OWN key tensor: one reused 29 MB
key would sit in the Infinity Cache and flatter the flat call.  The one assertion is the condition for the feature to exist as a speed
feature: at R = 256 (16 x 16; the flat call then holds 7.5 GB of keys) the candidate is not slower.  R = 64 (8 x 8) is timed and printed
without an assertion: by the byte counts the two should be close there.  No ratio is fixed in advance because none can be derived --
except for the one accumulate kernel the launches sit at their latency floor at batch 1.  The measured values and the
per-family times are printed (`-s`) and recorded in DESIGN.md 4.7b."""
import statistics

import pytest

import params as P

pytestmark = pytest.mark.perf


def test_bsgs_is_not_slower_than_the_flat_call_at_256_diagonals():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from hehub_amd.engine import Engine

    logn, L, k, alpha = 15, 10, 4, 3
    n, nd = 1 << logn, (L + alpha - 1) // alpha
    mext = P.P40[:L] + P.P50[:k]
    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.use_stream(stream)
    try:
        with torch.cuda.stream(stream):
            gen = torch.Generator(device="cuda").manual_seed(19)
            rand = lambda *shape: torch.randint(0, 1 << 40, shape, dtype=torch.int64, device="cuda", generator=gen)   # level B takes any words
            ct = rand(1, 2, L, n)

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

            ratios = {}
            for side in (8, 16):
                R = side * side
                diags = [rand(L + k, n) for _ in range(R)]
                keys = [rand(nd, 2, L + k, n) for _ in range(R)]           # R distinct keys
                steps = list(range(1, R + 1))
                flat = lambda: eng.ckks_lintrans_hks(mext, k, alpha, ct, keys, steps, diags)
                t_flat, f_flat = median_ms(flat), families(flat)
                stream.synchronize()
                del flat
                bkeys, gkeys = keys[:side], keys[side:2 * side]             # 2 sqrt(R) of them, distinct
                del keys
                torch.cuda.empty_cache()
                bsteps, gsteps = list(range(side)), [side * g for g in range(side)]
                grid = [diags[g * side:(g + 1) * side] for g in range(side)]
                bsgs = lambda: eng.ckks_lintrans_bsgs_hks(mext, k, alpha, ct, bkeys, bsteps, gkeys, gsteps, grid)
                t_bsgs, f_bsgs = median_ms(bsgs), families(bsgs)
                stream.synchronize()
                ratios[R] = t_bsgs / t_flat
                print(f"\nN=2^{logn} L={L} k={k} alpha={alpha} batch 1, {R} diagonals: flat ({R} keys) {t_flat:.3f} ms, "
                      f"bsgs ({side} x {side}, {2 * side} keys) {t_bsgs:.3f} ms, ratio {ratios[R]:.3f}")
                for name, fam in (("flat", f_flat), ("bsgs", f_bsgs)):
                    print(name, {fa: (cnt, round(ms, 3)) for fa, (cnt, ms) in fam.items()})
                del bsgs, bkeys, gkeys, diags, grid
                torch.cuda.empty_cache()
            assert ratios[256] < 1.0, ratios
    finally:
        eng.close()
