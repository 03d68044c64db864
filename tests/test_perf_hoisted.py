"""Timing of the hoisted rotations against the unhoisted path (`pytest -m perf`, on an MI355X; not part of the correctness tiers:
tests/conftest.py).  The one assertion is the condition for the feature to exist: 16 rotations through
hp_dev_ckks_rotate_hoisted_hks are not slower than 16 calls of hp_dev_ckks_rotate_hks on the same context.  By transform count the
ratio would be near (28 + 56 / 16) / 84 = 0.38 plus what the gather costs; the measured value and the per-family times are printed
(`-s`) and recorded in DESIGN.md."""
import statistics

import pytest

import params as P

pytestmark = pytest.mark.perf


def test_sixteen_hoisted_rotations_are_not_slower_than_sixteen_calls():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from hehub_amd.engine import Engine

    logn, L, k, alpha, R = 15, 10, 4, 3, 16
    n, nd = 1 << logn, (L + alpha - 1) // alpha
    mext = P.P40[:L] + P.P50[:k]
    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.use_stream(stream)
    try:
        with torch.cuda.stream(stream):
            gen = torch.Generator(device="cuda").manual_seed(16)
            rand = lambda *shape: torch.randint(0, 1 << 40, shape, dtype=torch.int64, device="cuda", generator=gen)   # level B takes any words
            ct = rand(1, 2, L, n)
            keys = [rand(nd, 2, L + k, n) for _ in range(R)]
            steps = list(range(1, R + 1))

            def hoisted():
                return eng.ckks_rotate_hoisted_hks(mext, k, alpha, ct, keys, steps)

            def single_calls():
                return [eng.ckks_rotate_hks(mext, k, alpha, ct, keys[r], steps[r]) for r in range(R)]

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

            t_single, t_hoisted = median_ms(single_calls), median_ms(hoisted)
            print(f"\nN=2^{logn} L={L} k={k} alpha={alpha} batch 1, {R} rotations: {R} calls {t_single:.3f} ms, hoisted {t_hoisted:.3f} ms, "
                  f"ratio {t_hoisted / t_single:.3f}")
            for name, f in (("single calls", single_calls), ("hoisted", hoisted)):
                print(name, {fam: (cnt, round(ms, 3)) for fam, (cnt, ms) in families(f).items()})
            assert t_hoisted / t_single < 1.0, (t_hoisted, t_single)
    finally:
        eng.close()
