"""Timing of the fused ModRaise against the three calls it replaces (`pytest -m perf`, on an MI355X; not part of the correctness
tiers: tests/conftest.py).  N = 32768, L = 14, batch 32 -- a ciphertext batch at its last limb raised to a bootstrapping chain:
  * the baseline is hp_dev_intt (strict) on the 64 rows, hp_dev_rns_base_from_single into the 14-limb block, hp_dev_ntt on the block;
  * rows of 8 N bytes moved per polynomial: 2 + (1 + L) + 2 L = 3 L + 3 = 45 for the three calls; 2 + (1 + (L - 1)) + 2 = L + 4 = 18
    for hp_dev_ckks_mod_raise (inverse transform; one read of the coefficient row per group of moduli, L - 1 rows written; the
    canonical copy of row 0), a ratio of 2.5 by traffic.  Nobody had measured the call when this test was written: required is only
    that it is not slower.
Both sides are warmed, timed in alternating windows of 20 calls between device events and compared on the median of 7 windows; the two
outputs must be the same residues.  The measured times and the rates on the modelled bytes are printed (`-s`) and recorded in
DESIGN.md 4.7k."""
import statistics

import pytest

import params as P

pytestmark = pytest.mark.perf


def test_fused_mod_raise_is_not_slower_than_the_three_calls():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from hehub_amd import capi
    from hehub_amd.engine import Engine

    logn, L, B = 15, 14, 32
    n = 1 << logn
    q = [P.P50[1]] + P.ntt_primes(L - 1, logn, 40)
    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.use_stream(stream)
    try:
        with torch.cuda.stream(stream):
            gen = torch.Generator(device="cuda").manual_seed(31)
            ct = torch.randint(0, q[0], (B, 2, 1, n), dtype=torch.int64, device="cuda", generator=gen)   # strict words of q_0
            out, lifted, x = eng.empty((B, 2, L, n)), eng.empty((2 * B, L, n)), eng.empty((2 * B, 1, n))
            mods = (capi.u64 * L)(*q)

            def fused():
                return eng.ckks_mod_raise(q, ct, out=out)

            def three_calls():
                eng.intt_(q[:1], x, strict=True)      # in place: the words change from call to call, the work does not
                eng._chk(eng.lib.hp_dev_rns_base_from_single(eng.h, n, q[0], L, mods, 2 * B, eng._ptr(x), eng._ptr(lifted)))
                return eng.ntt_(q, lifted)

            def window_ms(f, calls=20):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(calls):
                    f()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1) / calls

            x.copy_(ct.view(2 * B, 1, n))
            qv = torch.tensor(q, dtype=torch.int64, device="cuda")[:, None]
            same = torch.equal(fused().view(2 * B, L, n) % qv, three_calls() % qv)
            for f in (fused, three_calls, fused, three_calls):     # warmed: workspace, tables, allocator, code objects
                f()
            stream.synchronize()
            t_f, t_c = [], []
            for _ in range(7):                                     # alternating windows: a neighbour's load hits both sides
                t_f.append(window_ms(fused))
                t_c.append(window_ms(three_calls))
            m_f, m_c = statistics.median(t_f), statistics.median(t_c)
            row = 8 * n * 2 * B
            print(f"\nN=2^{logn} L={L} batch {B}: three calls {m_c:.3f} ms (min {min(t_c):.3f}, max {max(t_c):.3f}), "
                  f"mod_raise {m_f:.3f} ms (min {min(t_f):.3f}, max {max(t_f):.3f}), ratio {m_c / m_f:.2f}x; "
                  f"{(3 * L + 3) * row / 1e6:.0f} MB at {(3 * L + 3) * row / 1e9 / (m_c * 1e-3):.0f} GB/s against "
                  f"{(L + 4) * row / 1e6:.0f} MB at {(L + 4) * row / 1e9 / (m_f * 1e-3):.0f} GB/s")
            assert same
            assert m_f <= m_c, (m_f, m_c)
    finally:
        eng.close()
