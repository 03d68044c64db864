"""Timing of the ciphertext linear-combination kernel against the calls it replaces (`pytest -m perf`, on an MI355X; not part of the
correctness tiers: tests/conftest.py).  sum_j c_j ct_j over 8 terms at N = 32768, L = 8, batch 16 (67 MB per operand):
  * the baseline is the same sum from hp_dev_poly_scalar_mul and hp_dev_poly_add, term after term -- calls this kernel does not touch;
  * per output word the kernel moves 8 (terms + 1) = 72 bytes against 16 per scalar multiplication + 24 per addition = 296: a ratio
    of 4.1 by traffic.  Required: at least 2x, half the traffic ratio (nobody had measured the kernel when the figure was set).
Both sides are warmed, timed in alternating windows of 100 calls between device events (10 ms and 40 ms), and compared on the median of 7 windows; the
two outputs must be the same residues.  The measured times, the ratio and the kernel's rate on 8 (terms + 1) bytes per word are printed
(`-s`) and recorded in profiles/lincomb_measure.txt and DESIGN.md 4.7j."""
import statistics

import pytest

import params as P

pytestmark = pytest.mark.perf


def test_lincomb_beats_the_chain_of_single_calls():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from hehub_amd.engine import Engine

    logn, L, B, T = 15, 8, 16, 8
    n, q = 1 << logn, P.P40[:L]
    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.use_stream(stream)
    try:
        with torch.cuda.stream(stream):
            gen = torch.Generator(device="cuda").manual_seed(29)
            cts = [torch.randint(0, 1 << 40, (B, 2, L, n), dtype=torch.int64, device="cuda", generator=gen) for _ in range(T)]   # words below q
            coefs = [[(0x9E3779B97F4A7C15 * (j * L + m + 1)) % q[m] for m in range(L)] for j in range(T)]
            out, acc, tmp = eng.empty((B, 2, L, n)), eng.empty((2 * B, L, n)), eng.empty((2 * B, L, n))
            rows = lambda t: t.view(2 * B, L, n)

            def lincomb():
                return eng.ckks_lincomb(q, cts, coefs, out=out)

            def chain():
                eng.poly_scalar_mul(q, rows(cts[0]), coefs[0], out=acc)
                for j in range(1, T):
                    eng.poly_scalar_mul(q, rows(cts[j]), coefs[j], out=tmp)
                    eng.poly_add(q, acc, tmp, out=acc)
                return acc

            def window_ms(f, calls=100):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(calls):
                    f()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1) / calls

            for f in (lincomb, chain, lincomb, chain):     # warmed: workspace, tables, allocator, code objects
                f()
            stream.synchronize()
            same = torch.equal(out.view(2 * B, L, n), eng.poly_reduce_strict_(q, chain().clone()))
            t_lin, t_chain = [], []
            for _ in range(7):                             # alternating windows: a neighbour's load hits both sides
                t_lin.append(window_ms(lincomb))
                t_chain.append(window_ms(chain))
            m_lin, m_chain = statistics.median(t_lin), statistics.median(t_chain)
            words = 2 * B * L * n
            print(f"\nN=2^{logn} L={L} batch {B}, {T} terms: scalar_mul + add chain {m_chain:.3f} ms (min {min(t_chain):.3f}, max {max(t_chain):.3f}), "
                  f"lincomb {m_lin:.3f} ms (min {min(t_lin):.3f}, max {max(t_lin):.3f}), ratio {m_chain / m_lin:.2f}x, "
                  f"{8 * (T + 1) * words / 1e9 / (m_lin * 1e-3):.0f} GB/s on 8 (terms + 1) bytes per word, the chain "
                  f"{(16 * T + 24 * (T - 1)) * words / 1e9 / (m_chain * 1e-3):.0f} GB/s on its 16 T + 24 (T - 1)")
            assert same
            assert m_chain / m_lin >= 2.0, (m_chain, m_lin)
    finally:
        eng.close()
