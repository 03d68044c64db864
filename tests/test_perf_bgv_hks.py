"""Timing of the BGV multiplication over the hybrid key switch against the composite of calls that existed before it (`pytest -m perf`,
on an MI355X; not part of the correctness tiers: tests/conftest.py).  Shape: BASELINE config 5 with a hybrid key -- N = 8192, L = 6,
k = 2, alpha = 2, t = 65537 -- at batch 512 and at batch 1.
  * one hp_dev_bgv_mult_relin_modswitch_hks, against hp_dev_mult_low_level, hp_dev_hks_switch on d2, two hp_dev_poly_add and
    hp_dev_bgv_mod_switch.  (The composite's switch runs the CKKS ModDown: the same kernels and traffic but for the two extra
    multiplications of k_hks_moddown_t; its result does not decrypt, which is why the call exists.)
  * both sides in the same run, alternating, warmed, device events on the engine's stream.  The ONE assertion: the fused call is not
    slower than the composite, within twice the run-to-run spread (max - min over the repetitions) measured on the composite side in
    that run.  No percentage is fixed in advance.  The composite needs two layout copies between its calls (d2 alone, (d0, d1) alone:
    mult_low_level writes [B][3][L][N]); they are timed on their own and taken OFF the composite's time before the comparison.
  * the per-family times of both sides, the two ModDown conversions (hks_moddown, hks_moddown_t) among them, are printed (`-s`) and
    recorded in DESIGN.md 4.7f.  No ratio against hehub's single-prime BGV path is asserted: its figure is printed only."""
import statistics

import pytest

import params as P

pytestmark = pytest.mark.perf


@pytest.mark.parametrize("B", [512, 1])
def test_fused_bgv_mult_is_not_slower_than_the_composite(B):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from hehub_amd.engine import Engine

    logn, L, k, alpha, t = P.C5_LOGN, 6, 2, 2, P.C5_T
    n, nd = 1 << logn, (L + alpha - 1) // alpha
    mext = P.P40[:L] + P.P50[:k]
    q = mext[:L]
    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.use_stream(stream)
    try:
        with torch.cuda.stream(stream):
            gen = torch.Generator(device="cuda").manual_seed(29)
            rand = lambda *shape: torch.randint(0, 1 << 40, shape, dtype=torch.int64, device="cuda", generator=gen)   # words below q
            a, b = rand(B, 2, L, n), rand(B, 2, L, n)
            key = rand(nd, 2, L + k, n)
            key1 = rand(L, 2, L + 1, n)   # hehub's single-prime key shape, for the figure that is only printed
            out_fused = eng.empty((B, 2, L - 1, n))
            lin = eng.empty((B, 2, L, n))

            def fused():
                return eng.bgv_mult_hks(mext, t, k, alpha, a, b, key, out=out_fused)

            quad0 = eng.mult_low_level(q, a, b)
            rows = lambda x: x.view(2 * B, L, n)

            def glue(quad=quad0):
                """the layout copies the composite needs between its calls: d2 alone for the switch, (d0, d1) without d2 for the adds"""
                return quad[:, 2].contiguous(), quad[:, :2].contiguous()

            def composite():
                d2, d01 = glue(eng.mult_low_level(q, a, b))
                sw = eng.hks_switch(mext, k, alpha, d2, key)
                eng.poly_add(q, rows(sw)[:B], rows(d01)[:B], out=rows(lin)[:B])   # two adds of B polynomials each
                eng.poly_add(q, rows(sw)[B:], rows(d01)[B:], out=rows(lin)[B:])
                return eng.bgv_mod_switch(q, t, lin)

            def single_prime():
                return eng.bgv_mult(q + [P.P50[0]], t, a, b, key1, inner_t=True)

            def once(f):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1)

            for f in (fused, composite, fused, composite):   # warmed: workspace, tables, allocator
                f()
            t_fused, t_comp = [], []
            for _ in range(7):                               # alternating
                t_fused.append(once(fused))
                t_comp.append(once(composite))
            m_fused, m_comp = statistics.median(t_fused), statistics.median(t_comp)
            spread = max(t_comp) - min(t_comp)
            m_glue = statistics.median([once(glue) for _ in range(7)])
            print(f"\nN=2^{logn} L={L} k={k} alpha={alpha} t={t} batch {B}: bgv_mult_hks {m_fused:.3f} ms, composite {m_comp:.3f} ms "
                  f"(spread {spread:.3f} ms; {m_glue:.3f} ms of it layout copies), ratio {m_fused / m_comp:.3f}, "
                  f"without the copies {m_fused / (m_comp - m_glue):.3f}")
            for name, f in (("bgv_mult_hks", fused), ("composite", composite)):
                eng.prof_begin("*")
                f()
                print(name, {fam: (cnt, round(ms, 3)) for fam, (cnt, ms) in eng.prof_end_families().items()})
            single_prime()
            print(f"hehub-keyed single-prime bgv mult (the _t extension), same run: {statistics.median([once(single_prime) for _ in range(5)]):.3f} ms")
            # the composite's layout copies are not held against it: the fused call must match its four calls alone
            assert m_fused <= (m_comp - m_glue) + 2 * spread, (m_fused, m_comp, m_glue, spread)
    finally:
        eng.close()
