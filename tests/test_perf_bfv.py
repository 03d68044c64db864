"""Timing of the BFV lift (`pytest -m perf`, on an MI355X; not part of the correctness tiers: tests/conftest.py) at N = 8192, L = 4,
M = 6, batch 64:
  fused     hp_dev_bfv_lift: one Garner composition per coefficient, then its residue in every b_j (and the Q rows carried over);
  composed  hp_dev_intt (strict) + hp_dev_poly_reduce_strict + hp_dev_rns_base_many_to_many + hp_dev_ntt on preallocated buffers, the
            calls that were there before (unchanged): the whole composition again for each of the M target moduli.
The ratio fused / composed measured when the call was written is LIFT_MEASURED (profiles/bfv_measure.txt); the
assertion is 1.5 times that, the margin tests/test_perf_sample.py uses for the run-to-run spread of a shared machine.  Both sides run
in the same process, alternating, warmed, timed by device events on the engine's stream; medians of 7.  Reported, not asserted: the
time of one hp_dev_bfv_mult_relin_hks at the same shape (k = 2, alpha = 2) and the share of it spent in the scale kernel, with the
kernel families of every side (`-s`)."""
import statistics

import numpy as np
import pytest

import params as P
from hks_model import chain
from oracle.pyoracle import SplitMix

pytestmark = pytest.mark.perf

LIFT_MEASURED = 0.50   # fused / composed
LOGN, L, M, K, ALPHA, BATCH, T = 13, 4, 6, 2, 2, 64, 65537
Q, AUX = P.P40[:L], P.P40[L:L + M]


def test_fused_lift_against_the_composed_path():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from hehub_amd.engine import Engine, _u64arr

    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.use_stream(stream)
    n, qb, mext = 1 << LOGN, Q + AUX, chain(L, K)
    try:
        with torch.cuda.stream(stream):
            def once(f):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1)

            rng = SplitMix(9900)
            x = eng.to_device(rng.poly((BATCH, L, n), Q))
            ct1, ct2 = eng.to_device(rng.poly((BATCH, 2, L, n), Q)), eng.to_device(rng.poly((BATCH, 2, L, n), Q))
            key = eng.to_device(rng.poly(((L + ALPHA - 1) // ALPHA, 2, L + K, n), mext))
            up, lin = eng.empty((BATCH, L + M, n)), eng.empty((BATCH, 2, L, n))
            c, conv = eng.empty((BATCH, L, n)), eng.empty((BATCH, M, n))
            qarr, barr, lib, h, p = _u64arr(Q), _u64arr(AUX), eng.lib, eng.h, eng._ptr

            def fused():
                eng.bfv_lift(qb, L, x, out=up)

            def composed():   # (in place on c: after the first round its words are other strict rows, the work is the same)
                eng._chk(lib.hp_dev_intt(h, LOGN, L, qarr, BATCH, p(c), 1))
                eng._chk(lib.hp_dev_poly_reduce_strict(h, n, L, qarr, BATCH, p(c)))
                eng._chk(lib.hp_dev_rns_base_many_to_many(h, n, L, qarr, M, barr, BATCH, p(c), p(conv)))
                eng._chk(lib.hp_dev_ntt(h, LOGN, M, barr, BATCH, p(conv)))

            def mult():
                eng.bfv_mult_hks(mext, AUX, T, K, ALPHA, ct1, ct2, key, out=lin)

            # the same rows on both sides, once, before the timing
            c.copy_(x)
            fused()
            composed()
            eng.sync()
            assert np.array_equal(eng.to_host(up[-1, L:]), eng.to_host(conv[-1]) % np.array(AUX, dtype=np.uint64)[:, None])

            sides = (("composed", composed), ("fused", fused), ("mult_relin", mult))
            for _ in range(2):
                for _, f in sides:
                    f()
            times = {name: [] for name, _ in sides}
            for _ in range(7):
                for name, f in sides:
                    times[name].append(once(f))
            med = {name: statistics.median(t) for name, t in times.items()}
            ratio = med["fused"] / med["composed"]
            print(f"\nN=2^{LOGN} L={L} M={M} batch={BATCH}: " + ", ".join(f"{name} {med[name]:.3f} ms (min {min(t):.3f} max {max(t):.3f})"
                                                                         for name, t in times.items()))
            print(f"fused / composed = {ratio:.3f} (recorded {LIFT_MEASURED})")
            for name, f in sides:
                eng.prof_begin("*")
                f()
                fams = eng.prof_end_families()
                print(name, {fam: (cnt, round(ms, 3)) for fam, (cnt, ms) in fams.items()})
                if name == "mult_relin":
                    total = sum(ms for _, ms in fams.values())
                    print(f"mult_relin: scale kernel {fams['bfv_scale'][1]:.3f} ms of {total:.3f} ms in kernels = {fams['bfv_scale'][1] / total:.1%}; "
                          f"both conversions (bfv_scale + bfv_lift) {(fams['bfv_scale'][1] + fams['bfv_lift'][1]) / total:.1%}")
            assert ratio <= 1.5 * LIFT_MEASURED, (med, LIFT_MEASURED)
    finally:
        eng.close()
