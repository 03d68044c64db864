"""Timing of seeded secret-key encryption (`pytest -m perf`, on an MI355X; not part of the correctness tiers: tests/conftest.py) at
N = 32768, L = 10, batch 64 -- 168 MB of c0 rows, 336 MB of full ciphertexts:
  fused     hp_dev_rlwe_encrypt_seeded, full (with_c1 = 1) and compressed (with_c1 = 0);
  composed  hp_dev_sample_uniform + hp_dev_sample_cbd + hp_dev_rlwe_encrypt_core on preallocated buffers, the three calls that were there
            before (unchanged): a goes to memory, is read back and copied into the ciphertext, the error through an int64 row.
The ratios fused / composed measured when the calls were written are FULL_MEASURED and COMPRESSED_MEASURED (profiles/enc_seeded_measure.txt,
DESIGN.md 4.7h); the assertions are 1.5 times those, the margin tests/test_perf_sample.py uses for the run-to-run spread of a shared
machine.  All sides run in the same process, alternating, warmed, timed by device events on the engine's stream; medians of 7.  The
kernel families of each side are printed (`-s`)."""
import statistics

import pytest

import params as P
import sample_cases as K
import sample_model as S

pytestmark = pytest.mark.perf

FULL_MEASURED = 0.95          # fused full / composed
COMPRESSED_MEASURED = 0.88    # fused compressed / composed
LOGN, MODULI, BATCH = P.C3_LOGN, P.C3_Q, 64


def test_fused_encryption_against_the_three_existing_calls():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from hehub_amd.engine import Engine, _u64arr

    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.use_stream(stream)
    L, n = len(MODULI), 1 << LOGN
    try:
        with torch.cuda.stream(stream):
            def once(f):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1)

            sk = eng.sample_small_ntt(LOGN, MODULI, S.TERNARY, K.SEED2, 1)[0]
            pt = eng.sample_uniform(LOGN, MODULI, K.SEED2, 2, BATCH)
            ct, c0 = eng.empty((BATCH, 2, L, n)), eng.empty((BATCH, L, n))
            a, e, ref = eng.empty((BATCH, L, n)), eng.empty((BATCH, n)), eng.empty((BATCH, 2, L, n))
            marr, seed, lib, h, p = _u64arr(MODULI), eng._seed(K.SEED), eng.lib, eng.h, eng._ptr

            def full():
                eng.rlwe_encrypt_seeded(MODULI, sk, pt, K.SEED, 1, out=ct)

            def compressed():
                eng.rlwe_encrypt_seeded(MODULI, sk, pt, K.SEED, 1, with_c1=False, out=c0)

            def composed():
                eng._chk(lib.hp_dev_sample_uniform(h, LOGN, L, marr, None, BATCH, seed, 1, 0, p(a)))
                eng._chk(lib.hp_dev_sample_cbd(h, LOGN, BATCH, seed, 1, p(e)))
                eng._chk(lib.hp_dev_rlwe_encrypt_core(h, LOGN, L, marr, BATCH, p(e), p(a), p(pt), p(sk), p(ref)))

            sides = (("composed", composed), ("full", full), ("compressed", compressed))
            for _ in range(2):
                for _, f in sides:
                    f()
            times = {name: [] for name, _ in sides}
            for _ in range(7):
                for name, f in sides:
                    times[name].append(once(f))
            med = {name: statistics.median(t) for name, t in times.items()}
            r_full, r_comp = med["full"] / med["composed"], med["compressed"] / med["composed"]
            print(f"\nN=2^{LOGN} L={L} batch={BATCH}: " + ", ".join(f"{name} {med[name]:.3f} ms (min {min(t):.3f} max {max(t):.3f})"
                                                                    for name, t in times.items()))
            print(f"full / composed = {r_full:.3f} (recorded {FULL_MEASURED}), compressed / composed = {r_comp:.3f} (recorded {COMPRESSED_MEASURED})")
            for name, f in sides:
                eng.prof_begin("*")
                f()
                print(name, {fam: (cnt, round(ms, 3)) for fam, (cnt, ms) in eng.prof_end_families().items()})
            # the same ciphertext on both sides (canonical against hehub's lazy words: compared modulo q on one row)
            eng.sync()
            q = MODULI[-1]
            assert bool(((ref[-1, 0, -1] % q) == ct[-1, 0, -1]).all()) and bool((ref[-1, 1] == ct[-1, 1]).all()) and bool((c0 == ct[:, 0]).all())
            assert r_full <= 1.5 * FULL_MEASURED, (med, FULL_MEASURED)
            assert r_comp <= 1.5 * COMPRESSED_MEASURED, (med, COMPRESSED_MEASURED)
    finally:
        eng.close()
