"""Timing of the device samplers (`pytest -m perf`, on an MI355X; not part of the correctness tiers: tests/conftest.py), at the shape
include/hehub_amd.h quotes for a BSGS key set: N = 32768, L = 10, k = 4, alpha = 3 (14 moduli, dnum = 4), 32 keys -- 470 MB of uniform
rows, half of the 940 MB key set.
  1. A CONDITION: sampling the set's uniform rows on the device takes at most half the time of hp_memcpy_h2d_async of the same bytes
     from registered host memory.  Below that the feature has no point.
  2. The seeded generator against hp_dev_hks_keygen on resident rows (that call is the parent commit's, unchanged; it reads its a rows
     from a second buffer, the seeded call samples them into the keys): the ratio measured when the samplers were written is
     RATIO_MEASURED (profiles/sample_measure.txt), and the assertion is 1.5 times that -- the run-to-run spread of this
     machine is 3-12 % (NOTES.md, "Sharp edges").
Both sides of a comparison run in the same process, alternating, warmed, timed by device events on the engine's stream; medians of 7.
The sampler's GB/s and its fraction of the 2.3 TB/s VALU estimate (1000 VALU operations per 64 bytes, 1024 SIMDs at 2.27 GHz) are
printed (`-s`)."""
import ctypes as C
import statistics

import pytest

import params as P
import sample_cases as K

pytestmark = pytest.mark.perf

RATIO_MEASURED = 1.36
VALU_ESTIMATE_GBS = 2300.0
LOGN, L, KP, ALPHA, KEYS = P.C3_LOGN, len(P.C3_Q), 4, 3, 32


def setup():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from hehub_amd.engine import Engine

    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.use_stream(stream)
    mext = P.C3_Q + P.ntt_primes(KP, LOGN, 50, exclude=P.C3_Q)
    return torch, eng, stream, mext


def timer(torch, stream):
    def once(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        f()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)
    return once


def test_sampling_a_key_set_beats_copying_it_from_the_host():
    from hehub_amd import capi

    torch, eng, stream, mext = setup()
    n, E, nd = 1 << LOGN, L + KP, (L + ALPHA - 1) // ALPHA
    rows = KEYS * nd
    nbytes = rows * E * n * 8
    host = capi.P()
    try:
        with torch.cuda.stream(stream):
            once = timer(torch, stream)
            dst = eng.empty((rows, E, n))
            eng._chk(eng.lib.hp_host_alloc(eng.h, nbytes, C.byref(host)))
            C.memset(host, 0x3C, nbytes)

            def copy():
                eng._chk(eng.lib.hp_memcpy_h2d_async(eng.h, eng._ptr(dst), host, nbytes))

            def sample():
                eng.sample_uniform(LOGN, mext, K.SEED, 1, rows, out=dst, stride_words=E * n)

            for f in (copy, sample, copy, sample):
                f()
            t_copy, t_sample = [], []
            for _ in range(7):
                t_copy.append(once(copy))
                t_sample.append(once(sample))
            m_copy, m_sample = statistics.median(t_copy), statistics.median(t_sample)
            gbs = nbytes / (m_sample * 1e-3) / 1e9
            print(f"\nN=2^{LOGN} E={E} rows={rows}: {nbytes / 1e6:.1f} MB of uniform rows; sampled in {m_sample:.3f} ms ({gbs:.0f} GB/s, "
                  f"{100 * gbs / VALU_ESTIMATE_GBS:.0f} % of the {VALU_ESTIMATE_GBS:.0f} GB/s VALU estimate; min {min(t_sample):.3f} max {max(t_sample):.3f}), "
                  f"copied from page-locked host memory in {m_copy:.3f} ms ({nbytes / (m_copy * 1e-3) / 1e9:.1f} GB/s), "
                  f"copy / sample = {m_copy / m_sample:.1f}")
            assert 2 * m_sample <= m_copy, (m_sample, m_copy)
    finally:
        if host:
            eng.lib.hp_host_free(eng.h, host)
        eng.close()


def test_seeded_generator_against_the_plain_one_on_resident_rows():
    torch, eng, stream, mext = setup()
    n, E, nd = 1 << LOGN, L + KP, (L + ALPHA - 1) // ALPHA
    try:
        with torch.cuda.stream(stream):
            once = timer(torch, stream)
            s = eng.poly_from_signed(mext, eng.sample_ternary(LOGN, K.SEED2, 1, 1))
            s_from = eng.sample_uniform(LOGN, mext, K.SEED2, 2, KEYS)
            a = eng.sample_uniform(LOGN, mext, K.SEED, 1, KEYS * nd).view(KEYS, nd, E, n)
            e = eng.sample_cbd(LOGN, K.SEED, 1, KEYS * nd).view(KEYS, nd, n)
            out = eng.empty((KEYS, nd, 2, E, n))

            def plain():
                eng.hks_keygen(mext, KP, ALPHA, s[0], s_from, a, e, out=out)

            def seeded():
                eng.hks_keygen_seeded(mext, KP, ALPHA, s[0], s_from, K.SEED, 1, 1, out=out)

            for f in (plain, seeded, plain, seeded):
                f()
            t_plain, t_seeded = [], []
            for _ in range(7):
                t_plain.append(once(plain))
                t_seeded.append(once(seeded))
            m_plain, m_seeded = statistics.median(t_plain), statistics.median(t_seeded)
            print(f"\nN=2^{LOGN} L={L} k={KP} alpha={ALPHA} keys={KEYS}: hks_keygen on resident rows {m_plain:.3f} ms (min {min(t_plain):.3f} max "
                  f"{max(t_plain):.3f}), hks_keygen_seeded {m_seeded:.3f} ms (min {min(t_seeded):.3f} max {max(t_seeded):.3f}), "
                  f"ratio {m_seeded / m_plain:.3f} (recorded {RATIO_MEASURED})")
            for name, f in (("hks_keygen", plain), ("hks_keygen_seeded", seeded)):
                eng.prof_begin("*")
                f()
                print(name, {fam: (cnt, round(ms, 3)) for fam, (cnt, ms) in eng.prof_end_families().items()})
            assert m_seeded / m_plain <= 1.5 * RATIO_MEASURED, (m_seeded, m_plain)
    finally:
        eng.close()
