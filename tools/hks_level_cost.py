#!/usr/bin/env python3
"""What reading a top-level hybrid key in place costs at a lower level: hp_dev_ckks_mult_relin_rescale_hks on the
compact level key against hp_dev_ckks_mult_relin_rescale_hks_at on the top key -- the same bytes, strided key rows.

    python tools/hks_level_cost.py [--batch 32] [--iters 30] [--repeats 5]

C3 shape at the top (N = 32768, key_L0 = 10, k = 4, alpha = 3), every level L = 10 .. 2; random words (timing does not depend on them).
Host clock around `iters` calls that end in a synchronise, warmed, the two forms alternating, median of `repeats`.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch

    import params as P
    from benchkit.inputs import rand_words
    from hehub_amd.engine import Engine

    logn, key_L0, k, alpha = P.C3_LOGN, len(P.C3_Q), 4, 3
    n = 1 << logn
    mtop = P.C3_Q + P.ntt_primes(k, logn, 50, exclude=P.C3_Q)
    eng = Engine(0)
    dev = f"cuda:{eng.device}"
    rows = []
    try:
        top = rand_words(torch, ((key_L0 + alpha - 1) // alpha, 2, key_L0 + k, n), mtop, dev, 7)
        for L in range(key_L0, 1, -1):
            mext = mtop[:L] + mtop[key_L0:]
            keep = list(range(L)) + list(range(key_L0, key_L0 + k))
            sub = top[:(L + alpha - 1) // alpha][:, :, keep].contiguous()
            ct1 = rand_words(torch, (args.batch, 2, L, n), mext[:L], dev, 3)
            ct2 = rand_words(torch, (args.batch, 2, L, n), mext[:L], dev, 1003)
            out = eng.empty((args.batch, 2, L - 1, n))
            forms = {"plain": lambda: eng.ckks_mult_hks(mext, k, alpha, ct1, ct2, sub, out=out),
                     "at": lambda: eng.ckks_mult_hks(mext, k, alpha, ct1, ct2, top, out=out, key_L0=key_L0)}
            ms = {name: [] for name in forms}
            for f in forms.values():
                for _ in range(5):
                    f()
            eng.sync()
            for _ in range(args.repeats):
                for name, f in forms.items():
                    eng.sync()
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        f()
                    eng.sync()
                    ms[name].append(1e3 * (time.perf_counter() - t0) / args.iters)
            plain, at = statistics.median(ms["plain"]), statistics.median(ms["at"])
            rows.append({"L": L, "plain_ms": round(plain, 4), "at_ms": round(at, 4), "at_over_plain": round(at / plain, 4),
                         "plain_spread": round(max(ms["plain"]) / min(ms["plain"]), 4)})
    finally:
        eng.close()
    print(json.dumps({"what": "ckks_mult_hks per call, compact level key (plain) against the top key read in place (at)", "N": n,
                      "key_L0": key_L0, "k": k, "alpha": alpha, "batch": args.batch, "iters": args.iters, "repeats": args.repeats,
                      "levels": rows}))


if __name__ == "__main__":
    main()
