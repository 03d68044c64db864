"""Per-kernel-family timing of hybrid key generation on the device (hp_prof_begin / end): one hks_keygen_rot call -- and, beside
it, one hks_keygen call -- of 32 keys at N = 32768, L = 10, k = 4, alpha = 3, with the fused kernel's achieved bytes per second.
    python tools/bench_hks_keygen.py [OUTPUT.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import params as P
from hehub_amd.engine import Engine

STEPS = 5
eng = Engine(0)
logn, L, k, alpha, R = P.C3_LOGN, len(P.C3_Q), 4, 3, 32
mext = P.C3_Q + P.ntt_primes(k, logn, 50, exclude=P.C3_Q)
n, nd, E = 1 << logn, (L + alpha - 1) // alpha, L + k
assert (n, L, nd, E) == (32768, 10, 4, 14)
dev = f"cuda:{eng.device}"
steps = list(range(16)) + [16 * g for g in range(16)]          # 16 baby and 16 giant steps of a 16 x 16 diagonal transform
s = eng.poly_from_signed(mext, torch.randint(-1, 2, (1, n), dtype=torch.int64, device=dev))
a = torch.randint(0, 1 << 39, (R, nd, E, n), dtype=torch.int64, device=dev)
e = torch.randint(-8, 9, (R, nd, n), dtype=torch.int64, device=dev)
s_from = torch.randint(0, 1 << 39, (R, E, n), dtype=torch.int64, device=dev)
out = eng.empty((R, nd, 2, E, n))

fused_bytes = 8 * n * (R * nd * E          # NTT(e), read from the key rows
                       + R * nd * E        # a
                       + R * L             # the source secret, on the limbs of its digit
                       + 2 * R * nd * E    # the two key rows
                       + E)                # s_to, once
lines = [f"shape: N={n} L={L} k={k} alpha={alpha} dnum={nd} keys={R}: {R * nd * E} transforms, "
         f"{8 * n * 3 * R * nd * E / 1e9:.2f} GB of a and key rows, fused kernel {fused_bytes / 1e9:.3f} GB per call; {STEPS} calls per figure"]
for name, call in (("hks_keygen_rot", lambda: eng.hks_keygen_rot(mext, k, alpha, s[0], steps, a, e, out=out)),
                   ("hks_keygen", lambda: eng.hks_keygen(mext, k, alpha, s[0], s_from, a, e, out=out))):
    call()
    eng.sync()
    eng.prof_begin("*")
    for _ in range(STEPS):
        call()
    fam = eng.prof_end_families()
    total = 0.0
    for f, (launches, ms) in fam.items():
        total += ms / STEPS
        line = f"{name:15s} {f:14s} {launches / STEPS:5.1f} launches  {ms / STEPS:8.3f} ms per call"
        if f == "hks_keygen":
            line += f"  {fused_bytes / (ms / STEPS * 1e-3) / 1e9:8.1f} GB/s"
        lines.append(line)
    lines.append(f"{name:15s} sum {total:.3f} ms per call")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
print("\n".join(lines))
eng.close()
