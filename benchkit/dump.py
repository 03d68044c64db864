"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, as .npy files, so that two builds can be compared output
for output on the same seeded inputs.

Every output is a tensor of u64 words (int64 storage) whose first axis is the batch.  The words stay below 2^53 (moduli of at most 50
bits, lazy words below 4q), so float64 holds each one exactly; a word at or above 2^53 is an error, never a rounded dump.  An output larger
than its share of the byte budget is sampled: whole batch items chosen by a fixed seed, or, when one item alone is too large, a fixed
seeded set of flat positions.  `manifest.json` in DIR says which items / positions each file holds."""
from __future__ import annotations

import json
import os

BUDGET_BYTES = 48 << 20     # all .npy payloads of one run together (the limit is 64 MB)
SEED = 20261016


def _sample(torch, t, budget):
    """(float64 numpy array, manifest entry) of device tensor `t` within `budget` bytes"""
    import numpy as np

    ent = {"shape": list(t.shape), "words": "u64 residues as float64 (exact: every word < 2^53)"}
    per_item = t[0].numel() * 8 if t.dim() and t.shape[0] else 0
    if t.numel() * 8 <= budget:
        part, ent["sample"] = t, "all"
    elif 0 < per_item <= budget:
        k = budget // per_item
        idx = np.sort(np.random.default_rng(SEED).choice(t.shape[0], size=k, replace=False))
        part = t.index_select(0, torch.from_numpy(idx).to(t.device))
        ent["sample"], ent["items"] = "batch items", idx.tolist()
    else:
        k = budget // 8
        pos = np.sort(np.random.default_rng(SEED).choice(t.numel(), size=k, replace=False))
        part = t.reshape(-1).index_select(0, torch.from_numpy(pos).to(t.device))
        ent["sample"], ent["flat_positions_seed"], ent["count"] = "flat positions", SEED, int(k)
    if bool(((part < 0) | (part >= (1 << 53))).any()):
        raise ValueError(f"output of shape {tuple(t.shape)} holds a word outside [0, 2^53): float64 would not hold it exactly")
    return part.to(torch.float64).cpu().numpy(), ent


def dump_outputs(run, wl, outdir, budget=BUDGET_BYTES):
    """write wl.outputs() of this rank to outdir/<name>.npy (rank suffix when world > 1) plus outdir/manifest.json; returns the file names"""
    import numpy as np

    torch = run.torch
    os.makedirs(outdir, exist_ok=True)
    outs = wl.outputs()
    share = budget // (max(1, len(outs)) * max(1, run.world))
    manifest, names = {}, []
    for name, t in outs.items():
        arr, ent = _sample(torch, t, share)
        fname = name if run.world == 1 else f"{name}_rank{run.rank}"
        np.save(os.path.join(outdir, fname + ".npy"), arr)
        manifest[fname] = ent
        names.append(fname + ".npy")
    mpath = os.path.join(outdir, "manifest.json" if run.world == 1 else f"manifest_rank{run.rank}.json")
    with open(mpath, "w") as f:
        json.dump({"workload": wl.cfg.get("workload"), "steps_plus_warmup": run.args.steps + run.args.warmup, "outputs": manifest}, f, indent=1)
        f.write("\n")
    return names
