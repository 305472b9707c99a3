"""Times vt_sample_rows_wm (the SynthID text watermark inside the per-row sampler) against vt_sample_rows_trunc on the
same decode-sized logits: 16 rows, V = 32000, fp32, temperature 1, every row sampled.

Arms, each at top_k = 0 (the whole row survives: every token is hashed in every round) and top_k = 50 (a handful of threads own a
survivor): "trunc" (vt_sample_rows_trunc with all-inactive rows: what a call without a watermark launches), "wm cells NULL" (the wm
kernel, every row without a cell: the tournament never runs), and "wm depth 9" / "wm depth 30" (ngram_len 5, a 65536-entry table, a
history of 1024) with the cells alternating fresh (even rows: the tournament runs) and repeated (odd rows: the context's hash already
stands in the history ring, so the row is drawn plainly). The cells are restored from a snapshot in front of every launch, outside the
timed span, so every launch of an arm does the same work.

Two figures per arm and round: "device_us", the mean span between two device events placed around ONE launch -- for a wm arm that span
holds the read-back of the vt_wm_row array the entry point validates on the host (rows * 48 bytes) and the kernel; and "host_us", the
host clock over all the launches of the round divided by their number, a device synchronise at the end -- for a wm arm every launch waits
for its read-back, so this is what a decode loop pays per step on the host. The arms are alternated inside one process over `--rounds`
rounds; per arm the output gives every round, the median and the spread (max - min) / median. No threshold is set: the run records what
is found (profiles/wm_bench.json).

  python tools/wm_bench.py [--rows 16] [--iters 200] [--rounds 3] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vitron_amd import _lib, ops  # noqa: E402
from vitron_amd.sampling import pack_sample_rows, pack_trunc_rows  # noqa: E402
from vitron_amd.watermark import SynthIDWatermark, pack_wm_rows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=16)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()

_lib.load()
dev = torch.device("cuda:0")
V, SEED, ROWS = 32000, 1, args.rows
KEYS = [654, 400, 836, 123, 340, 443, 597, 160, 57, 29, 590, 639, 13, 715, 468, 990, 966, 226, 324, 585, 118, 504, 421, 521, 129, 669, 732,
        225, 90, 960]
lg = torch.randn((ROWS, V), device=dev) * 3
trunc_off = pack_trunc_rows([None] * ROWS, dev)


def params(top_k):
    return pack_sample_rows([(1.0, top_k, 1.0, 1.0, SEED, 2, r, 0, 0) for r in range(ROWS)], dev)


def wm_arm(depth, pr):
    wm = SynthIDWatermark(dict(ngram_len=5, keys=KEYS[:depth]))
    cells = torch.zeros((ROWS, wm.cell_words), dtype=torch.int64, device=dev)
    snap = np.zeros((ROWS, wm.cell_words), dtype=np.uint64)
    snap[1::2, 12] = wm.context_hash(np.zeros((4,), np.int64))          # odd rows: the fresh context's hash is in the ring already
    snap = torch.from_numpy(snap.view(np.int64)).to(dev)
    rows = pack_wm_rows([(wm, cells[r]) for r in range(ROWS)], dev)

    def restore():
        cells.copy_(snap)

    def check():          # the arm does what it says: even rows watermarked (flag 1), odd rows repeated (flag 2)
        restore()
        ops.sample_rows(lg, pr, trunc=trunc_off, watermark=rows)
        flags = cells[:, 3].cpu().tolist()
        assert flags == [1, 2] * (ROWS // 2) + [1] * (ROWS % 2), flags
    check()
    return (lambda: ops.sample_rows(lg, pr, trunc=trunc_off, watermark=rows)), restore


def measure(fn, restore):
    for _ in range(3):
        restore()
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
    t0 = time.perf_counter()
    for a, b in pairs:
        restore()
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) / args.iters * 1e6
    return sum(a.elapsed_time(b) for a, b in pairs) / args.iters * 1e3, host


arms = {}
null_rows = pack_wm_rows([None] * ROWS, dev)
nothing = lambda: None          # noqa: E731
for top_k in (0, 50):
    pr = params(top_k)
    arms[f"trunc top_k={top_k}"] = ((lambda pr=pr: ops.sample_rows(lg, pr, trunc=trunc_off)), nothing)
    arms[f"wm cells NULL top_k={top_k}"] = ((lambda pr=pr: ops.sample_rows(lg, pr, trunc=trunc_off, watermark=null_rows)), nothing)
    for depth in (9, 30):
        arms[f"wm depth {depth} top_k={top_k}"] = wm_arm(depth, pr)

result = {"V": V, "rows": ROWS, "iters": args.iters, "rounds": args.rounds, "ngram_len": 5, "table_size": 65536, "history_size": 1024,
          "cells": "even rows fresh, odd rows repeated", "device": torch.cuda.get_device_name(0), "arms": {}}
samples = {name: {"device_us": [], "host_us": []} for name in arms}
for _ in range(args.rounds):
    for name, (fn, restore) in arms.items():
        d, h = measure(fn, restore)
        samples[name]["device_us"].append(d)
        samples[name]["host_us"].append(h)
for name, s in samples.items():
    out = {}
    for what, vals in s.items():
        med = statistics.median(vals)
        out[what] = {"rounds": [round(v, 2) for v in vals], "median": round(med, 2), "spread": round((max(vals) - min(vals)) / med, 3)}
    result["arms"][name] = out
    print(f"{name:28s} device {out['device_us']['median']:8.2f} us (spread {out['device_us']['spread']:.3f})   "
          f"host {out['host_us']['median']:8.2f} us (spread {out['host_us']['spread']:.3f})")
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
