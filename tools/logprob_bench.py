"""Times vt_logprob_rows on decode-sized logits ([4, 32000] and [16, 32000] fp32) and on the prompt-scoring case
([512, 32000]), with n_top 0, 5 and 20 and the picked ids as targets.

Beside it, in the same alternation:
  "ops n_top=N"        the same launch through ops.logprob_rows with its one output allocation (what generate's loop does NOT pay: it
                       writes into preallocated step buffers; ServingEngine._pick pays it);
  "host log_softmax"   what the launch replaces: the [rows, V] fp32 rows read back, torch.log_softmax + torch.topk(20) + a gather on the
                       CPU (timed over iters / 20 passes: it is three orders of magnitude slower);
  "read-back only"     the device -> host copy of the rows alone;
  "rows sampled +logprob"  one vt_sample_rows launch with its logprob output, for scale (decode shapes only).

The arms are alternated inside one process over `--rounds` rounds of `--iters` launches between two device events; per arm the output
gives every round, the median and the spread (max - min) / median. `--json FILE` writes the table (profiles/logprob_bench.json).

  python tools/logprob_bench.py [--rows 4,16,512] [--iters 200] [--rounds 3] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vitron_amd import _lib, ops  # noqa: E402
from vitron_amd.sampling import pack_sample_rows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="4,16,512")
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()

lib = _lib.load()
dev = torch.device("cuda:0")
V, T, P, SEED, STEP = 32000, 0.2, 0.7, 1, 2


def time_us(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


result = {"V": V, "iters": args.iters, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "shapes": {}}
for rows in [int(r) for r in args.rows.split(",")]:
    lg = torch.randn((rows, V), device=dev) * 3
    tg = ops.argmax(lg)
    stream = torch.cuda.current_stream().cuda_stream
    lp = torch.empty((rows,), dtype=torch.float32, device=dev)
    rk = torch.empty((rows,), dtype=torch.int32, device=dev)
    ti = torch.empty((rows, 20), dtype=torch.int32, device=dev)
    tl = torch.empty((rows, 20), dtype=torch.float32, device=dev)
    arms, iters = {}, {}
    for n in (0, 5, 20):
        arms[f"kernel n_top={n}"] = lambda n=n: lib.vt_logprob_rows(lg.data_ptr(), rows, V, V, tg.data_ptr(), n, None, lp.data_ptr(), rk.data_ptr(),
                                                                   ti.data_ptr() if n else None, tl.data_ptr() if n else None, stream)
        arms[f"ops n_top={n}"] = lambda n=n: ops.logprob_rows(lg, tg, n, return_rank=True)

    def host():
        x = lg.cpu()
        ls = torch.log_softmax(x, -1)
        return ls.gather(1, tg.cpu().long().unsqueeze(1)), torch.topk(ls, 20, dim=-1)
    arms["host log_softmax + topk(20)"] = host
    arms["read-back only"] = lambda: lg.cpu()
    iters["host log_softmax + topk(20)"] = iters["read-back only"] = max(args.iters // 20, 5)
    if rows <= 64:
        pr = pack_sample_rows([(T, 0, P, 1.0, SEED, STEP, r, 0, 0) for r in range(rows)], dev)
        arms["rows sampled +logprob"] = lambda: ops.sample_rows(lg, pr, return_logprob=True)
    got = ops.logprob_rows(lg, tg, 20, return_rank=True)              # the arms compute the same thing
    want = torch.topk(torch.log_softmax(lg, -1), 20, dim=-1)
    assert torch.equal(lg.gather(1, got["top_ids"].long()), lg.gather(1, want.indices)) and bool((got["rank"] == 1).all())
    assert float((got["top_logprobs"] - want.values).abs().max()) < 1e-4
    times = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name, fn in arms.items():
            times[name].append(time_us(fn, iters.get(name, args.iters)))
    shape = {}
    for name, ts in times.items():
        med = statistics.median(ts)
        shape[name] = {"us": [round(t, 2) for t in ts], "median_us": round(med, 2), "spread": round((max(ts) - min(ts)) / med, 4)}
        print(f"rows={rows:3d} {name:30s} {med:10.1f} us   rounds {[f'{t:.1f}' for t in ts]}  spread {shape[name]['spread']:.3f}", flush=True)
    result["shapes"][f"{rows}x{V}"] = shape
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
