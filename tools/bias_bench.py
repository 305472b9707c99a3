"""Times the additive adjustments, bf16, one MI355X:
  1. vt_bias_rows through ops.bias_rows at 4 and 16 rows x V = 32000 (64 biased ids, presence and frequency set) with generated
     histories of 64 and of 1024 ids; beside it vt_sample_rows_adj reading the adjustments it wrote and vt_sample_rows_allow on the same
     rows (greedy rows, and sampled rows with top_k = 50 / top_p = 0.9), all with all-ones masks
  2. ms per decode step of generate() at the 7B width with and without frequency_penalty=0.5 (the one-token call subtracted)
The arms alternate inside every round of one process; medians of --rounds rounds with the rounds shown. One JSON line per arm; --json
PATH also writes them to a file (profiles/bias_bench.json). Reported, not gating."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vitron_amd import _lib, ops, synth  # noqa: E402
from vitron_amd.model import LlavaConfig, LlavaLlamaForCausalLM  # noqa: E402
from vitron_amd.sampling import mask_words, pack_bias_rows, pack_sample_rows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--prompt", type=int, default=609)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--json", default=None)
ap.add_argument("--skip-generate", action="store_true")
args = ap.parse_args()
results = []


def note(**kw):
    results.append(kw)
    print(json.dumps(kw), flush=True)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn, iters):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # us


def median(xs):
    return sorted(xs)[len(xs) // 2]


_lib.load()
dev = torch.device("cuda:0")
gen = synth.make_generator(4322, dev)

# ---- 1: vt_bias_rows alone, beside the sampler launch it feeds --------------------------------------------------------------------------------
V, N_BIAS = 32000, 64
kernel = {}
for ROWS in (4, 16):
    lg = torch.randn((ROWS, V), generator=gen, device=dev) * 3.0
    greedy = pack_sample_rows([(0.0, 0, 1.0, 1.0, 0, 0, b, 0, 0) for b in range(ROWS)], dev)
    sampled = pack_sample_rows([(0.8, 50, 0.9, 1.0, 7, 0, b, 0, 0) for b in range(ROWS)], dev)
    ones = torch.full((mask_words(V),), -1, dtype=torch.int32, device=dev)
    allow_ptrs = torch.tensor([ones.data_ptr()] * ROWS, dtype=torch.int64).to(dev)
    adj = torch.zeros((ROWS, V, 2), dtype=torch.float32, device=dev)
    adj_ptrs = torch.tensor([adj[b].data_ptr() for b in range(ROWS)], dtype=torch.int64).to(dev)
    bias_ids = torch.randperm(V, generator=gen, device=dev)[:N_BIAS].to(torch.int32)
    bias_vals = torch.randn((N_BIAS,), generator=gen, device=dev)
    for n_hist in (64, 1024):
        hist = torch.randint(3, V, (ROWS, n_hist), generator=gen, device=dev).to(torch.int32)
        rows = pack_bias_rows([(hist[b].data_ptr(), n_hist, bias_ids.data_ptr(), bias_vals.data_ptr(), N_BIAS, adj[b].data_ptr(), 0.3, 0.5)
                               for b in range(ROWS)], dev)
        arms = {
            "bias_rows": lambda rows=rows, ROWS=ROWS: ops.bias_rows(rows, ROWS, V),
            "sample_rows_adj greedy": lambda: ops.sample_rows(lg, greedy, _allow_ptrs=allow_ptrs, _adjust_ptrs=adj_ptrs),
            "sample_rows_allow greedy": lambda: ops.sample_rows(lg, greedy, _allow_ptrs=allow_ptrs),
            "sample_rows_adj sampled": lambda: ops.sample_rows(lg, sampled, _allow_ptrs=allow_ptrs, _adjust_ptrs=adj_ptrs),
            "sample_rows_allow sampled": lambda: ops.sample_rows(lg, sampled, _allow_ptrs=allow_ptrs),
        }
        us = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, fn in arms.items():
                us[name].append(events(fn, args.iters))
        for name in arms:
            note(arm=name, rows=ROWS, V=V, history_len=n_hist, n_bias=N_BIAS, us=median(us[name]), us_rounds=us[name])
        kernel[f"{ROWS}x{n_hist}"] = {name: median(v) for name, v in us.items()}

# ---- 2: a generate decode step at the 7B width with and without the penalty -------------------------------------------------------------------
if not args.skip_generate:
    model = LlavaLlamaForCausalLM(LlavaConfig(**synth.VICUNA_7B, mm_hidden_size=1024))
    model.init_synthetic(dev, seed=1234)
    model.config.kv_prefix_reuse = False
    ids = torch.cat([torch.tensor([1], device=dev), torch.randint(3, 32000, (args.prompt - 1,), generator=gen, device=dev)]).unsqueeze(0)
    steps = args.steps
    arms = {
        "plain": lambda n: model.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=-1, pad_token_id=0),
        "frequency_penalty=0.5": lambda n: model.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=-1, pad_token_id=0,
                                                          frequency_penalty=0.5),
    }
    for fn in arms.values():
        fn(4)
    times = {name: {"full": [], "first": []} for name in arms}
    for _ in range(args.rounds):          # the arms alternate inside every round
        for name, fn in arms.items():
            times[name]["first"].append(wall(lambda: fn(1)))
            times[name]["full"].append(wall(lambda: fn(steps + 1)))
    per_arm = {}
    for name in arms:
        per = [(f - p) / steps for f, p in zip(times[name]["full"], times[name]["first"])]
        per_arm[name] = median(per)
        note(arm=f"generate step, {name}", prompt_rows=args.prompt, steps=steps, ms_per_step=median(per), ms_per_step_rounds=per,
             first_token_ms=median(times[name]["first"]))
    note(arm="summary", step_pays_us=(per_arm["frequency_penalty=0.5"] - per_arm["plain"]) * 1e3,
         bias_rows_us={k: v["bias_rows"] for k, v in kernel.items()},
         sample_rows_adj_greedy_us={k: v["sample_rows_adj greedy"] for k, v in kernel.items()},
         sample_rows_allow_greedy_us={k: v["sample_rows_allow greedy"] for k, v in kernel.items()})

if args.json:
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
