"""Times the device-side history bans, bf16, one MI355X:
  1. vt_ban_rows through ops.ban_rows at 4 rows x V = 32000, g = 3, eight 3-token sequences, histories of 640 and of 5632 ids; beside
     it vt_sample_rows_allow (greedy rows) reading the masks it wrote, and vt_sample_rows without masks on the same logits
  2. ms per decode step of generate() at the 7B width with and without no_repeat_ngram_size=3 (the one-token call subtracted)
The arms alternate inside every round of one process; medians of --rounds rounds with the rounds shown. One JSON line per arm; --json
PATH also writes them to a file (profiles/ban_bench.json). Reported, not gating."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vitron_amd import _lib, ops, synth  # noqa: E402
from vitron_amd.model import LlavaConfig, LlavaLlamaForCausalLM  # noqa: E402
from vitron_amd.sampling import flatten_ban_seqs, mask_words, pack_ban_rows, pack_sample_rows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--prompt", type=int, default=609)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--json", default=None)
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
gen = synth.make_generator(4321, dev)

# ---- 1: vt_ban_rows alone, beside the sampler launch it feeds --------------------------------------------------------------------------------
ROWS, V, G = 4, 32000, 3
lg = torch.randn((ROWS, V), generator=gen, device=dev) * 3.0
params = pack_sample_rows([(0.0, 0, 1.0, 1.0, 0, 0, b, 0, 0) for b in range(ROWS)], dev)
seqs = torch.from_numpy(flatten_ban_seqs([[100 + 3 * i, 101 + 3 * i, 102 + 3 * i] for i in range(8)])).to(dev)
work = torch.empty((ROWS, mask_words(V)), dtype=torch.int32, device=dev)
ptrs = torch.tensor([work[b].data_ptr() for b in range(ROWS)], dtype=torch.int64).to(dev)
kernel = {}
for n_hist in (640, 5632):
    hist = torch.randint(3, V, (ROWS, n_hist), generator=gen, device=dev).to(torch.int32)
    rows = pack_ban_rows([(hist[b].data_ptr(), n_hist, 0, work[b].data_ptr(), G, seqs.data_ptr(), 8, int(seqs.numel())) for b in range(ROWS)], dev)
    arms = {
        "ban_rows": lambda rows=rows: ops.ban_rows(rows, ROWS, V),
        "sample_rows_allow greedy": lambda: ops.sample_rows(lg, params, _allow_ptrs=ptrs),
        "sample_rows greedy": lambda: ops.sample_rows(lg, params),
    }
    us = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name, fn in arms.items():
            us[name].append(events(fn, args.iters))
    for name in arms:
        note(arm=name, rows=ROWS, V=V, history_len=n_hist, ngram=G, n_seqs=8, us=median(us[name]), us_rounds=us[name])
    kernel[n_hist] = {name: median(v) for name, v in us.items()}

# ---- 2: a generate decode step at the 7B width with and without the ban ------------------------------------------------------------------------
model = LlavaLlamaForCausalLM(LlavaConfig(**synth.VICUNA_7B, mm_hidden_size=1024))
model.init_synthetic(dev, seed=1234)
model.config.kv_prefix_reuse = False
ids = torch.cat([torch.tensor([1], device=dev), torch.randint(3, 32000, (args.prompt - 1,), generator=gen, device=dev)]).unsqueeze(0)
steps = args.steps
arms = {
    "plain": lambda n: model.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=-1, pad_token_id=0),
    "no_repeat_ngram_size=3": lambda n: model.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=-1, pad_token_id=0,
                                                       no_repeat_ngram_size=G),
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
note(arm="summary", step_pays_us=(per_arm["no_repeat_ngram_size=3"] - per_arm["plain"]) * 1e3,
     ban_rows_us={str(n): kernel[n]["ban_rows"] for n in kernel},
     sample_rows_allow_us={str(n): kernel[n]["sample_rows_allow greedy"] for n in kernel})

if args.json:
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
