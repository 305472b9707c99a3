"""Times beam search at the 7B width, bf16, one MI355X:
  1. ms per beam step of generate(num_beams=k): prompt of --prompt rows, k beams, --steps steps (the prefill-only call subtracted)
  2. ms of a plain batch-k greedy decode step on the same build and the same prompt (k copies of it)
  3. vt_beam_step alone on [k, 32000] logits, beside vt_sample_rows (greedy rows) on the same rows
  4. vt_kv_copy_pages per page, beside a device-to-device copy of the same bytes (page bytes x 2 pools x layers)
One JSON line per arm; --json PATH also writes them to a file. Reported, not gating."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vitron_amd import _lib, ops, synth  # noqa: E402
from vitron_amd.engine import PagedKVCache  # noqa: E402
from vitron_amd.model import LlavaConfig, LlavaLlamaForCausalLM  # noqa: E402
from vitron_amd.sampling import pack_sample_rows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--prompt", type=int, default=609)
ap.add_argument("--beams", type=int, default=4)
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
k, steps = args.beams, args.steps
model = LlavaLlamaForCausalLM(LlavaConfig(**synth.VICUNA_7B, mm_hidden_size=1024))
model.init_synthetic(dev, seed=1234)
model.config.kv_prefix_reuse = False
gen = synth.make_generator(4321, dev)
ids = torch.cat([torch.tensor([1], device=dev), torch.randint(3, 32000, (args.prompt - 1,), generator=gen, device=dev)]).unsqueeze(0)

# ---- 1, 2: a beam step beside a plain batch-k decode step -----------------------------------------------------------------------------------
arms = {
    "beam": lambda n: model.generate(ids, num_beams=k, max_new_tokens=n, eos_token_id=-1, pad_token_id=0),
    "plain": lambda n: model.generate(ids.repeat(k, 1), do_sample=False, max_new_tokens=n, eos_token_id=-1, pad_token_id=0),
}
for fn in arms.values():
    fn(4)
times = {name: {"full": [], "first": []} for name in arms}
for _ in range(args.rounds):          # the arms alternate inside every round
    for name, fn in arms.items():
        times[name]["first"].append(wall(lambda: fn(1)))
        times[name]["full"].append(wall(lambda: fn(steps + 1)))
for name in arms:
    per = [(f - p) / steps for f, p in zip(times[name]["full"], times[name]["first"])]
    note(arm=f"{name} step", prompt_rows=args.prompt, rows_per_step=k, steps=steps, ms_per_step=median(per), ms_per_step_rounds=per,
         first_token_ms=median(times[name]["first"]))

# ---- 3: vt_beam_step alone ---------------------------------------------------------------------------------------------------------------------
V = 32000
lg = torch.randn((k, V), generator=gen, device=dev) * 3.0
bs = torch.zeros((k,), device=dev) - 1.0
rows = pack_sample_rows([(0.0, 0, 1.0, 1.0, 0, 0, b, 0, 0) for b in range(k)], dev)
for _ in range(args.rounds):
    note(arm="beam_step", rows=k, V=V, n_out=2 * k, us=events(lambda: ops.beam_step(lg, bs, 1, k, 2 * k), args.iters))
    note(arm="sample_rows greedy", rows=k, V=V, us=events(lambda: ops.sample_rows(lg, rows), args.iters))
    note(arm="sample_rows greedy +logprob", rows=k, V=V, us=events(lambda: ops.sample_rows(lg, rows, return_logprob=True), args.iters))

# ---- 4: vt_kv_copy_pages -----------------------------------------------------------------------------------------------------------------------
llama = model.model.llama
for fmt in ("16bit", "fp8"):
    kv = PagedKVCache(llama, 16, kv_dtype=fmt)
    page_bytes = llama.heads * 64 * llama.hd * kv.k.element_size()
    moved = page_bytes * 2 * llama.L                     # bytes read (and as many written) per page pair
    n = 4
    src, dst = list(range(n)), list(range(8, 8 + n))
    a = torch.empty((n * moved,), dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    for _ in range(args.rounds):
        us = events(lambda: ops.kv_copy_pages(kv, src, dst), 50)
        us_d2d = events(lambda: b.copy_(a), 50)
        note(arm=f"kv_copy_pages {fmt}", pages=n, bytes_per_page=moved, us_per_page=us / n, GBps_read_plus_write=2 * n * moved / us / 1e3,
             d2d_copy_same_bytes_us_per_page=us_d2d / n, d2d_GBps_read_plus_write=2 * n * moved / us_d2d / 1e3)
    del kv, a, b

if args.json:
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
