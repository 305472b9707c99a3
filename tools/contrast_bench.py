"""Times contrastive search at the 7B width, bf16, one MI355X:
  1. ms per step of generate(penalty_alpha=0.6, top_k=k): prompt of --prompt rows, --steps steps (the one-token call subtracted), beside
     a plain batch-k greedy decode step on the same build and the same prompt (k copies of it); arms alternated in every round
  2. the step's parts alone, as the step launches them: ops.logprob_rows (top k of one row), ops.unit_rows (k rows), ops.contrast_rows
     (one group, T = --prompt), the read-back of (sel, id), and ops.kv_copy_pages of k - 1 pages
  3. vt_contrast_rows alone at T = --prompt and T = 5120 + 256, k = 4 and 16, beside T * H * 2 bytes at vt_probe_read's rate measured in the
     same run (banks of random unit rows; the bank at the large T is 44 MB). These are device events around ops.contrast_rows, host work
     included; --trace-T runs the launches alone for a kernel trace
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

ap = argparse.ArgumentParser()
ap.add_argument("--prompt", type=int, default=609)
ap.add_argument("--k", type=int, default=4)
ap.add_argument("--steps", type=int, default=32)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--no-model", action="store_true", help="skip the generate() arms (parts 1 and the page copies of part 2)")
ap.add_argument("--trace-T", type=int, default=0, help="only --iters launches of vt_contrast_rows at this bank length and --k: the run to put under "
                "rocprofv3 --kernel-trace --stats for the two stages' device times")
ap.add_argument("--cold", action="store_true", help="with --trace-T: read 1 GiB (vt_probe_read) between the launches, so that the bank comes from "
                "HBM as it does behind a decode pass that streamed the weights, not from the Infinity Cache")
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


lib = _lib.load()
dev = torch.device("cuda:0")
k, steps, H, V = args.k, args.steps, 4096, 32000
gen = synth.make_generator(4321, dev)

if args.trace_T:
    T = args.trace_T
    x = torch.randn((T + 1, H), generator=gen, device=dev)
    bank = (x / x.norm(dim=1, keepdim=True)).bfloat16()
    cand = bank[:k].clone()
    lp = torch.log_softmax(torch.randn((k,), generator=gen, device=dev), 0)
    d, sc, sel = torch.empty((k,), device=dev), torch.empty((k,), device=dev), torch.empty((1,), dtype=torch.int32, device=dev)
    ws = ops.contrast_workspace(1, T, dev)
    grp = [dict(bank=bank, bank_len=T, k=k, first=0, alpha=0.6, lp=lp, d=d, score=sc, sel=sel)]
    flush = torch.empty((1 << 28,), dtype=torch.float32, device=dev)
    flag = torch.zeros((1,), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def one():
        if args.cold:
            _lib.check(lib.vt_probe_read(flush.data_ptr(), flush.numel() * 4, 1, flag.data_ptr(), st), "vt_probe_read", lib)
        ops.contrast_rows(grp, cand, ws)
    note(arm="contrast_rows under trace", T=T, k=k, H=H, cold=bool(args.cold), us_with_host_and_flush=events(one, args.iters))
    sys.exit(0)

# ---- 1: a contrastive step beside a plain batch-k decode step ----------------------------------------------------------------------------------
if not args.no_model:
    model = LlavaLlamaForCausalLM(LlavaConfig(**synth.VICUNA_7B, mm_hidden_size=1024))
    model.init_synthetic(dev, seed=1234)
    model.config.kv_prefix_reuse = False
    ids = torch.cat([torch.tensor([1], device=dev), torch.randint(3, 32000, (args.prompt - 1,), generator=gen, device=dev)]).unsqueeze(0)
    arms = {
        "contrastive": lambda n: model.generate(ids, penalty_alpha=0.6, top_k=k, max_new_tokens=n, eos_token_id=-1, pad_token_id=0),
        "plain": lambda n: model.generate(ids.repeat(k, 1), do_sample=False, max_new_tokens=n, eos_token_id=-1, pad_token_id=0),
    }
    for fn in arms.values():
        fn(4)
    times = {name: {"full": [], "first": []} for name in arms}
    for _ in range(args.rounds):          # the arms alternate inside every round
        for name, fn in arms.items():
            times[name]["first"].append(wall(lambda: fn(1)))
            times[name]["full"].append(wall(lambda: fn(steps + 1)))
            if name == "contrastive":
                stats = dict(model.last_generate_stats)
    for name in arms:
        per = [(f - p) / steps for f, p in zip(times[name]["full"], times[name]["first"])]
        note(arm=f"{name} step", prompt_rows=args.prompt, rows_per_step=k, steps=steps, ms_per_step=median(per), ms_per_step_rounds=per,
             first_token_ms=median(times[name]["first"]))
    note(arm="contrastive pages copied", pages=stats["pages_copied"], steps=stats["contrastive_steps"])


# ---- 2, 3: the parts ----------------------------------------------------------------------------------------------------------------------------------
def unit_bank(T):
    x = torch.randn((T + 1, H), generator=gen, device=dev)
    return (x / x.norm(dim=1, keepdim=True)).bfloat16()


flag = torch.zeros((1,), dtype=torch.int32, device=dev)
probe = torch.empty((1 << 28,), dtype=torch.float32, device=dev)          # 1 GiB: larger than the Infinity Cache
st = torch.cuda.current_stream().cuda_stream
row = torch.randn((1, V), generator=gen, device=dev) * 3.0
hid = torch.randn((k, H), generator=gen, device=dev)
w = 1.0 + 0.1 * torch.randn((H,), generator=gen, device=dev)
for rnd in range(args.rounds):
    gbps = (1 << 30) / (events(lambda: _lib.check(lib.vt_probe_read(probe.data_ptr(), probe.numel() * 4, 1, flag.data_ptr(), st), "vt_probe_read", lib), 10) * 1e-6) / 1e9
    note(arm="probe_read", round=rnd, GBps=gbps)
    note(arm="logprob_rows top-k", round=rnd, rows=1, V=V, n_top=k, us=events(lambda: ops.logprob_rows(row, None, k), args.iters))
    note(arm="unit_rows", round=rnd, rows=k, H=H, us=events(lambda: ops.unit_rows(hid, w, dtype=torch.bfloat16), args.iters))
    for T in (args.prompt, 5120 + 256):
        for kk in (4, 16):
            bank = unit_bank(T)
            cand = unit_bank(kk - 1)
            lp = torch.log_softmax(torch.randn((kk,), generator=gen, device=dev), 0)
            d, sc, sel = torch.empty((kk,), device=dev), torch.empty((kk,), device=dev), torch.empty((1,), dtype=torch.int32, device=dev)
            ws = ops.contrast_workspace(1, T, dev)
            grp = [dict(bank=bank, bank_len=T, k=kk, first=0, alpha=0.6, lp=lp, d=d, score=sc, sel=sel)]
            us = events(lambda: ops.contrast_rows(grp, cand, ws), args.iters)
            ideal = T * H * 2 / (gbps * 1e9) * 1e6
            note(arm="contrast_rows", round=rnd, T=T, k=kk, H=H, us=us, bank_bytes=T * H * 2, us_at_probe_rate=ideal, ratio=us / ideal)
            del bank
    pair = torch.zeros((2, 1), dtype=torch.int32, device=dev)
    note(arm="read-back of (sel, id)", round=rnd, us=events(lambda: pair.cpu(), args.iters))
    if not args.no_model:
        llama = model.model.llama
        kv = PagedKVCache(llama, 16, kv_dtype="16bit")
        us = events(lambda: ops.kv_copy_pages(kv, [0] * (k - 1), list(range(8, 8 + k - 1))), 50)
        note(arm="kv_copy_pages of k - 1 pages", round=rnd, pages=k - 1, us=us, us_per_page=us / (k - 1))
        del kv

if args.json:
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
