"""Times classifier-free guidance, bf16, one MI355X:
  1. vt_cfg_rows through ops.cfg_rows at V = 32000 with 1, 4 and 8 rows, in place, beside the torch composition of the same run (two
     log_softmax and the blend s * (cl - ul) + ul into a preallocated output)
  2. ms per decode step of generate() at the 7B width (32 layers) at B = 1 and B = 4, unguided and guided against a negative prompt of
     the prompt's own length (the same context lengths in all 2B rows): (time of --steps tokens - time of 1 token) / (steps - 1)
  3. --unguided-only: part 2's unguided arm alone, with more repeats. It uses nothing this file's commit added, so the same file runs
     in a checkout of the parent commit: the two outputs side by side show whether the unguided step moved, against the spread of the
     parent's own repeats.
The arms alternate inside every round of one process; medians of --rounds rounds with the rounds shown. One JSON line per arm; --json
PATH also writes them to a file (profiles/cfg_bench.json). Reported, not gating."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vitron_amd import _lib, synth  # noqa: E402
from vitron_amd.model import LlavaConfig, LlavaLlamaForCausalLM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--prompt", type=int, default=64)
ap.add_argument("--steps", type=int, default=33)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--json", default=None)
ap.add_argument("--label", default="this commit")
ap.add_argument("--no-model", action="store_true", help="part 1 only")
ap.add_argument("--unguided-only", action="store_true", help="part 3: the unguided decode step alone (runs on the parent commit too)")
args = ap.parse_args()
results = []


def note(**kw):
    results.append(kw)
    print(json.dumps(kw), flush=True)


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
V = 32000

# ---- 1: vt_cfg_rows beside the torch composition ---------------------------------------------------------------------------------------------
if not args.unguided_only:
    from vitron_amd import ops
    from vitron_amd.sampling import pack_cfg_rows
    kernel = {}
    for ROWS in (1, 4, 8):
        c = torch.randn((ROWS, V), generator=gen, device=dev) * 3.0
        u = torch.randn((ROWS, V), generator=gen, device=dev) * 3.0
        work = c.clone()
        out = torch.empty_like(c)
        rows = pack_cfg_rows([(work[b].data_ptr(), u[b].data_ptr(), work[b].data_ptr(), 0, 0, 0, 2.5, -float("inf")) for b in range(ROWS)], dev)

        def torch_arm(c=c, u=u, out=out):
            cl, ul = torch.log_softmax(c, -1), torch.log_softmax(u, -1)
            torch.add(ul, cl - ul, alpha=2.5, out=out)

        # (in place: after the first launch the kernel blends its own output again -- the same work on other values)
        arms = {"cfg_rows (in place)": lambda rows=rows, n=ROWS: ops.cfg_rows(rows, n, V), "torch: 2 log_softmax + blend": torch_arm}
        us = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, fn in arms.items():
                work.copy_(c)
                us[name].append(events(fn, args.iters))
        for name in arms:
            note(arm=name, rows=ROWS, V=V, us=median(us[name]), us_rounds=us[name])
        kernel[ROWS] = {name: median(v) for name, v in us.items()}
    note(arm="summary kernels", us={str(r): kernel[r] for r in kernel},
         torch_over_cfg_rows={str(r): kernel[r]["torch: 2 log_softmax + blend"] / kernel[r]["cfg_rows (in place)"] for r in kernel})

# ---- 2 / 3: the decode step of generate(), unguided and guided ---------------------------------------------------------------------------------
if not args.no_model:
    model = LlavaLlamaForCausalLM(LlavaConfig(**synth.VICUNA_7B, mm_hidden_size=1024))
    model.init_synthetic(dev, seed=1234)
    model.config.kv_prefix_reuse = False
    steps = args.steps
    rounds = args.rounds + (4 if args.unguided_only else 0)

    def prompt(B):
        return torch.cat([torch.ones((B, 1), dtype=torch.long, device=dev),
                          torch.randint(3, V, (B, args.prompt - 1), generator=gen, device=dev)], 1)

    def step_ms(ids, **kw):
        t = {}
        for n in (1, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=-1, pad_token_id=0, **kw)
            torch.cuda.synchronize()
            t[n] = (time.perf_counter() - t0) * 1e3
        return (t[steps] - t[1]) / (steps - 1)

    per = {}
    for B in (1, 4):
        ids, neg = prompt(B), prompt(B)
        arms = {"unguided": {}}
        if not args.unguided_only:
            arms["guided (scale 2.5)"] = dict(guidance_scale=2.5, negative_prompt_ids=neg)
        ms = {name: [] for name in arms}
        for rnd in range(rounds + 1):                       # round 0 warms up
            for name, kw in arms.items():
                v = step_ms(ids, **kw)
                if rnd:
                    ms[name].append(v)
        for name in arms:
            per[(B, name)] = median(ms[name])
            note(arm=f"decode step, {name}", label=args.label, B=B, decode_rows=B * (2 if name != "unguided" else 1), prompt=args.prompt,
                 steps=steps, ms_per_step=median(ms[name]), ms_per_step_rounds=ms[name],
                 spread=(max(ms[name]) - min(ms[name])) / median(ms[name]))
    if not args.unguided_only:
        note(arm="summary decode step", guided_over_unguided={str(B): per[(B, "guided (scale 2.5)")] / per[(B, "unguided")] for B in (1, 4)})

if args.json:
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
