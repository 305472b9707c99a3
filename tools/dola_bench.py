"""Times DoLa decoding, bf16, one MI355X:
  1. vt_dola_rows through ops.dola_rows at V = 32000 with 8 candidates and 1, 4 and 8 rows, in place, beside the torch composition of
     the same arithmetic (log_softmax of the final row and of the candidates, the divergences, the arg-max, the contrast and the filter
     into a preallocated output)
  2. ms per decode step of generate() at the 7B width (32 layers) at B = 1 and B = 4, plain and with dola_layers="high" (8 candidates):
     (time of --steps tokens - time of 1 token) / (steps - 1)
  3. --plain-only: part 2's plain arm alone, with more repeats. It uses nothing this file's commit added, so the same file runs in a
     checkout of the parent commit: the two outputs side by side show whether the plain step moved, against the spread of the parent's
     own repeats.
The arms alternate inside every round of one process; medians of --rounds rounds with the rounds shown. One JSON line per arm; --json
PATH also writes them to a file (profiles/dola_bench.json). Reported, not gating."""
import argparse
import json
import math
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
ap.add_argument("--plain-only", action="store_true", help="part 3: the plain decode step alone (runs on the parent commit too)")
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
V, N_CAND, RT = 32000, 8, 0.1

# ---- 1: vt_dola_rows beside the torch composition ------------------------------------------------------------------------------------------
if not args.plain_only:
    from vitron_amd import ops
    from vitron_amd.sampling import pack_dola_rows
    kernel = {}
    for ROWS in (1, 4, 8):
        f = torch.randn((ROWS, V), generator=gen, device=dev) * 4.0
        w = torch.linspace(0.1, 1.0, N_CAND, device=dev).view(N_CAND, 1, 1)
        p = ((1.0 - w) * f + w * 4.0 * torch.randn((N_CAND, ROWS, V), generator=gen, device=dev)).contiguous()
        work = f.clone()
        out = torch.empty_like(f)
        layer = torch.empty((ROWS,), dtype=torch.int32, device=dev)
        rows = pack_dola_rows([(work[b].data_ptr(), p[0, b].data_ptr(), p.stride(0), N_CAND, work[b].data_ptr(), 0, 0,
                                layer[b:b + 1].data_ptr(), 0, 0, math.log(RT)) for b in range(ROWS)], dev)

        def torch_arm(f=f, p=p, out=out):
            lf, lp = torch.log_softmax(f, -1), torch.log_softmax(p, -1)
            m = 0.5 * (lf.exp() + lp.exp())
            lm = m.log()
            div = (m * (lm - lf) + m * (lm - lp)).sum(-1)                    # [n_cand, rows] (a term with m == 0 does not occur here)
            j = div.argmax(0)
            sel = lp.gather(0, j.view(1, -1, 1).expand(1, -1, V))[0]
            keep = f >= f.max(-1, keepdim=True).values + math.log(RT)
            torch.where(keep, lf - sel, torch.full_like(lf, -float("inf")), out=out)

        # (in place: after the first launch the kernel contrasts its own output again -- the same work on other values)
        arms = {"dola_rows (in place)": lambda rows=rows, n=ROWS: ops.dola_rows(rows, n, V), "torch: log_softmax, divergences, contrast": torch_arm}
        us = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, fn in arms.items():
                work.copy_(f)
                us[name].append(events(fn, args.iters))
        for name in arms:
            note(arm=name, rows=ROWS, n_cand=N_CAND, V=V, us=median(us[name]), us_rounds=us[name])
        kernel[ROWS] = {name: median(v) for name, v in us.items()}
    note(arm="summary kernels", us={str(r): kernel[r] for r in kernel},
         torch_over_dola_rows={str(r): kernel[r]["torch: log_softmax, divergences, contrast"] / kernel[r]["dola_rows (in place)"] for r in kernel})

# ---- 2 / 3: the decode step of generate(), plain and with DoLa --------------------------------------------------------------------------------
if not args.no_model:
    model = LlavaLlamaForCausalLM(LlavaConfig(**synth.VICUNA_7B, mm_hidden_size=1024))
    model.init_synthetic(dev, seed=1234)
    model.config.kv_prefix_reuse = False
    steps = args.steps
    rounds = args.rounds + (4 if args.plain_only else 0)

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
        ids = prompt(B)
        arms = {"plain": {}}
        if not args.plain_only:
            arms['dola_layers="high"'] = dict(dola_layers="high")
        ms = {name: [] for name in arms}
        for rnd in range(rounds + 1):                       # round 0 warms up
            for name, kw in arms.items():
                v = step_ms(ids, **kw)
                if rnd:
                    ms[name].append(v)
        for name in arms:
            per[(B, name)] = median(ms[name])
            note(arm=f"decode step, {name}", label=args.label, B=B, prompt=args.prompt, steps=steps, ms_per_step=median(ms[name]),
                 ms_per_step_rounds=ms[name], spread=(max(ms[name]) - min(ms[name])) / median(ms[name]))
    if not args.plain_only:
        note(arm="summary decode step", dola_over_plain={str(B): per[(B, 'dola_layers="high"')] / per[(B, "plain")] for B in (1, 4)},
             dola_minus_plain_ms={str(B): per[(B, 'dola_layers="high"')] - per[(B, "plain")] for B in (1, 4)})

if args.json:
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
