"""In-process A/B of vt_llama_model.last_layer_full: a 32-layer decoder at 7B width with DISTINCT synthetic weights per layer (13 GB: every
layer's weights arrive cold from HBM, as in the benchmark step), one prefill pass per measurement through vt_llama_forward with the default
logit rows (the last row of every sequence), arms alternated pass by pass on one box, device events around the call.

    python tools/last_layer_ab.py [--pairs 6] [--layers 32] [--shapes C3,C3-224,C2,C2-224,C4]

arm "pruned" = last_layer_full 0 (the default: the last layer runs q / attention / o_proj / MLP on the logit rows only), arm "full" = 1 (the
last layer on all rows, as before the switch existed). One JSON line per shape. The numbers are times, not results; this is the code under
test on both arms, so it supports a comparison against the previous commit (bench.py on both trees) and does not replace it."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vitron_amd import _lib, synth  # noqa: E402
from vitron_amd.engine import PackedLlama, PagedKVCache, SequenceState, llama_forward  # noqa: E402

SHAPES = {"C3": [5120], "C3-224": [2560], "C2": [1088], "C2-224": [768], "C4": [5120] * 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--shapes", default="C3,C3-224,C2,C2-224,C4")
    args = ap.parse_args()
    _lib.load()
    dev = torch.device("cuda:0")
    cfg = dict(synth.VICUNA_7B, num_hidden_layers=args.layers)
    sd = synth.llama_state(cfg, synth.make_generator(1, device=dev), device=dev)
    llama = PackedLlama(sd, cfg, dev, rope_len=5120)
    del sd
    names = args.shapes.split(",")
    kv = PagedKVCache(llama, max(sum((q + 63) // 64 for q in SHAPES[n]) for n in names))
    g = torch.Generator(device=dev).manual_seed(2)
    for name in names:
        q_lens = SHAPES[name]
        x = (torch.randn((sum(q_lens), llama.H), generator=g, device=dev) * 0.02).to(torch.bfloat16)

        def one_pass(full):
            llama.set_last_layer_full(full)
            seqs = [SequenceState() for _ in q_lens]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            llama_forward(llama, kv, seqs, x, q_lens)
            b.record()
            torch.cuda.synchronize()
            for s in seqs:
                kv.release(s.pages)
            return a.elapsed_time(b)

        arms = (("pruned", False), ("full", True))
        for _, full in arms:   # warm-up
            one_pass(full)
        times = {n: [] for n, _ in arms}
        for _ in range(args.pairs):
            for n, full in arms:
                times[n].append(one_pass(full))
        llama.set_last_layer_full(False)
        out = {"shape": name, "q_lens": q_lens, "layers": args.layers, "pairs": args.pairs, "arms": {}}
        for n, _ in arms:
            t = sorted(times[n])
            out["arms"][n] = {"ms_median": round(t[len(t) // 2], 3), "ms_min": round(t[0], 3), "ms_max": round(t[-1], 3), "ms": [round(v, 3) for v in times[n]]}
        d = [f - p for p, f in zip(times["pruned"], times["full"])]
        out["full_minus_pruned_ms"] = {"mean": round(sum(d) / len(d), 3), "min": round(min(d), 3), "max": round(max(d), 3)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
