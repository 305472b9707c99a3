"""A/B of two PLANS of the MFMA GEMM on given shapes -- a single grid or a forced column split (vt_gemm_bf16_colsplit) -- measurement
helper, not part of the product path.

    python tools/colsplit_ab.py "5120,22016,4096,SWIGLU_BF16:13:14/12288/13;768,22016,4096,SWIGLU_BF16:13/21760/0:16/16384/15" [iters] [rounds]

A plan is `cfg` (one launch) or `cfg_first/cols_first/cfg_rest` (two launches; cfg_rest 0 = planned again). Per shape: the weights are
rotated over enough copies (>= 4, >= 600 MB in total) that no launch streams them from the 256 MB Infinity Cache; after one untimed round of
every arm (clocks and code objects warm) the arms run in the order old A, new, old B for `rounds` rounds, each arm timed with device events
over `iters` calls -- both launches of a split inside the window. The two old arms are the noise: `new_below_both_every_round` is the verdict
a plan change needs. The outputs of the two plans are compared bit for bit. One JSON line per round and one summary line per shape."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vitron_amd import _lib, ops  # noqa: E402


def parse_plan(s):
    p = [int(x) for x in s.split("/")]
    assert len(p) in (1, 3), s
    return (p[0], None) if len(p) == 1 else (p[0], (p[1], p[2]))


def main():
    specs = [s for s in sys.argv[1].split(";") if s]
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    _lib.load()
    dev = torch.device("cuda:0")
    for spec in specs:
        shape, old_s, new_s = spec.split(":")
        M, N, K, epi_name = shape.split(",")
        M, N, K = int(M), int(N), int(K)
        epi = getattr(ops, "EPI_" + epi_name)
        plans = {"old": parse_plan(old_s), "new": parse_plan(new_s)}
        a = torch.randn((M, K), device=dev).bfloat16()
        nw = max(4, -(-600_000_000 // (N * K * 2)))
        ws = [(torch.randn((N, K), device=dev) * 0.02).bfloat16() for _ in range(nw)]
        resid = torch.randn((M, N), device=dev) if epi_name == "F32_RESID" else None

        def run(plan, i, out):
            cfg, split = plans[plan]
            return ops.gemm(a, ws[i % nw], None, epi, out=out, cfg=cfg, colsplit=split)

        outs = {p: run(p, 0, resid.clone() if resid is not None else None).clone() for p in plans}
        torch.cuda.synchronize()
        bit_equal = bool(torch.equal(outs["old"], outs["new"]))
        out = outs["old"]
        del outs

        def timed(plan):
            for i in range(3):
                run(plan, i, out)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                run(plan, i, out)
            e1.record()
            torch.cuda.synchronize()
            return round(e0.elapsed_time(e1) / iters * 1e3, 1)

        for arm in ("old", "new", "old"):   # untimed round
            timed(arm)
        rows = []
        for r in range(rounds):
            row = {"shape": [M, N, K], "epi": epi_name, "round": r, "old_a": timed("old"), "new": timed("new"), "old_b": timed("old")}
            rows.append(row)
            print(json.dumps(row), flush=True)
        med = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731
        print(json.dumps({"shape": [M, N, K], "epi": epi_name, "old_plan": old_s, "new_plan": new_s, "weight_sets": nw, "iters": iters,
                          "auto_plan": list(ops.gemm_plan_split(M, N, K, epi)), "bit_equal": bit_equal,
                          "old_us_median": med([r["old_a"] for r in rows] + [r["old_b"] for r in rows]), "new_us_median": med([r["new"] for r in rows]),
                          "new_below_both_every_round": all(r["new"] < min(r["old_a"], r["old_b"]) for r in rows)}), flush=True)
        del a, ws, out, resid


if __name__ == "__main__":
    main()
