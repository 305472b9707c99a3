"""16-bit vs FP8 (e4m3) paged KV cache at 7B shape, in one process, alternating (config.kv_cache_dtype): the decode step
at batch 4 x 608 cached positions (C5's shape), 4 x 5120 and 16 x 5120 (video chats), the decode-attention kernel class alone
(vt_profile_begin / _end, VT_PROF_ATTN_DECODE) with the page bytes it reads, the C3-shape prefill (5120 rows: the fp8 pool's staging
overhead), vt_probe_read's rate in the same run, and the pool bytes per token. Decoder level only (PackedLlama + llama_forward). The
contexts are written straight into the pools (random finite values): a decode step's time does not depend on what the pages hold.
Prints one JSON line; --out writes it. --shapes prints the byte arithmetic and exits without touching a device.

    python tools/kv8_bench.py [--layers 32] [--iters 20] [--rounds 3] [--dtype bf16] [--out profiles/kv8_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(4, 608), (4, 5120), (16, 5120)]      # (sequences, cached positions incl. the new token)
H, HEADS, HD, PAGE = 4096, 32, 128, 64


def shapes(layers, prefill):
    """byte arithmetic of the run (no device): pool bytes per token, page bytes one decode step's attention reads, staging pool"""
    out = {"bytes_per_token": {"16bit": 2 * layers * HEADS * HD * 2, "fp8": 2 * layers * HEADS * HD}, "cases": {}}
    for b, ctx in CASES:
        tiles = (ctx + PAGE - 1) // PAGE
        out["cases"][f"{b}x{ctx}"] = {fmt: b * tiles * PAGE * out["bytes_per_token"][fmt] for fmt in ("16bit", "fp8")}   # whole tiles are streamed
    ntab = (prefill + PAGE - 1) // PAGE
    out["prefill_staging_bytes"] = ntab * HEADS * PAGE * HD * 2 * 2
    out["pool_pages"] = max(b * ((ctx + PAGE) // PAGE + 1) for b, ctx in CASES) + ntab + 2
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--prefill", type=int, default=5120)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--shapes", action="store_true", help="print the byte arithmetic and exit (no device)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sh = shapes(args.layers, args.prefill)
    if args.shapes:
        print(json.dumps(sh))
        return
    import torch

    from vitron_amd import _lib, synth
    from vitron_amd.engine import PackedLlama, PagedKVCache, SequenceState, llama_forward
    dev = torch.device("cuda:0")
    dt = _lib.torch_dtype(args.dtype)
    lib = _lib.load(operand=args.dtype)
    cfg = dict(hidden_size=H, intermediate_size=11008, num_attention_heads=HEADS, num_hidden_layers=args.layers, vocab_size=32000,
               rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=8192)
    pl = PackedLlama(synth.llama_state(cfg, synth.make_generator(1234, dev), dev, 0.02), cfg, dev, dtype=dt)
    torch.cuda.empty_cache()
    g = torch.Generator(device=dev).manual_seed(5)
    pools = {fmt: PagedKVCache(pl, sh["pool_pages"], kv_dtype=fmt) for fmt in ("16bit", "fp8")}
    assert {f: p.bytes_per_token() for f, p in pools.items()} == sh["bytes_per_token"]
    # contexts straight into the pools: N(0, 1) values in the 16-bit pool, finite e4m3 codes of |x| < 2 in the fp8 pool (chunked: 40 GiB)
    for fmt, kv in pools.items():
        for t in (kv.k, kv.vt):
            for i in range(0, t.numel(), 1 << 28):
                c = t[i:i + (1 << 28)]
                if fmt == "fp8":
                    c.copy_(torch.randint(0, 0x40, c.shape, generator=g, device=dev, dtype=torch.uint8) | (torch.randint(0, 2, c.shape, generator=g, device=dev, dtype=torch.uint8) << 7))
                else:
                    c.copy_(torch.randn(c.shape, generator=g, device=dev, dtype=torch.float32).to(c.dtype))
    step_emb = (torch.randn((16, H), generator=g, device=dev) * 0.5).to(dt)
    pre_emb = (torch.randn((args.prefill, H), generator=g, device=dev) * 0.5).to(dt)

    def make_seqs(b, ctx):       # ctx - 1 cached positions, the step adds one; all cases share the pool's first pages
        per = (ctx + PAGE) // PAGE + 1
        seqs = []
        for i in range(b):
            s = SequenceState()
            s.pages, s.length = list(range(i * per, (i + 1) * per)), ctx - 1
            seqs.append(s)
        return seqs

    def decode(fmt, b, ctx, seqs):
        llama_forward(pl, pools[fmt], seqs, step_emb[:b], [1] * b)
        for s in seqs:            # the same cache position every time
            s.length = ctx - 1

    def prefill(fmt):
        kv = pools[fmt]
        s = SequenceState()
        first = sh["pool_pages"] - (args.prefill + PAGE - 1) // PAGE - 1
        s.pages = list(range(first, first + (args.prefill + PAGE - 1) // PAGE))
        llama_forward(pl, kv, [s], pre_emb, [args.prefill])

    def timed(fn, n):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    res = {"layers": args.layers, "dtype": args.dtype, "iters": args.iters, "rounds": args.rounds, **sh, "decode_ms": {}, "attn_decode_ms": {},
           "attn_decode_GBps": {}, "prefill_ms": {"16bit": [], "fp8": []}}
    for b, ctx in CASES:
        key = f"{b}x{ctx}"
        seqs = make_seqs(b, ctx)
        res["decode_ms"][key] = {"16bit": [], "fp8": []}
        res["attn_decode_ms"][key] = {"16bit": [], "fp8": []}
        for _ in range(args.rounds):          # alternating, so clocks and thermals hit both formats alike
            for fmt in ("16bit", "fp8"):
                res["decode_ms"][key][fmt].append(timed(lambda: decode(fmt, b, ctx, seqs), args.iters))
            for fmt in ("16bit", "fp8"):      # the attention class alone: one launch per layer and step, device-side event timing
                decode(fmt, b, ctx, seqs)
                torch.cuda.synchronize()
                _lib.profile_begin()
                for _ in range(max(2, args.iters // 4)):
                    decode(fmt, b, ctx, seqs)
                prof = _lib.profile_end()["attn_decode"]
                assert prof["launches"] == args.layers * max(2, args.iters // 4), prof
                res["attn_decode_ms"][key][fmt].append(prof["ms"] / prof["launches"] * args.layers)       # per step (all layers)
        res["decode_ms"][key] = {k: min(v) for k, v in res["decode_ms"][key].items()}
        res["attn_decode_ms"][key] = {k: min(v) for k, v in res["attn_decode_ms"][key].items()}
        res["attn_decode_GBps"][key] = {fmt: sh["cases"][key][fmt] / (res["attn_decode_ms"][key][fmt] * 1e-3) / 1e9 for fmt in ("16bit", "fp8")}
    for _ in range(args.rounds):
        for fmt in ("16bit", "fp8"):
            res["prefill_ms"][fmt].append(timed(lambda: prefill(fmt), max(2, args.iters // 10)))
    res["prefill_ms"] = {k: min(v) for k, v in res["prefill_ms"].items()}
    res["decode_ratio_fp8_over_16bit"] = {k: v["fp8"] / v["16bit"] for k, v in res["decode_ms"].items()}
    res["attn_decode_ratio_fp8_over_16bit"] = {k: v["fp8"] / v["16bit"] for k, v in res["attn_decode_ms"].items()}
    res["prefill_ratio_fp8_over_16bit"] = res["prefill_ms"]["fp8"] / res["prefill_ms"]["16bit"]
    # read rate of a kernel that only reads (1 GiB, read-once policy), the yardstick of the page stream, in the same run
    buf = torch.ones(1 << 28, dtype=torch.float32, device=dev)
    flag = torch.zeros(4, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    res["read_probe_GBps"] = (1 << 30) / (timed(lambda: _lib.check(lib.vt_probe_read(buf.data_ptr(), buf.numel() * 4, 1, flag.data_ptr(), st), "vt_probe_read", lib), 20) * 1e-3) / 1e9
    res["attn_decode_share_of_read_probe"] = {k: {f: x / res["read_probe_GBps"] for f, x in v.items()} for k, v in res["attn_decode_GBps"].items()}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
