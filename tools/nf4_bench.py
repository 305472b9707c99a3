"""16-bit vs NF4 (load_4bit) decoder at 7B shape, in one process, alternating: the decode step of C5's decoder shape (4 sequences, one new
token each, ~608 cached positions) and the prefill of C3's decoder shape (one 5120-row sequence), plus vt_probe_read's read rate.
Decoder level only (PackedLlama + llama_forward: the towers are the same code in both formats). Prints one JSON line; --out writes it.

    python tools/nf4_bench.py [--layers 32] [--iters 20] [--dtype bf16] [--out profiles/nf4_bench.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--prefill", type=int, default=5120)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from vitron_amd import _lib, synth
    from vitron_amd.engine import PackedLlama, PagedKVCache, SequenceState, llama_forward
    dev = torch.device("cuda:0")
    dt = _lib.torch_dtype(args.dtype)
    lib = _lib.load(operand=args.dtype)
    cfg = dict(hidden_size=4096, intermediate_size=11008, num_attention_heads=32, num_hidden_layers=args.layers, vocab_size=32000,
               rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=8192)
    sd = synth.llama_state(cfg, synth.make_generator(1234, dev), dev, 0.02)
    models = {"16bit": PackedLlama(sd, cfg, dev, dtype=dt), "nf4": PackedLlama(sd, cfg, dev, dtype=dt, weight_format="nf4")}
    del sd
    torch.cuda.empty_cache()
    H = cfg["hidden_size"]
    g = torch.Generator(device=dev).manual_seed(5)
    ctx_emb = (torch.randn((4 * 607, H), generator=g, device=dev) * 0.5).to(dt)
    pre_emb = (torch.randn((args.prefill, H), generator=g, device=dev) * 0.5).to(dt)
    step_emb = (torch.randn((4, H), generator=g, device=dev) * 0.5).to(dt)
    state = {}
    for name, pl in models.items():
        kv = PagedKVCache(pl, 4 * 12 + args.prefill // 64 + 2)
        seqs = [SequenceState() for _ in range(4)]
        llama_forward(pl, kv, seqs, ctx_emb, [607] * 4)
        state[name] = (pl, kv, seqs)

    def decode(name):
        pl, kv, seqs = state[name]
        lens = [s.length for s in seqs]
        llama_forward(pl, kv, seqs, step_emb, [1] * 4)
        for s, n in zip(seqs, lens):      # the same cache position every time: rewind after the step
            s.length = n

    def prefill(name):
        pl, kv, _ = state[name]
        s = SequenceState()
        llama_forward(pl, kv, [s], pre_emb, [args.prefill])
        kv.release(s.pages)

    def timed(fn, name, n):
        fn(name)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn(name)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    res = {"layers": args.layers, "dtype": args.dtype, "decode_rows": 4, "decode_ctx": 608, "prefill_rows": args.prefill,
           "decoder_weight_bytes": {k: m.decoder_weight_bytes() for k, m in models.items()}, "decode_ms": {}, "prefill_ms": {}}
    for name in models:
        res["decode_ms"][name], res["prefill_ms"][name] = [], []
    for _ in range(args.rounds):          # alternating, so clocks and thermals hit both formats alike
        for name in models:
            res["decode_ms"][name].append(timed(decode, name, args.iters))
        for name in models:
            res["prefill_ms"][name].append(timed(prefill, name, max(2, args.iters // 5)))
    for key in ("decode_ms", "prefill_ms"):
        res[key] = {k: min(v) for k, v in res[key].items()}
    res["decode_ratio_nf4_over_16bit"] = res["decode_ms"]["nf4"] / res["decode_ms"]["16bit"]
    res["prefill_ratio_nf4_over_16bit"] = res["prefill_ms"]["nf4"] / res["prefill_ms"]["16bit"]
    # read rate of a kernel that only reads (1 GiB, read-once policy), the yardstick of the weight stream
    buf = torch.ones(1 << 28, dtype=torch.float32, device=dev)
    flag = torch.zeros(4, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        _lib.check(lib.vt_probe_read(buf.data_ptr(), buf.numel() * 4, 1, flag.data_ptr(), st), "vt_probe_read", lib)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        lib.vt_probe_read(buf.data_ptr(), buf.numel() * 4, 1, flag.data_ptr(), st)
    torch.cuda.synchronize()
    res["read_probe_GBps"] = (1 << 30) * 20 / (time.perf_counter() - t0) / 1e9
    nf4_bytes = res["decoder_weight_bytes"]["nf4"]
    res["nf4_decode_weight_GBps"] = nf4_bytes / (res["decode_ms"]["nf4"] * 1e-3) / 1e9   # weights only (+ lm_head, KV not counted)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
