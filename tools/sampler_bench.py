"""Times vt_argmax, vt_sample_top_p, vt_sample_rows and vt_sample_rows_allow on decode-sized logits ([rows, 32000] fp32).

vt_sample_rows runs all-sampled, all-greedy and mixed batches (even rows greedy), each without a history and with a 2048-id history under
a repetition penalty of 1.3, and all-sampled with the log-probability output.

The constrained arms (vt_sample_rows_allow) run the all-sampled batch only, with an allow mask of about half the vocabulary
on every row ("allow all rows") and on the odd rows only ("allow half rows", the others NULL). Each runs with the pointer array built
beforehand (the kernel's cost) and built per call from the list of masks ("+ptrs": what ServingEngine._pick pays). "step mask upload" is
the host build and the ceil(V / 32) * 4-byte upload of ONE step-dependent mask, of 16000 ids and of 8: the engine's extra cost per
constrained row and step.

The truncation arms (vt_sample_rows_trunc) run the all-sampled batch too: the entry point with trunc = NULL (the
vt_sample_rows launch itself) and with all-inactive rows (the trunc kernel, stages skipped) -- to be read against "rows sampled" and, with
--baseline-lib, against the two "baseline rows sampled" arms, whose difference is the spread of repeated parent runs --, each stage
alone and all four. "host warpers" is what the feature replaces: the [rows, V] fp32 logits read back and transformers' temperature /
top-p / MinP / Typical / Epsilon / Eta warpers, a softmax and torch.multinomial on the CPU.

The Mirostat arms (vt_sample_rows_miro) run the all-sampled batch through raw ctypes: "miro tau 5" (every row on Mirostat,
tau 5, eta 0.1, no truncation) beside "trunc all inactive +restore", and "miro tau 5 + all four" beside "trunc all four +restore", on the
same rows. A Mirostat launch moves its cells, so every launch of these four arms is preceded by the same 8 * rows-byte copy that puts the
cells back ("+restore": the trunc arms pay it too, so that a pair differs by the kernel and its read-back of the array alone).
"miro cells NULL" is the entry point with an array whose every cell is NULL: the read-back of the array and the kMiro kernel with its
stage off, so "miro cells NULL" less "trunc all inactive +restore" is what the validation costs and "miro tau 5" less "miro cells NULL"
what the stage costs. "miro entry, miro=NULL" is the vt_sample_rows_trunc launch itself. profiles/miro_bench.json is the run of DESIGN.md 9.17.

The arms are alternated inside one process over `--rounds` rounds of `--iters` launches between two device events; per arm the output
gives every round, the median and the spread (max - min) / median -- two arms are apart only when they differ by more than the spreads.
`--baseline-lib PATH` adds ANOTHER build of libvitron_hip.so (for instance the parent commit's) to the same alternation: its vt_argmax
and vt_sample_top_p, and one "baseline raw ..." arm per flavour of the vt_sample_rows kernel beside a "new raw ..." arm of this build, both
through raw ctypes on the same device arrays -- plain, allow (all rows), adj (a zero adjustment on every row), trunc (all four) and wm
(depth 30, the array of tools/wm_bench.py; the cells are put back in front of every launch of either arm). Where PATH lies inside a
vitron_amd package, that package's ops.sample_rows runs beside this one's as well ("baseline ops ..." / "new ops ...": the host cost of
the Python path). Every such pair is listed under "ab" with its verdict: apart only when the medians differ by more than the largest of
the two spreads and the spread of "baseline rows sampled (again)". `--json FILE` writes the table (profiles/sampler_rows_bench.json: the
run of DESIGN.md 9.3; profiles/sampler_allow_bench.json: the run of 9.4, with the constrained arms; profiles/sampler_one_kernel_ab.json:
the A/B against the parent of the one-kernel sampler, 9.3).

  python tools/sampler_bench.py [--rows 4,16] [--iters 200] [--rounds 3] [--baseline-lib path/libvitron_hip.so] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vitron_amd import _lib, ops  # noqa: E402
from vitron_amd.sampling import allow_mask, pack_sample_rows, pack_trunc_rows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="1,4,16")
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--baseline-lib", default=None)
ap.add_argument("--json", default=None)
args = ap.parse_args()

_lib.load()
dev = torch.device("cuda:0")
V, T, P, SEED, STEP, HIST = 32000, 0.2, 0.7, 1, 2, 2048
base = base_ops = None
if args.baseline_lib:
    base = C.CDLL(os.path.abspath(args.baseline_lib))
    base.vt_argmax.argtypes = _lib.SIGNATURES["vt_argmax"][1]
    base.vt_sample_top_p.argtypes = _lib.SIGNATURES["vt_sample_top_p"][1]
    for name in ("vt_sample_rows", "vt_sample_rows_allow", "vt_sample_rows_adj", "vt_sample_rows_trunc", "vt_sample_rows_wm"):
        getattr(base, name).argtypes = _lib.SIGNATURES[name][1]
    pkg_dir = os.path.dirname(os.path.abspath(args.baseline_lib))
    if os.path.exists(os.path.join(pkg_dir, "ops.py")):       # the library sits in its package: that package's Python path beside this one's
        import importlib.util
        spec = importlib.util.spec_from_file_location("vitron_amd_baseline", os.path.join(pkg_dir, "__init__.py"),
                                                      submodule_search_locations=[pkg_dir])
        sys.modules["vitron_amd_baseline"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules["vitron_amd_baseline"])
        base_ops = importlib.import_module("vitron_amd_baseline.ops")


def wm_depth30(rows):
    """The vt_wm_row array of tools/wm_bench.py's "wm depth 30" arm (ngram_len 5, a 65536-entry table, a history of 1024; even rows fresh,
    odd rows repeated) and the function that puts its cells back, so that every launch does the same work"""
    from vitron_amd.watermark import SynthIDWatermark, pack_wm_rows
    wm = SynthIDWatermark(dict(ngram_len=5, keys=[654, 400, 836, 123, 340, 443, 597, 160, 57, 29, 590, 639, 13, 715, 468, 990, 966, 226, 324, 585,
                                                  118, 504, 421, 521, 129, 669, 732, 225, 90, 960]))
    cells = torch.zeros((rows, wm.cell_words), dtype=torch.int64, device=dev)
    snap = np.zeros((rows, wm.cell_words), dtype=np.uint64)
    snap[1::2, 12] = wm.context_hash(np.zeros((4,), np.int64))
    snap = torch.from_numpy(snap.view(np.int64)).to(dev)
    return pack_wm_rows([(wm, cells[r]) for r in range(rows)], dev), lambda wm=wm: cells.copy_(snap)      # (wm: its device tables stay alive)


def time_us(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.iters * 1e3


result = {"V": V, "iters": args.iters, "rounds": args.rounds, "temperature": T, "top_p": P, "history_ids": HIST, "penalty": 1.3,
          "baseline_lib": bool(base), "device": torch.cuda.get_device_name(0), "shapes": {}, "ab": {}}
for rows in [int(r) for r in args.rows.split(",")]:
    lg = torch.randn((rows, V), device=dev) * 3
    out = torch.empty((rows,), dtype=torch.int32, device=dev)
    hist = torch.randint(0, V, (rows, HIST), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def params(kind, with_hist):
        rs = []
        for r in range(rows):
            greedy = kind == "greedy" or (kind == "mixed" and r % 2 == 0)
            rs.append((0.0 if greedy else T, 0, P, 1.3 if with_hist else 1.0, SEED, STEP, r,
                       hist[r].data_ptr() if with_hist else 0, HIST if with_hist else 0))
        return pack_sample_rows(rs, dev)

    arms = {"argmax": lambda: ops.argmax(lg), "top_p 0.7": lambda: ops.sample_top_p(lg, T, P, SEED, STEP),
            "top_p 1.0": lambda: ops.sample_top_p(lg, 1.0, 1.0, SEED, STEP)}
    if base is not None:
        arms["baseline argmax"] = lambda: base.vt_argmax(lg.data_ptr(), rows, V, V, out.data_ptr(), stream)
        arms["baseline top_p 0.7"] = lambda: base.vt_sample_top_p(lg.data_ptr(), rows, V, V, T, 0, P, SEED, STEP, out.data_ptr(), None, stream)
    for kind in ("sampled", "greedy", "mixed"):
        for with_hist in (False, True):
            pr = params(kind, with_hist)
            arms[f"rows {kind}" + (" +hist" if with_hist else "")] = lambda pr=pr: ops.sample_rows(lg, pr)
    pr_s = params("sampled", False)
    if base is not None:
        arms["baseline rows sampled"] = lambda: base.vt_sample_rows(lg.data_ptr(), rows, V, V, pr_s.data_ptr(), out.data_ptr(), None, None, stream)
    g = np.random.default_rng(rows)
    host_masks = [allow_mask(V, np.flatnonzero(g.random(V) < 0.5)) for _ in range(rows)]
    masks = [torch.from_numpy(m.view(np.int32)).to(dev) for m in host_masks]
    for label, lst in (("allow all rows", masks), ("allow half rows", [m if r % 2 else None for r, m in enumerate(masks)])):
        ptrs = ops.allow_pointers(lst, rows, V, dev)
        arms[f"rows sampled {label}"] = lambda ptrs=ptrs: ops.sample_rows(lg, pr_s, _allow_ptrs=ptrs)
        arms[f"rows sampled {label} +ptrs"] = lambda lst=lst: ops.sample_rows(lg, pr_s, allow=lst)
    half_ids = np.flatnonzero(g.random(V) < 0.5)
    arms["step mask upload (16000 ids)"] = lambda: torch.from_numpy(allow_mask(V, half_ids).view(np.int32)).to(dev)
    arms["step mask upload (8 ids)"] = lambda: torch.from_numpy(allow_mask(V, [5, 31, 32, 1023, 1024, 7777, 20000, V - 1]).view(np.int32)).to(dev)
    lib = _lib.load()
    if base is not None:      # the same parent launch a second time: the spread of repeated parent runs, measured in this run
        arms["baseline rows sampled (again)"] = arms["baseline rows sampled"]
        # one arm per flavour of the vt_sample_rows kernel, this library against the baseline through raw ctypes on the same device arrays
        zero_adj = torch.zeros((V, 2), device=dev)
        all_ptrs, adj_ptrs = ops.allow_pointers(masks, rows, V, dev), ops.adjust_pointers([zero_adj] * rows, rows, V, dev)
        tr4 = pack_trunc_rows([(0.1, 0.9, 1e-3, 1e-3)] * rows, dev)
        wm_rows, wm_restore = wm_depth30(rows)
        flavours = {"rows sampled": ("vt_sample_rows", ()), "allow all rows": ("vt_sample_rows_allow", (all_ptrs,)), "adj zero": ("vt_sample_rows_adj", (None, adj_ptrs)),
                    "trunc all four": ("vt_sample_rows_trunc", (None, None, tr4)), "wm depth 30": ("vt_sample_rows_wm", (None, None, None, wm_rows))}
        for label, (entry, arrays) in flavours.items():
            call = (lg.data_ptr(), rows, V, V, pr_s.data_ptr(), *(a if a is None else a.data_ptr() for a in arrays), out.data_ptr(), None, None,
                    stream)
            before = wm_restore if entry == "vt_sample_rows_wm" else (lambda: None)      # every wm launch starts from the same cells
            for who, l in (("new", lib), ("baseline", base)):
                arms[f"{who} raw {label}"] = lambda fn=getattr(l, entry), call=call, before=before: (before(), fn(*call))
        if base_ops is not None:      # ... and the Python path in front of them, this package's against the baseline's
            for label, kw in (("rows sampled", {}), ("allow all rows", dict(_allow_ptrs=all_ptrs)), ("allow all rows +ptrs", dict(allow=masks)),
                              ("adj zero +ptrs", dict(adjust=[zero_adj] * rows)), ("trunc all four", dict(trunc=tr4))):
                for who, o in (("new", ops), ("baseline", base_ops)):
                    arms[f"{who} ops {label}"] = lambda o=o, kw=kw: o.sample_rows(lg, pr_s, **kw)
    arms["trunc entry, trunc=NULL"] = lambda: lib.vt_sample_rows_trunc(lg.data_ptr(), rows, V, V, pr_s.data_ptr(), None, None, None,
                                                                       out.data_ptr(), None, None, stream)
    # Mirostat beside the truncation launch on the same rows; the cells are put back in front of every launch of the four arms
    from vitron_amd.sampling import pack_miro_rows
    miro_cells = torch.tensor([[10.0, 0.0]] * rows, dtype=torch.float32).to(dev)
    miro_snap = miro_cells.clone()
    miro_rows = pack_miro_rows([(miro_cells[r], 5.0, 0.1) for r in range(rows)], dev)
    tr_off, tr_all = pack_trunc_rows([None] * rows, dev), pack_trunc_rows([(0.1, 0.9, 1e-3, 1e-3)] * rows, dev)
    head = (lg.data_ptr(), rows, V, V, pr_s.data_ptr(), None, None)
    tail = (out.data_ptr(), None, None, stream)
    for label, tr in (("all inactive", tr_off), ("all four", tr_all)):
        arms[f"trunc {label} +restore"] = lambda tr=tr: (miro_cells.copy_(miro_snap), lib.vt_sample_rows_trunc(*head, tr.data_ptr(), *tail))
    arms["miro tau 5"] = lambda: (miro_cells.copy_(miro_snap), lib.vt_sample_rows_miro(*head, None, miro_rows.data_ptr(), *tail))
    arms["miro tau 5 + all four"] = lambda: (miro_cells.copy_(miro_snap),
                                             lib.vt_sample_rows_miro(*head, tr_all.data_ptr(), miro_rows.data_ptr(), *tail))
    miro_null = pack_miro_rows([None] * rows, dev)
    arms["miro cells NULL"] = lambda: (miro_cells.copy_(miro_snap), lib.vt_sample_rows_miro(*head, None, miro_null.data_ptr(), *tail))
    arms["miro entry, miro=NULL"] = lambda: lib.vt_sample_rows_miro(*head, tr_all.data_ptr(), None, *tail)
    stages = {"all inactive": None, "min_p 0.1": (0.1, 1.0, 0.0, 0.0), "typical_p 0.9": (0.0, 0.9, 0.0, 0.0),
              "epsilon 1e-3": (0.0, 1.0, 1e-3, 0.0), "eta 1e-3": (0.0, 1.0, 0.0, 1e-3), "all four": (0.1, 0.9, 1e-3, 1e-3)}
    for label, t in stages.items():
        tr = pack_trunc_rows([t] * rows, dev)
        arms[f"trunc {label}"] = lambda tr=tr: ops.sample_rows(lg, pr_s, trunc=tr)
    from transformers.generation import logits_process as LP
    chain = [LP.TemperatureLogitsWarper(T), LP.TopPLogitsWarper(top_p=P), LP.MinPLogitsWarper(min_p=0.1), LP.TypicalLogitsWarper(mass=0.9),
             LP.EpsilonLogitsWarper(epsilon=1e-3), LP.EtaLogitsWarper(epsilon=1e-3, device="cpu")]

    def host_warpers():
        x = lg.cpu()
        for w in chain:
            x = w(None, x)
        return torch.multinomial(torch.softmax(x, -1), 1).to(dev)
    arms["host warpers (read-back + all four)"] = host_warpers
    pr_lp = params("sampled", False)
    arms["rows sampled +logprob"] = lambda: ops.sample_rows(lg, pr_lp, return_logprob=True)
    assert torch.equal(ops.sample_rows(lg, params("sampled", False)), ops.sample_top_p(lg, T, P, SEED, STEP))      # the same draw
    times = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name, fn in arms.items():
            times[name].append(time_us(fn))
    shape = {}
    for name, ts in times.items():
        med = statistics.median(ts)
        shape[name] = {"us": [round(t, 2) for t in ts], "median_us": round(med, 2), "spread": round((max(ts) - min(ts)) / med, 4)}
        print(f"rows={rows:2d} {name:36s} {med:8.1f} us   rounds {[f'{t:.1f}' for t in ts]}  spread {shape[name]['spread']:.3f}")
    result["shapes"][f"{rows}x{V}"] = shape
    for a_name, b_name in (("miro tau 5", "trunc all inactive +restore"), ("miro tau 5 + all four", "trunc all four +restore")):
        result.setdefault("miro", {})[f"{rows}x{V} {a_name}"] = {
            "miro_us": shape[a_name]["median_us"], "trunc_us": shape[b_name]["median_us"],
            "added_us": round(shape[a_name]["median_us"] - shape[b_name]["median_us"], 2),
            "cells_null_us": shape["miro cells NULL"]["median_us"]}
        print(f"rows={rows:2d} {a_name:24s} {shape[a_name]['median_us']:8.1f} us beside {b_name} {shape[b_name]['median_us']:8.1f} us")
    # "new X" against "baseline X": apart only beyond the largest of the two spreads and the spread of the repeated parent run
    again = shape.get("baseline rows sampled (again)", {}).get("spread", 0.0)
    for name in [n for n in shape if n.startswith("new ") and "baseline " + n[4:] in shape]:
        new, old = shape[name], shape["baseline " + name[4:]]
        diff, allowed = (new["median_us"] - old["median_us"]) / old["median_us"], max(new["spread"], old["spread"], again)
        result["ab"][f"{rows}x{V} {name[4:]}"] = {"new_us": new["median_us"], "baseline_us": old["median_us"], "diff": round(diff, 4),
                                                  "allowed": allowed, "apart": abs(diff) > allowed}
        print(f"rows={rows:2d} A/B {name[4:]:28s} new {new['median_us']:8.1f} baseline {old['median_us']:8.1f}  diff {diff:+.3f}  allowed "
              f"{allowed:.3f}  {'APART' if abs(diff) > allowed else 'same'}")
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
