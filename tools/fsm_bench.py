"""Times guided decoding by token automata, bf16, one MI355X:
  1. vt_fsm_rows through ops.fsm_rows at 4 and 16 rows x V = 32000, every row one generated id behind its cell's state: on a trie state
     with 8 edges (the mask starts from zeros) and on a default-edge state with 8 exceptions (it starts from ones); beside them, as the
     yardstick of the same run, vt_ban_rows as tools/ban_bench.py times it (g = 3, eight 3-token sequences, a history of 640 ids)
  2. ms per ServingEngine decode step at the 7B width with 4 and 16 requests held to the same choices: through
     SamplingParams(choices=) (the host trie, one mask upload per row and step) and through SamplingParams(automaton=from_choices)
The arms alternate inside every round of one process; medians of --rounds rounds with the rounds shown. One JSON line per arm; --json
PATH also writes them to a file (profiles/fsm_bench.json). Reported, not gating."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vitron_amd import _lib, ops, synth  # noqa: E402
from vitron_amd.automaton import TokenAutomaton  # noqa: E402
from vitron_amd.model import LlavaConfig, LlavaLlamaForCausalLM  # noqa: E402
from vitron_amd.sampling import SamplingParams, flatten_ban_seqs, mask_words, pack_ban_rows, pack_fsm_rows  # noqa: E402
from vitron_amd.serving import ServingEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--prompt", type=int, default=64)
ap.add_argument("--steps", type=int, default=48)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--json", default=None)
ap.add_argument("--no-engine", action="store_true", help="part 1 only")
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
V, G, EOS = 32000, 3, 2

# ---- 1: vt_fsm_rows alone, beside vt_ban_rows ----------------------------------------------------------------------------------------------------
EIGHT = [1000 + 37 * i for i in range(8)]
# state 0 --(8 listed ids)--> state 1 (a trie node: 8 edges back to 0, no default); state 2 <--> state 3 (free text: a default edge, 8 forbidden ids)
A = TokenAutomaton.from_states([{t: 1 for t in EIGHT}, {t: 0 for t in EIGHT}, {t: -1 for t in EIGHT}, {t: -1 for t in EIGHT}],
                               [-1, -1, 3, 2], [0, 0, 1, 1])
seqs = torch.from_numpy(flatten_ban_seqs([[100 + 3 * i, 101 + 3 * i, 102 + 3 * i] for i in range(8)])).to(dev)
kernel = {}
for ROWS in (4, 16):
    work = torch.empty((ROWS, mask_words(V)), dtype=torch.int32, device=dev)
    hist = torch.randint(3, V, (ROWS, 640), generator=gen, device=dev).to(torch.int32)
    ban = pack_ban_rows([(hist[b].data_ptr(), 640, 0, work[b].data_ptr(), G, seqs.data_ptr(), 8, int(seqs.numel())) for b in range(ROWS)], dev)
    packs = {}
    for name, start, tok in (("fsm_rows trie state, 8 edges", 0, EIGHT[3]), ("fsm_rows default edge, 8 exceptions", 2, 7)):
        cells = torch.tensor([[start, 0]] * ROWS, dtype=torch.int32, device=dev)
        one = torch.tensor([tok], dtype=torch.int32, device=dev)
        # the steady state of a decode loop is timed: after the first launch consumed == gen_len == 1 and the cell holds the state reached
        # (the trie node / the free-text state); the advance is one thread's few loads, the mask build is the work
        rows = pack_fsm_rows([(one.data_ptr(), 1, cells[b].data_ptr(), 0, work[b].data_ptr(), *A.row_fields(dev), [EOS]) for b in range(ROWS)], dev)
        packs[name] = (rows, cells, one)
    arms = {name: (lambda rows=p[0], n=ROWS: ops.fsm_rows(rows, n, V)) for name, p in packs.items()}
    arms["ban_rows"] = lambda ban=ban, n=ROWS: ops.ban_rows(ban, n, V)
    us = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name, fn in arms.items():
            us[name].append(events(fn, args.iters))
    for name in arms:
        note(arm=name, rows=ROWS, V=V, us=median(us[name]), us_rounds=us[name])
    kernel[ROWS] = {name: median(v) for name, v in us.items()}
note(arm="summary kernels", us={str(r): kernel[r] for r in kernel},
     fsm_over_ban={str(r): {n: kernel[r][n] / kernel[r]["ban_rows"] for n in kernel[r] if n != "ban_rows"} for r in kernel})

# ---- 2: an engine decode step with the same choices through the host path and as an automaton ------------------------------------------------------
if not args.no_engine:
    model = LlavaLlamaForCausalLM(LlavaConfig(**synth.VICUNA_7B, mm_hidden_size=1024))
    model.init_synthetic(dev, seed=1234)
    model.config.kv_prefix_reuse = False
    ids = torch.cat([torch.tensor([1], device=dev), torch.randint(3, V, (args.prompt - 1,), generator=gen, device=dev)]).unsqueeze(0)
    steps = args.steps
    # the main path is the greedy run held to eight ids; every node of it has those eight ids as children, seven of them leaves: under the
    # trie the model picks the main path again, so a request runs `steps` tokens through nodes with 8 edges each
    main = model.generate(ids, do_sample=False, allowed_token_ids=EIGHT, max_new_tokens=steps, eos_token_id=-1, pad_token_id=0)[0, args.prompt:].tolist()
    choices = [main] + [main[:d] + [s] for d in range(steps) for s in EIGHT if s != main[d]]
    auto = TokenAutomaton.from_choices(choices)
    arms = {"choices (host trie, upload per step)": lambda: SamplingParams(choices=choices),
            "automaton (vt_fsm_rows)": lambda: SamplingParams(automaton=auto)}
    per_arm = {}
    for ROWS in (4, 16):
        times = {name: [] for name in arms}
        uploads = {}
        for rnd in range(args.rounds + 1):                  # round 0 warms up
            for name, sp in arms.items():
                eng = ServingEngine(model, max_batch=ROWS, kv_pages=4 * ROWS + 8)
                rids = [eng.submit(ids, None, None, steps, eos_token_id=EOS, sampling=sp()) for _ in range(ROWS)]
                eng.step()                                   # admission and prefill
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = 0
                while eng.pending():
                    eng.step()
                    n += 1
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                assert not eng.failed and all(eng.finished[r].tokens == main for r in rids), "the request left the main path"
                uploads[name] = eng.finished[rids[0]].mask_uploads
                if rnd:
                    times[name].append(dt / n)
        for name in arms:
            per_arm[(ROWS, name)] = median(times[name])
            note(arm=f"engine step, {name}", rows=ROWS, steps=steps, ms_per_step=median(times[name]), ms_per_step_rounds=times[name],
                 mask_uploads_per_request=uploads[name])
    note(arm="summary engine", host_minus_automaton_us_per_step={
        str(r): (per_arm[(r, "choices (host trie, upload per step)")] - per_arm[(r, "automaton (vt_fsm_rows)")]) * 1e3 for r in (4, 16)})

if args.json:
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
