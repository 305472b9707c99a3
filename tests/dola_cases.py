"""The tiny synthetic multimodal model of tests/allow_cases.tiny_model with EIGHT decoder layers (dola_layers "low" = [0, 2], "high" =
[4, 6]) for tests/test_gpu_dola_requests.py, and the loop generate(dola_layers=) is held to, driven from the test: llama_forward with
the logit-row trace, ops.gemm over the candidate rows, ops.dola_rows in place, a pick."""
import math

import torch

LAYERS = 8


def tiny_model8(dev):
    from tests.golden import cases
    from vitron_amd import synth
    from vitron_amd.model import LlavaConfig, LlavaLlamaForCausalLM
    llm = dict(cases.LLM, num_hidden_layers=LAYERS)
    st = {
        "image_tower": synth.vit_state(cases.VIT_IMAGE, synth.make_generator(cases.SEED_VIT), **cases.VIT_INIT),
        "video_tower": synth.vit_state(cases.VIT_VIDEO, synth.make_generator(cases.SEED_VIT), **cases.VIT_INIT),
        "projector": synth.projector_state(cases.MM_HIDDEN, llm["hidden_size"], synth.make_generator(cases.SEED_PROJ), **cases.MLP_INIT),
        "region": synth.region_state(cases.MM_HIDDEN, llm["hidden_size"], synth.make_generator(cases.SEED_REGION), **cases.MLP_INIT),
        "llama": synth.llama_state(llm, synth.make_generator(cases.SEED_LLM), **cases.LLM_INIT),
    }
    cfg = LlavaConfig(**llm, mm_hidden_size=cases.MM_HIDDEN, mm_image_tower="golden/LanguageBind_Image",
                      mm_video_tower="golden/LanguageBind_Video_merge", kv_prefix_reuse=False)
    m = LlavaLlamaForCausalLM(cfg)
    m.get_image_tower().load_state(cases.VIT_IMAGE, st["image_tower"])
    m.get_video_tower().load_state(cases.VIT_VIDEO, st["video_tower"])
    sd = dict(st["llama"])
    sd.update({"model.mm_projector." + k: v for k, v in st["projector"].items()})
    sd.update({"model.region_extractor." + k: v for k, v in st["region"].items()})
    m.load_state_dict(sd)
    m = m.to(dev)
    m.config.kv_prefix_reuse = False
    return m


def drive(model, dev, ids, images, attention_mask, layers, n_new, relative_top=0.1, pick=None):
    """Prompts embedded and prefilled as generate() does it (one packed pass, with the trace of `layers` at the last rows); per step the
    candidate rows gathered candidate-major, the bare lm_head over them in launches of at most 16 rows, ONE ops.dola_rows launch in place
    over the final rows (which also writes every row's mask and choice), then `pick(step, contrasted rows, masks)` (ops.argmax by
    default) and a decode pass of B rows through llama_forward with the trace. Returns (ids per sample, chosen layer per sample and
    step, every step's contrasted rows on the host, every step's final rows on the host)."""
    from vitron_amd import ops
    from vitron_amd.engine import SequenceState, llama_forward
    from vitron_amd.sampling import mask_words, pack_dola_rows
    B = ids.shape[0]
    llama = model.model.llama
    emb, mh, _ = model._embed_prompt(ids, attention_mask, images, None, use_vis_cache=False)
    flat, flat_lo, lens, _ = model._pack_rows(emb, mh)
    model._ensure_kv(sum((n + n_new + 63) // 64 + 1 for n in lens))
    seqs = [SequenceState() for _ in range(B)]
    n_cand = len(layers)
    idx = torch.tensor([l * B + b for l in layers for b in range(B)], dtype=torch.long, device=dev)
    prem = torch.empty((n_cand, B, llama.V_pad), dtype=torch.float32, device=dev)
    masks = torch.empty((B, mask_words(llama.V)), dtype=torch.int32, device=dev)
    choice = torch.empty((B,), dtype=torch.int32, device=dev)
    toks, chosen, rows_out, finals = [], [], [], []
    try:
        f, trace = llama_forward(llama, model.kv, seqs, flat, lens, embeds_lo=flat_lo, trace_rows_layers=layers)
        for st in range(n_new):
            finals.append(f.float().cpu().numpy().copy())
            cand = trace.view(-1, llama.H).index_select(0, idx)
            flat_p = prem.view(-1, llama.V_pad)
            for r0 in range(0, cand.shape[0], 16):
                ops.gemm(cand[r0:r0 + 16], llama.lm_head, None, ops.EPI_F32, out=flat_p[r0:r0 + 16])
            desc = pack_dola_rows([(f[b].data_ptr(), prem[0, b].data_ptr(), prem.stride(0), n_cand, f[b].data_ptr(), 0, masks[b].data_ptr(),
                                    choice[b:b + 1].data_ptr(), 0, 0, math.log(relative_top)) for b in range(B)], dev)
            ops.dola_rows(desc, B, llama.V)
            rows_out.append(f.float().cpu().numpy().copy())
            chosen.append([layers[j] for j in choice.cpu().tolist()])
            nxt = ops.argmax(f) if pick is None else pick(st, f, masks)
            toks.append(nxt.cpu().tolist())
            if st + 1 < n_new:
                f, trace = llama_forward(llama, model.kv, seqs, llama.embed[nxt.long()], [1] * B, trace_rows_layers=layers)
    finally:
        for s in seqs:
            model.kv.release(s.pages)
    return [[t[b] for t in toks] for b in range(B)], [[c[b] for c in chosen] for b in range(B)], rows_out, finals
