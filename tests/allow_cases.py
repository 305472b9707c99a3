"""Inputs and call helpers shared by tests/test_gpu_sample_allow.py and tests/test_gpu_constrained_requests.py: the fixed fp32 logits
rows, the packing of one vt_sample_row tuple per row, and a request's solo generate() / its submission to a ServingEngine. Stated here
on their own so that the two files do not depend on the internals of other test modules."""
import torch

ROWS = 8
VS = (32000, 32003, 40000)          # rows in registers; odd stride: the ragged tail, the streaming form; the streaming form, aligned

_cache = {}


def logits(V):
    """fp32 [8][V] on the host, computed once per V and never modified: both signs, a zero, ties, one dominant and one near-uniform row"""
    if V not in _cache:
        g = torch.Generator().manual_seed(1000 + V)
        x = torch.randn((ROWS, V), generator=g) * 3.0
        x[0, 123] = 40.0                                   # dominant: logprob near 0, keep-set of one
        x[1] = torch.randn((V,), generator=g) * 1e-3       # near uniform
        x[2, 777] = x[2, V - 1] = 50.0                     # tie for the maximum: the first index wins
        x[2, 100] = 20.0
        x[3] = x[3].round()                                # ties everywhere
        x[:, 5] = 0.0
        x[4, 0], x[4, 31], x[4, 32], x[4, V - 1] = 13.0, -13.0, 14.0, 15.0      # the mask's word boundaries carry the row's extremes
        _cache[V] = x
    return _cache[V]


def pack(rows, dev):
    from vitron_amd.sampling import pack_sample_rows
    return pack_sample_rows(rows, dev)


def row(T=0.0, k=0, p=1.0, pen=1.0, seed=0, counter=0, stream=0, hist=None, hlen=None):
    """(temperature, top_k, top_p, penalty, seed, counter, stream, history pointer, history length) of sampling.sample_rows_array"""
    return (T, k, p, pen, seed, counter, stream, 0 if hist is None else hist.data_ptr(), 0 if hist is None else (hist.numel() if hlen is None else hlen))


def solo(model, dev, r, sp, **kw):
    """The new tokens of request r through generate() alone, with SamplingParams sp's temperature / top_p / top_k / seed / penalty"""
    o = model.generate(r["input_ids"].to(dev), images=r["images"], regions=r["regions"], do_sample=sp.temperature > 0,
                       temperature=sp.temperature if sp.temperature > 0 else 1.0, top_p=sp.top_p, top_k=sp.top_k, seed=sp.seed,
                       repetition_penalty=sp.repetition_penalty, max_new_tokens=r["max_new_tokens"], eos_token_id=-1, **kw)
    return o[0, r["input_ids"].shape[1]:].cpu().tolist()


def submit(eng, r, sp=None):
    return eng.submit(r["input_ids"], r["images"], r["regions"], r["max_new_tokens"], eos_token_id=-1, sampling=sp)


def tiny_model(dev):
    """The tiny synthetic multimodal model of the golden cases (2 decoder layers, V = 512), kv_prefix_reuse off"""
    from tests.golden import cases
    from vitron_amd import synth
    from vitron_amd.model import LlavaConfig, LlavaLlamaForCausalLM
    st = {
        "image_tower": synth.vit_state(cases.VIT_IMAGE, synth.make_generator(cases.SEED_VIT), **cases.VIT_INIT),
        "video_tower": synth.vit_state(cases.VIT_VIDEO, synth.make_generator(cases.SEED_VIT), **cases.VIT_INIT),
        "projector": synth.projector_state(cases.MM_HIDDEN, cases.LLM["hidden_size"], synth.make_generator(cases.SEED_PROJ), **cases.MLP_INIT),
        "region": synth.region_state(cases.MM_HIDDEN, cases.LLM["hidden_size"], synth.make_generator(cases.SEED_REGION), **cases.MLP_INIT),
        "llama": synth.llama_state(cases.LLM, synth.make_generator(cases.SEED_LLM), **cases.LLM_INIT),
    }
    cfg = LlavaConfig(**cases.LLM, mm_hidden_size=cases.MM_HIDDEN, mm_image_tower="golden/LanguageBind_Image",
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
