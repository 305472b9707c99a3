"""The seeded inputs of the vt_contrast_rows tests, shared by tests/test_contrast_ref_host.py (which proves that every random case has a
selection gap the kernel's error bounds cannot close) and tests/test_gpu_contrast_rows.py (which therefore demands the exact selection on
all of them), and the tiny synthetic model of the request tests in either operand format."""
import numpy as np
import torch

DTYPES = [torch.bfloat16, torch.float16]
GAP_FACTOR = 4.0                 # the fp64 gap between the two best scores exceeds GAP_FACTOR x the sum of their error bounds

# one launch each: H and the groups (T = bank_len, k, alpha) that share it -- different T and k in one launch, T below / at / above the
# kernel's 16-row chunk, k at both ends of [1, 16], alpha at 1 (the probabilities drop out)
LAUNCHES = [
    dict(H=256, seed=4107, groups=[(1, 1, 0.6), (17, 2, 0.6), (130, 3, 0.5), (257, 16, 0.7), (300, 15, 0.9), (16, 4, 0.25)]),
    dict(H=4096, seed=4211, groups=[(65, 4, 0.6), (333, 16, 0.6), (15, 2, 1.0)]),
]

_made = {}


def _unit(x):
    return x / np.sqrt((x * x).sum(-1, keepdims=True))


def launch_case(i: int, dtype):
    """Launch i in `dtype`: a list of groups, each a dict with bank fp32 [T, H] and cand fp32 [k, H] (unit rows ROUNDED to dtype, held in
    fp32), lp fp32 [k] (descending log-probabilities, as vt_logprob_rows orders them), T, k, alpha. A candidate leans on one bank row with
    a cosine drawn from [0.1, 0.95] -- the spread real hidden states show -- and is random otherwise. Computed once, never modified."""
    key = (i, dtype)
    if key not in _made:
        spec = LAUNCHES[i]
        rng = np.random.default_rng(spec["seed"])
        H = spec["H"]
        groups = []
        for T, k, alpha in spec["groups"]:
            bank = _unit(rng.standard_normal((T, H)))
            beta = rng.uniform(0.1, 0.95, size=(k, 1))
            lean = bank[rng.integers(0, T, size=k)]
            noise = _unit(rng.standard_normal((k, H)))
            cand = _unit(beta * lean + np.sqrt(1.0 - beta * beta) * noise)
            p = np.sort(rng.dirichlet(np.ones(k + 3))[:k] * 0.9)[::-1]
            groups.append(dict(T=T, k=k, alpha=alpha,
                               bank=torch.from_numpy(bank).float().to(dtype).float().numpy(),
                               cand=torch.from_numpy(cand).float().to(dtype).float().numpy(),
                               lp=np.log(p).astype(np.float32)))
        _made[key] = groups
    return _made[key]


def tiny_model(dev, dtype=torch.bfloat16):
    """tests/allow_cases.tiny_model (2 decoder layers, V = 512, both towers and the region extractor, kv_prefix_reuse off) packed in `dtype`"""
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
    m = m.to(dtype=dtype).to(dev)
    m.config.kv_prefix_reuse = False
    return m
