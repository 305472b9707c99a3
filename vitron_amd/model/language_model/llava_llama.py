"""LlavaLlamaForCausalLM on HIP kernels -- mirror of the reference's vitron/model/language_model/llava_llama.py.

Same class names (LlavaConfig, LlavaLlamaModel, LlavaLlamaForCausalLM) and the same forward / generate /
prepare_inputs_for_generation signatures (llava_llama.py:57-114), so app.py:562-571 and
inference_image.py:53-61 call it unchanged. The decoder itself (transformers-4.31 LlamaForCausalLM in the
reference) is vt_llama_forward: one C call per pass over a paged KV cache; `generate` is a greedy / top-p loop on
top of it (the reference gets its loop from GenerationMixin).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Optional

import torch

from ... import _lib, ops, synth
from ...engine import DecodeState, PackedLlama, PagedKVCache, SequenceState, llama_forward, pair_lo, parse_kv_cache_dtype
from ..llava_arch import LlavaMetaForCausalLM, LlavaMetaModel
from ..multimodal_encoder.builder import build_image_tower, build_video_tower
from ..multimodal_projector.builder import build_vision_projector
from ..region_extractor.builder import build_region_extractor


def _resolve_dtype(x, strict=True):
    """torch dtype for a `torch_dtype` entry ('float16' / 'bfloat16' strings as in a HF config.json, torch dtypes,
    'fp16' / 'bf16'); None stays None (= the package default). strict=False (a value READ FROM A CHECKPOINT's config.json): anything
    that is not one of the two operand formats -- "float32", unknown strings -- is treated as None instead of raising: the reference
    ignores the stored value and forces fp16 (builder.py:47), so a checkpoint saved with "torch_dtype": "float32" must still load."""
    if x is None:
        return None
    if isinstance(x, str):
        x = {"float16": torch.float16, "half": torch.float16, "fp16": torch.float16,
             "bfloat16": torch.bfloat16, "bf16": torch.bfloat16}.get(x.replace("torch.", ""), x)
    if not strict and x not in (torch.float16, torch.bfloat16):
        return None
    _lib.operand_of(x)
    return x


class LlavaConfig(SimpleNamespace):
    """LlamaConfig fields + the mm_* fields the reference reads (llava_arch.py:33-40,363,379)."""
    model_type = "llava"

    def __init__(self, **kw):
        base = dict(hidden_size=4096, intermediate_size=11008, num_hidden_layers=32, num_attention_heads=32,
                    vocab_size=32000, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=4096,
                    bos_token_id=1, eos_token_id=2, pad_token_id=0, mm_image_tower=None, mm_video_tower=None,
                    mm_projector_type="mlp2x_gelu", mm_vision_select_layer=-2, mm_vision_select_feature="patch",
                    mm_hidden_size=1024, tokenizer_model_max_length=None, tokenizer_padding_side="right",
                    pretraining_tp=1, use_cache=True)
        base.update(kw)
        super().__init__(**base)

    def to_dict(self):
        return dict(self.__dict__)


class CausalLMOutputWithPast(SimpleNamespace):
    def __getitem__(self, i):
        return [v for v in (self.loss, self.logits, self.past_key_values) if v is not None][i]


class PagedPast:
    """past_key_values of this implementation: per-sequence page lists in the model's paged KV pool."""

    def __init__(self, kv: PagedKVCache, seqs: List[SequenceState], padded_len: int):
        self.kv, self.seqs, self.padded_len = kv, seqs, padded_len

    def seq_length(self) -> int:  # what the reference reads as past_key_values[-1][-1].shape[-2] (llava_arch.py:198)
        return self.padded_len

    def release(self):
        for s in self.seqs:
            self.kv.release(s.pages)
            s.pages = []


class LlavaLlamaModel(LlavaMetaModel):
    """reference llava_llama.py:33-37 + LlavaMetaModel.__init__ (llava_arch.py:30-40)."""

    def __init__(self, config: LlavaConfig):
        self.config = config
        self.llama: Optional[PackedLlama] = None
        if getattr(config, "mm_image_tower", None) is not None:
            self.image_tower = build_image_tower(config, delay_load=True)
        if getattr(config, "mm_video_tower", None) is not None:
            self.video_tower = build_video_tower(config, delay_load=True)
        if getattr(config, "mm_image_tower", None) is not None or getattr(config, "mm_video_tower", None) is not None:
            self.mm_projector = build_vision_projector(config)
            self.region_extractor = build_region_extractor(config)

    @property
    def embed_tokens_weight(self) -> torch.Tensor:
        return self.llama.embed

    def embed_tokens(self, ids: torch.Tensor) -> torch.Tensor:
        """nn.Embedding forward. Like the reference's, an id outside the table is an error (IndexError), checked on a host
        copy of the ids (prompts only: the decode loop feeds tokens through vt_decode_feed, which cannot leave the table)."""
        host = ids.detach().reshape(-1).cpu()
        if host.numel() and (int(host.min()) < 0 or int(host.max()) >= self.llama.embed_rows):
            bad = int(host.min()) if int(host.min()) < 0 else int(host.max())
            raise IndexError(f"embed_tokens: token id {bad} outside the embedding table ({self.llama.embed_rows} rows)")
        flat = ids.reshape(-1).to(device=self.llama.device, dtype=torch.int32)
        plan = torch.stack([torch.zeros_like(flat), flat], dim=1).contiguous()
        return ops.embed_splice(self.llama.embed, None, None, plan).view(*ids.shape, -1)


class _DolaHead:
    """The candidate rows of a DoLa call: `trace` is the operand-dtype [L, B, H] buffer a decoder pass writes the
    candidate layers' streams into (vt_llama_model.logit_row_trace); head(out) gathers the n_cand * B candidate rows (candidate-major)
    and runs the bare lm_head over them into out, fp32 [n_cand, B, V_pad], in launches of at most 16 rows: the weight-streaming GEMM a
    decode step's lm_head runs. Nothing is allocated per step."""
    ROWS = 16

    def __init__(self, llama, layers, B: int, trace: torch.Tensor):
        self.llama, self.trace = llama, trace
        self.idx = torch.tensor([l * B + b for l in layers for b in range(B)], dtype=torch.long).to(trace.device)
        self.rows = torch.empty((len(layers) * B, llama.H), dtype=trace.dtype, device=trace.device)

    def head(self, out: torch.Tensor) -> torch.Tensor:
        from ... import ops
        torch.index_select(self.trace.view(-1, self.llama.H), 0, self.idx, out=self.rows)
        flat = out.view(-1, out.shape[-1])
        for r0 in range(0, self.rows.shape[0], self.ROWS):
            ops.gemm(self.rows[r0:r0 + self.ROWS], self.llama.lm_head, None, ops.EPI_F32, out=flat[r0:r0 + self.ROWS])
        return out


class LlavaLlamaForCausalLM(LlavaMetaForCausalLM):
    config_class = LlavaConfig

    def __init__(self, config: LlavaConfig):
        self.config = config
        self.model = LlavaLlamaModel(config)
        self.vocab_size = config.vocab_size
        self._device = torch.device("cpu")
        self._llama_sd = None
        # operand dtype of the packed weights and activations: bf16 (package default, BASELINE's dtype) or fp16 (the reference's
        # inference dtype, builder.py:47); set by config.torch_dtype / .to(dtype=...) / .half() before the weights are packed
        # (a config.json value is advisory: unsupported entries fall back to the default; explicit .to(dtype=) / torch_dtype= arguments are validated)
        self._dtype = _resolve_dtype(getattr(config, "torch_dtype", None), strict=False)
        # "16bit", or "nf4" (load_pretrained_model(..., load_4bit=True)): the decoder layers' Linears packed as NF4 (engine.PackedLlama)
        self.weight_format = "16bit"
        self.kv: Optional[PagedKVCache] = None
        self.kv_pages = getattr(config, "kv_pages", None)
        # "16bit" (default) or "fp8": the format of the paged KV pool (config.kv_cache_dtype; engine.PagedKVCache). An opt-in
        # capacity / throughput mode like load_4bit; anything unknown is a ValueError here, at construction
        self.kv_cache_dtype = parse_kv_cache_dtype(getattr(config, "kv_cache_dtype", None))
        # multi-turn reuse (vitron_amd/prefix_cache.py): generate() keeps the last conversation's KV pages and the encoded
        # images; config.kv_prefix_reuse / config.vis_cache_entries switch them off (benchmarks do)
        self._prefix = None
        self._vis_cache = None
        self.last_generate_stats = {}
        self.last_beam_scores = None      # fp32 [B * num_return_sequences]: the hypotheses' scores of the last generate(num_beams > 1)

    # ---- module-like plumbing -----------------------------------------------------------------------------------
    def get_model(self):
        return self.model

    @property
    def device(self):
        return self._device

    @property
    def dtype(self):
        if self.model.llama is not None:
            return self.model.llama.dtype
        return self._dtype or _lib.torch_dtype()

    def half(self):
        return self.to(dtype=torch.float16)

    def bfloat16(self):
        return self.to(dtype=torch.bfloat16)

    def eval(self):
        return self

    def requires_grad_(self, flag=False):
        return self

    def load_state_dict(self, sd, strict=True):
        """Accepts the reference checkpoint naming: LLaMA weights (`model.layers.*`, `model.embed_tokens.weight`,
        `model.norm.weight`, `lm_head.weight`) and the non-LoRA trainables `model.mm_projector.*`,
        `model.region_extractor.*` (reference builder.py:64-79)."""
        proj = {k[len("model.mm_projector."):]: v for k, v in sd.items() if k.startswith("model.mm_projector.")}
        reg = {k[len("model.region_extractor."):]: v for k, v in sd.items() if k.startswith("model.region_extractor.")}
        llm = {k: v for k, v in sd.items() if not k.startswith(("model.mm_projector.", "model.region_extractor.",
                                                                "model.image_tower.", "model.video_tower."))}
        if proj and self.model.mm_projector is not None:
            self.model.mm_projector.load_state_dict(proj, strict)
        if reg and self.model.region_extractor is not None:
            self.model.region_extractor.load_state_dict(reg, strict)
        if llm:
            self._llama_sd = llm
            self.model.llama = None
        self.reset_prefix_cache()        # cached visual tokens / KV pages belong to the previous weights
        return [], []

    def resize_token_embeddings(self, new_num_tokens: Optional[int] = None):
        """PreTrainedModel.resize_token_embeddings as reference builder.py:146 calls it after tokenizer.add_tokens: embed_tokens
        and lm_head get `new_num_tokens` rows (old rows kept, new rows ZERO -- transformers draws them from N(0, 0.02^2); they are
        the untrained <im_patch> / <vi_patch> placeholders that never reach the model, a zero row gives them logit 0), and
        config.vocab_size follows."""
        if new_num_tokens is None:
            return self
        n = int(new_num_tokens)
        sd = self._llama_sd
        if sd is None:
            if self.model.llama is None:
                raise RuntimeError("resize_token_embeddings: load weights first")
            raise RuntimeError("resize_token_embeddings: call it before .to(device) packs the weights (load_pretrained_model does)")
        for key in ("model.embed_tokens.weight", "lm_head.weight"):
            w = sd[key]
            if w.shape[0] == n:
                continue
            out = torch.zeros((n, w.shape[1]), dtype=w.dtype, device=w.device)
            keep = min(n, w.shape[0])
            out[:keep] = w[:keep]
            sd[key] = out
        self.config.vocab_size = n
        self.vocab_size = n
        return self

    def to(self, device=None, dtype=None):
        """nn.Module.to: `dtype` (torch.bfloat16 / torch.float16) is the operand format the weights are packed in when they
        reach the GPU; it cannot change once the decoder is packed (the checkpoint copy is dropped then)."""
        if isinstance(device, torch.dtype):          # .to(torch.float16)
            device, dtype = None, device
        if dtype is not None:
            _lib.operand_of(dtype)
            if self.model.llama is not None and dtype != self.model.llama.dtype:
                raise RuntimeError(f"model weights are already packed as {self.model.llama.dtype}; load the checkpoint again to change the dtype")
            self._dtype = dtype
            for m in (self.model.mm_projector, self.model.region_extractor, self.model.image_tower, self.model.video_tower):
                if m is not None and hasattr(m, "to"):
                    m.to(dtype=dtype)
        if device is None:
            return self
        dev = torch.device(device)
        if dev.type == "cuda":
            if self._llama_sd is not None:
                self.model.llama = PackedLlama(self._llama_sd, self.config.to_dict(), dev, dtype=self._dtype, weight_format=self.weight_format)
                self._llama_sd = None
            for m in (self.model.mm_projector, self.model.region_extractor, self.model.image_tower, self.model.video_tower):
                if m is not None:
                    m.to(dev, dtype=self.dtype) if hasattr(m, "_dtype") else m.to(dev)
        self._device = dev
        return self

    def cuda(self):
        return self.to("cuda")

    def init_synthetic(self, device, seed=1234, vit_image: Optional[dict] = None, vit_video: Optional[dict] = None,
                       w_std=0.02, resize_for=None, dtype=None):
        """Random-init weights of the configured architecture, generated on `device` (no checkpoints exist offline). The
        values are drawn as bf16-representable numbers whatever `dtype` (the operand format they are packed in) is, so a
        bf16 and an fp16 model built from one seed hold the same weights (bf16 -> fp16 is exact above 2^-14)."""
        if dtype is not None:
            self._dtype = _resolve_dtype(dtype)
        gen = synth.make_generator(seed, device)
        cfg = self.config
        self._llama_sd = synth.llama_state(cfg.to_dict(), gen, device, w_std)
        if vit_image is not None:
            self.model.image_tower = build_image_tower(SimpleNamespace(mm_image_tower="synthetic/LanguageBind_Image",
                                                                       mm_vision_select_layer=cfg.mm_vision_select_layer), delay_load=True)
            self.model.image_tower._dtype = self._dtype
            self.model.image_tower.init_synthetic(vit_image, gen, device, w_std)
        if vit_video is not None:
            self.model.video_tower = build_video_tower(SimpleNamespace(mm_video_tower="synthetic/LanguageBind_Video_merge",
                                                                       mm_vision_select_layer=cfg.mm_vision_select_layer), delay_load=True)
            self.model.video_tower._dtype = self._dtype
            self.model.video_tower.init_synthetic(vit_video, gen, device, w_std)
        if self.model.mm_projector is None:
            self.model.mm_projector = build_vision_projector(cfg)
            self.model.region_extractor = build_region_extractor(cfg)
        for m in (self.model.mm_projector, self.model.region_extractor):
            if hasattr(m, "_dtype"):
                m._dtype = self._dtype
        self.model.mm_projector.init_synthetic(gen, device, w_std)
        self.model.region_extractor.init_synthetic(gen, device, w_std)
        if resize_for is not None:            # load_pretrained_model: tokenizer.add_tokens + resize_token_embeddings before packing
            n = resize_for()
            if n is not None:
                self.resize_token_embeddings(n)
        return self.to(device)

    # ---- precision modes -----------------------------------------------------------------------------------------
    def set_precise(self, level: int):
        """0: standard. 1: precise_qk -- prefills carry q / k (and the norm output behind their projection) as hi + lo operand pairs.
        2: a VERIFICATION mode -- every GEMM A operand of a prefill travels as an operand pair, from the towers' MLPs and the projector
        (whose output enters the decoder's fp32 residual stream unrounded) through all decoder GEMMs to the lm_head: about twice the
        GEMM work, and the fp16 build's full-depth logits end below north_star's 1e-3 of the reference's fp32 output (DESIGN.md 4,
        tests/test_gpu_parity_fulldepth.py). Needs the weights on the GPU (call after .to(device)); decode steps are unchanged."""
        level = int(level)
        if level and "fp8" in (self.kv_cache_dtype, parse_kv_cache_dtype(getattr(self.config, "kv_cache_dtype", None))):
            raise RuntimeError(f"set_precise({level}): the precise modes cannot run on the fp8 KV cache (their kernels keep 16-bit operand pairs in "
                               "the pages); call set_kv_cache_dtype('16bit') first")
        llama = self.model.llama
        if llama is None:
            raise RuntimeError("set_precise: move the model to the GPU first (.to(device))")
        llama.set_precise(level)
        self.precise_level = level
        for tower in (self.get_image_tower(), self.get_video_tower()):
            if tower is not None and getattr(tower, "packed", None) is not None and hasattr(tower.packed, "set_precise"):
                tower.packed.set_precise(level)
        return self

    # ---- KV pool ----------------------------------------------------------------------------------------------
    def set_kv_cache_dtype(self, kv_cache_dtype):
        """Format of the paged KV pool: None / 'auto' / '16bit' (default), or 'fp8' / 'fp8_e4m3' -- unscaled OCP e4m3 pages, half the bytes
        per cached token and per decode step's attention (costs e4m3's 3 mantissa bits on K and V). Drops the kept
        conversation and the pool (the next call builds one in the new format); refused while pages are live, and together with the
        precise modes / qkv_fuse, which read or write 16-bit pages."""
        fmt = parse_kv_cache_dtype(kv_cache_dtype)
        llama = self.model.llama
        if fmt == "fp8":
            if int(getattr(self, "precise_level", 0)) or (llama is not None and llama.model.precise_qk):
                raise RuntimeError("set_kv_cache_dtype('fp8'): a precise mode is on, and its kernels keep 16-bit operand pairs in the pages; "
                                   "call set_precise(0) first")
            if llama is not None and llama.model.qkv_fuse:
                raise RuntimeError("set_kv_cache_dtype('fp8'): qkv_fuse is on, and its epilogue writes 16-bit pages; call set_qkv_fuse(False) first")
        self.reset_prefix_cache()
        if self.kv is not None and len(self.kv.free) != self.kv.num_pages:
            raise RuntimeError("set_kv_cache_dtype: KV pages are live; release past_key_values / finish the served requests first")
        self.kv = None
        self.kv_cache_dtype = fmt
        self.config.kv_cache_dtype = None if fmt == "16bit" else fmt
        if llama is not None:
            llama.kv_dtype = fmt
        return self

    def _kv_format(self) -> str:
        """The pool format in force: config.kv_cache_dtype when the caller changed it after construction, else the parsed value."""
        fmt = parse_kv_cache_dtype(getattr(self.config, "kv_cache_dtype", None))
        if fmt != self.kv_cache_dtype:
            self.set_kv_cache_dtype(fmt)
        if self.model.llama is not None:
            self.model.llama.kv_dtype = fmt
        return fmt

    def new_kv_pool(self, num_pages: int) -> PagedKVCache:
        """A pool of `num_pages` pages in the model's KV format (generate()'s own pool and ServingEngine(kv_pages=...) use this)."""
        return PagedKVCache(self.model.llama, int(num_pages), kv_dtype=self._kv_format())

    def reset_prefix_cache(self):
        """Drop the kept conversation (KV pages go back to the pool) and the encoded-image cache."""
        if self._prefix is not None and self.kv is not None:
            self.kv.release(self._prefix.pages)
        self._prefix = None
        if self._vis_cache is not None:
            self._vis_cache.clear()

    def _ensure_kv(self, pages_needed: int):
        if self.kv is not None and self.kv.kv_dtype != self._kv_format():
            raise RuntimeError(f"the KV pool holds {self.kv.kv_dtype} pages but kv_cache_dtype is {self.kv_cache_dtype!r}: use set_kv_cache_dtype()")
        if self.kv is not None and len(self.kv.free) >= pages_needed:
            return
        if self._prefix is not None:            # the kept conversation is the first thing to go when pages run short
            if self.kv is not None:
                self.kv.release(self._prefix.pages)
            self._prefix = None
            if self.kv is not None and len(self.kv.free) >= pages_needed:
                return
        if self.kv is not None and len(self.kv.free) != self.kv.num_pages:
            raise RuntimeError("KV pool exhausted while sequences are live; release past_key_values or raise config.kv_pages")
        n = max(pages_needed, int(self.kv_pages or 0))
        self.kv = None
        self.kv = self.new_kv_pool(n)

    def _pack_rows(self, embeds, mask_host):
        """The valid rows of a padded batch: embeds [B, S, H] and a host 0 / 1 mask [B][S] -> (the rows where the mask is 1 packed as
        [rows, H], their low halves or None, the samples' lengths, the rows' indices in the flattened [B * S] batch). Padding never
        enters the decoder; when there is any, the rows are gathered by the splice kernel (embeds of another float dtype are legal: the
        gather moves rows in the model's operand dtype)."""
        B, S, H = embeds.shape
        lens = [sum(r) for r in mask_host]
        idx = [b * S + j for b in range(B) for j in range(S) if mask_host[b][j]]
        flat = embeds.reshape(B * S, H)
        flat_lo = pair_lo(embeds)                        # precise level 2: the embeddings came out of the splice as an operand pair
        if flat_lo is not None:
            flat_lo = flat_lo.reshape(B * S, H)
        if len(idx) != B * S:
            dtype = self.model.llama.dtype
            rowsel = torch.tensor(idx, dtype=torch.int32, device=flat.device)
            gather = torch.stack([torch.zeros_like(rowsel), rowsel], 1).contiguous()
            flat = ops.embed_splice(flat.to(dtype).contiguous(), None, None, gather)
            if flat_lo is not None:
                flat_lo = ops.embed_splice(flat_lo.to(dtype).contiguous(), None, None, gather)
        return flat, flat_lo, lens, idx

    # ---- reference llava_llama.py:57-102 ----------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None,
                labels=None, use_cache=None, output_attentions=None, output_hidden_states=None, images=None,
                regions=None, return_dict=None):
        splice = None
        if inputs_embeds is None:
            (input_ids, position_ids, attention_mask, past_key_values, inputs_embeds, labels) = \
                self.prepare_inputs_labels_for_multimodal(input_ids, position_ids, attention_mask, past_key_values,
                                                          labels, images, regions)
            splice = getattr(self, "_last_splice", None) if inputs_embeds is not None else None
        llama = self.model.llama
        if inputs_embeds is None:
            inputs_embeds = self.model.embed_tokens(input_ids)
        B, S, H = inputs_embeds.shape
        # valid rows of every sample (padding rows never enter the decoder: the batch is packed)
        if splice is not None:
            mask_host = splice[0]
        elif attention_mask is not None and past_key_values is None:
            mask_host = attention_mask.to(torch.int32).tolist()
        else:
            mask_host = [[1] * S for _ in range(B)]
        if past_key_values is None:
            seqs = [SequenceState() for _ in range(B)]
            need = sum((sum(r) + 63) // 64 + 1 for r in mask_host)
            if use_cache:
                self._ensure_kv(need + B * 2)
            else:
                self._ensure_kv(need)
            past = PagedPast(self.kv, seqs, S)
        else:
            past = past_key_values
            seqs = past.seqs
            mask_host = [[1] * S] * B                    # a continuation has no padding: every row is fed
            past.padded_len += S
        flat, flat_lo, lens, idx = self._pack_rows(inputs_embeds, mask_host)
        rows = flat.shape[0]
        if output_attentions:
            # (the reference's eager LlamaAttention returns the [B, heads, S, S] probabilities of every layer; the flash kernels never
            # materialise them -- refuse instead of returning None silently)
            raise NotImplementedError("output_attentions=True: the attention probabilities are never materialised by the HIP flash-attention kernels")
        trace = None
        if output_hidden_states:
            logits_p, hidden, trace = llama_forward(llama, past.kv, seqs, flat, lens, logit_rows=list(range(rows)), return_all_hidden=True,
                                                    embeds_lo=flat_lo)
        else:
            logits_p, hidden = llama_forward(llama, past.kv, seqs, flat, lens, logit_rows=list(range(rows)), return_hidden=True, embeds_lo=flat_lo)
        sel = torch.tensor(idx, device=flat.device) if len(idx) != B * S else None

        def unpack(t):       # packed rows [rows, D] -> the caller's padded [B, S, D] (zeros at the padding rows)
            if sel is None:
                return t.contiguous().view(B, S, t.shape[-1])
            full = torch.zeros((B * S, t.shape[-1]), dtype=t.dtype, device=t.device)
            full.index_copy_(0, sel, t.contiguous())
            return full.view(B, S, t.shape[-1])

        logits = unpack(logits_p)
        all_hidden = None
        if output_hidden_states:
            # transformers 4.31 LlamaModel.forward: the stream in front of every decoder layer (entry 0 = inputs_embeds), then the
            # FINAL-NORMED output of the last layer -- num_layers + 1 tensors [B, S, H]; fp32 here (the residual stream is fp32), the
            # last one in the operand dtype (it is the lm_head's operand)
            final = ops.rmsnorm(hidden, llama.final_norm, float(llama.model.rms_eps), dtype=llama.dtype)
            all_hidden = tuple(unpack(trace[l]) for l in range(trace.shape[0])) + (unpack(final),)
        loss = None
        if labels is not None:  # shifted cross entropy, ignore_index -100 (LlamaForCausalLM.forward)
            # one row per (sample, position < S-1): position j scores label j+1; the last position of every sample scores nothing
            shifted = torch.full((B, S), -100, dtype=torch.int32, device=logits.device)
            shifted[:, :-1] = labels[:, 1:].to(device=logits.device, dtype=torch.int32)
            loss = ops.cross_entropy(logits.view(B * S, llama.V), shifted.reshape(-1), ignore_index=-100)
        if not use_cache and past_key_values is None:
            past.release()
            past = None
        return CausalLMOutputWithPast(loss=loss, logits=logits, past_key_values=past, hidden_states=all_hidden, attentions=None)

    __call__ = forward

    # ---- reference llava_llama.py:104-114 ----------------------------------------------------------------------
    def prepare_inputs_for_generation(self, input_ids, past_key_values=None, inputs_embeds=None, **kwargs):
        images = kwargs.pop("images", None)
        regions = kwargs.pop("regions", None)
        if past_key_values is not None:
            input_ids = input_ids[:, -1:]
        inputs = {"input_ids": input_ids, "past_key_values": past_key_values, "use_cache": kwargs.get("use_cache", True),
                  "attention_mask": kwargs.get("attention_mask", None)}
        if inputs_embeds is not None and past_key_values is None:
            inputs = {"inputs_embeds": inputs_embeds, **{k: v for k, v in inputs.items() if k != "input_ids"}}
        if images is not None:
            inputs["images"] = images
        if regions is not None:
            inputs["regions"] = regions
        return inputs

    # ---- GenerationMixin.generate / sample, as app.py:562-571 drives it ----------------------------------------
    @torch.no_grad()
    def generate(self, input_ids=None, images=None, regions=None, attention_mask=None, do_sample=False,
                 temperature=1.0, top_p=1.0, top_k=None, max_new_tokens=None, max_length=None, use_cache=True,
                 stopping_criteria=None, eos_token_id=None, pad_token_id=None, num_beams=1, seed=None,
                 return_logits=False, padded_batch=False, repetition_penalty=1.0, return_logprobs=False, suppress_tokens=None,
                 begin_suppress_tokens=None, min_new_tokens=None, bad_words_ids=None, allowed_token_ids=None, num_return_sequences=1,
                 length_penalty=1.0, early_stopping=False, no_repeat_ngram_size=None, sequence_bias=None, presence_penalty=0.0,
                 frequency_penalty=0.0, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None, top_logprobs=0, automaton=None, choices=None,
                 **kwargs):
        """repetition_penalty (RepetitionPenaltyLogitsProcessor; 1.0 is off) and return_logprobs: with both at their defaults a step
        launches what it always did (vt_argmax / vt_sample_top_p). Otherwise every step is ONE vt_sample_rows launch (row b: stream = b,
        counter = step -- today's draws) whose penalty history -- the sample's non-negative prompt ids plus what it has generated -- lives
        and grows on the device. return_logprobs=True additionally returns a [B, n_new] fp32 tensor: log_softmax of the raw logits at every
        emitted id (for a row that has finished, of the id it would have emitted instead of the pad). Returns ids; (ids, all_logits) with
        return_logits; the log-probabilities come last: (ids, logprobs) or (ids, all_logits, logprobs).
        Constraints on which ids may be emitted at all, for the whole batch: suppress_tokens
        (SuppressTokensLogitsProcessor), begin_suppress_tokens (BeginSuppressTokensLogitsProcessor: the first generated token only),
        min_new_tokens (MinNewTokensLengthLogitsProcessor: the EOS ids are banned while fewer tokens have been generated), bad_words_ids
        (NoBadWordsLogitsProcessor, single-token entries only; a longer entry raises NotImplementedError) and this project's own
        allowed_token_ids (only these ids). With any of them every step is ONE vt_sample_rows_allow launch; the few distinct masks a call
        needs and the per-step pointer array are uploaded once before the loop. At the defaults nothing changes.
        no_repeat_ngram_size = g (NoRepeatNGramLogitsProcessor; None or 0 is off): no n-gram of g ids occurs twice in a
        sample's history -- its input_ids where attention_mask is 1, in order and with the image / region sentinels as they are, followed
        by the tokens it emits. The history lives and grows on the device; every step is one vt_ban_rows launch, which builds each row's
        allow mask from (the step's static mask above, or nothing; the history), followed by one vt_sample_rows_allow launch that reads
        those masks. Every step's vt_ban_row array is uploaded once before the loop: no host wait, no per-step upload. The device-built
        mask is never read back, so a row it leaves nothing for cannot raise: it gets what vt_sample_rows_allow defines for a row with
        nothing allowed (the static constraints keep their host checks). Refused with NotImplementedError: num_beams > 1, padded_batch.
        Additive adjustments: sequence_bias (transformers' dict {tuple of ids: float}, SequenceBiasLogitsProcessor; a bare
        int is a one-token key; a key of several tokens raises NotImplementedError) is added to the logits BEFORE the repetition penalty;
        presence_penalty and frequency_penalty (OpenAI's / vLLM's; any finite float) take presence + frequency * count off every id the
        sample has GENERATED so far, AFTER it. Each sample owns a [V][2] adjustment on the device that vt_bias_rows rebuilds before every
        pick from the sample's generated ids (once, before the prefill, with sequence_bias alone) and vt_sample_rows_adj reads; nothing
        is uploaded or waited for in the loop. return_logits and return_logprobs stay RAW. ValueError: an id outside [0, vocab_size), a
        value that is not finite, an id given twice. Refused with NotImplementedError: num_beams > 1, padded_batch.
        Truncation: min_p, typical_p, epsilon_cutoff and eta_cutoff are transformers' MinPLogitsWarper,
        TypicalLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper (None, or min_p 0 / typical_p 1 / a cutoff 0, is off). With
        do_sample=True they run in that order after top-k and top-p inside the sampler kernel: every step is ONE vt_sample_rows_trunc
        launch, nothing is read back; without do_sample they are ignored, as transformers applies warpers only when sampling.
        ValueError: min_p outside [0, 1], typical_p outside (0, 1], a cutoff outside [0, 1), a value that is not finite. Refused with
        NotImplementedError: num_beams > 1, padded_batch.
        padded_batch=True (B > 1, right padding): reproduce what the REFERENCE's batched generate() returns -- transformers 4.31 reads the
        first token of every sample from the last COLUMN of the padded logits (a pad row for the shorter samples) and the decode-step
        fix-up (llava_arch.py:196-205) attends the pad rows of the spliced batch while masking the rows that share an index with the
        ids-length mask's zeros (engine.padded_batch_fixup; pinned by tests/golden/greedy_batch.npz). Default False: sequences are packed
        and every sample gets the ids the reference returns for it ALONE.
        num_beams = k > 1: greedy beam search in packed mode for B >= 1 prompts, transformers' algorithm (the release
        this project is tested against) with num_return_sequences (<= num_beams), length_penalty and early_stopping (False / True /
        "never"). One ordinary prefill per prompt, then per step one decoder pass over the live groups' B * k rows, one vt_beam_step and
        one read-back of the candidates; the k beams of a prompt share its whole prompt pages and own their tails (vitron_amd.beam).
        Returns a LongTensor [B * num_return_sequences, longest] that starts with the prompt's ids and is padded with pad_token_id; the
        hypotheses' scores are left in self.last_beam_scores (fp32 [B * num_return_sequences]). The call neither reuses nor leaves a KV
        prefix. Refused with NotImplementedError before any page is taken: do_sample, padded_batch, repetition_penalty != 1, every
        constraint argument above (no_repeat_ngram_size included), stopping_criteria, return_logits / return_logprobs, num_beams > 16, and a candidate list
        (max(2, 1 + number of EOS ids) * num_beams per step, as in transformers) beyond the vocabulary or beyond vt_beam_step's 32.
        num_beams = 1 runs the code it always ran.
        top_logprobs = N in [1, 20] (0 is off): after the other outputs a dict is returned -- top_ids int32 [B, n_new, N]
        and top_logprobs fp32 [B, n_new, N], every step's N most likely tokens of the RAW distribution (larger logit first, ties by the
        lower id) with their log-probabilities, and rank int32 [B, n_new], the emitted id's rank in that order (1 is the most likely).
        Every pick is followed by ONE vt_logprob_rows launch that writes into buffers allocated before the loop; the pick itself, the
        ids and return_logprobs are what they are without it. For a row that has finished the values are those of the id it would have
        emitted, as with return_logprobs. Refused with NotImplementedError: num_beams > 1, padded_batch; ValueError outside [0, 20].
        Guided decoding: automaton = a vitron_amd.automaton.TokenAutomaton (TokenAutomaton.from_regex(pattern, vocab),
        .from_choices(...)); choices=[[ids], ...] is automaton=TokenAutomaton.from_choices(choices). Every sample runs the automaton from
        its start state with a {state, consumed} cell of its own on the device: every step is one vt_fsm_rows launch, which moves the
        state over the id the sample emitted last and builds its allow mask from (the step's static mask above, or nothing; the
        state), then vt_ban_rows with that mask as its base when no_repeat_ngram_size is on, then one vt_sample_rows_allow launch that
        reads the last mask built. The tables, the cells and every step's vt_fsm_row array are uploaded once before the loop: no host
        wait, no per-step upload. The call's EOS ids are allowed exactly in the accepting states (min_new_tokens still withholds them).
        The device-built mask is never read back: a state that allows nothing cannot raise. ValueError before the prefill: more than 4
        EOS ids, an accepting state with no EOS id in [0, vocab_size), a start state that allows nothing, automaton together with
        choices. Refused with NotImplementedError: num_beams > 1, padded_batch.
        Classifier-free guidance (transformers' guidance_scale / negative_prompt_ids, its
        UnbatchedClassifierFreeGuidanceLogitsProcessor), taken from **kwargs: guidance_scale = s (None or 1 is off and the call runs the
        launches it always ran), negative_prompt_ids ([B, Ln], or [1, Ln] for every sample; None: each sample's last token, a
        ValueError when that is a sentinel), negative_attention_mask, negative_images / negative_regions (for the sentinels of the negative
        prompt, as images / regions are for input_ids; with a [1, Ln] prompt they are given once and used for every sample) and
        guidance_plausibility = beta in [0, 1] (0 is off; contrastive decoding's cut: a token stays only if p_cond >= beta max p_cond).
        The call owns 2B sequences: the conditional prefill is the unguided call's (same packing, same prefix reuse, so the step-0
        conditional logits are bit-identical), the negative prompts are prefilled in a pass of their own and neither take nor leave a KV
        prefix, and one DecodeState steps all 2B with the picked ids fed twice. A step is one decoder pass over 2B rows, ONE vt_cfg_rows
        launch that writes scale * (log_softmax(cond) - log_softmax(uncond)) + log_softmax(uncond) in place over the conditional rows, then
        the picker as it is: penalties, bias, masks, the sampler, return_logprobs and top_logprobs all see the guided row (transformers
        runs its CFG processor first). return_logits keeps returning the conditional model rows. Every step's vt_cfg_row array is
        uploaded once before the loop. With beta > 0 the picker runs per row and the launch also writes each row's plausibility mask
        from (the step's static mask, the conditional row); that mask is the base of vt_fsm_rows / vt_ban_rows or what the sampler
        reads. ValueError before any device work: a scale that is not finite, beta outside [0, 1], a negative_* argument or beta
        without a scale, an empty negative prompt or one whose batch size is neither 1 nor B. Refused with NotImplementedError:
        num_beams > 1, padded_batch.
        Contrastive search (transformers' penalty_alpha / top_k, Su et al. 2022), penalty_alpha taken from **kwargs: the
        mode is on when penalty_alpha > 0, top_k > 1, do_sample is False and num_beams == 1 (transformers' rule); penalty_alpha None or 0,
        or top_k == 1, is off and the call runs the launches it always ran. Per sequence and step: the k = top_k most probable ids of the
        current logit row with their probabilities p (softmax over the full vocabulary, no warper), k single-query decode rows behind
        the same context, d = the largest cosine between a candidate's final-normed hidden state and that of EVERY earlier position
        (prompt, visual and generated rows -- the context bank, unit vectors in the operand format), and the candidate with the largest
        (1 - alpha) p - alpha d is emitted (ties to the lower rank); its hidden state joins the bank on the device and its logit row is the
        next step's current row. A step is ONE vt_logprob_rows launch, one decoder pass over the live sequences' k rows, ONE vt_unit_rows
        and ONE vt_contrast_rows launch and one read-back (the selection and the id, per sequence); a contrastive.CandidateGroup copies
        at most k - 1 KV pages. n new tokens cost n passes of k rows. The call neither takes nor leaves a KV prefix. stopping_criteria
        is served. ValueError before any device work: penalty_alpha not a finite number in [0, 1], or > 0 with do_sample=True. Refused
        with NotImplementedError, naming the argument: top_k left at its default or outside [2, 16] (1 is off), num_beams > 1,
        padded_batch, repetition_penalty != 1, every optional processor argument (suppress_tokens ... automaton), return_logits,
        return_logprobs, top_logprobs, guidance_scale.
        DoLa (transformers 4.4x' dola_layers, Chuang et al. 2023), dola_layers and dola_relative_top (default 0.1) taken
        from **kwargs: dola_layers "low" / "high" / a list of layer indices names the candidate layers (index i = the INPUT stream of
        decoder layer i, sampling.dola_candidate_layers); None is off and the call runs the launches it always ran. Per step: the decoder
        pass also writes the candidate layers' streams at the B logit rows (vt_llama_model.logit_row_trace: one small launch per
        candidate layer), the bare lm_head runs over those n_cand * B rows in launches of at most 16 rows (the weight-streaming kernel of
        a decode step's lm_head) into a buffer the call owns, and ONE vt_dola_rows launch picks, per row, the candidate furthest from
        the final layer and writes log_softmax(final) - log_softmax(candidate) in place over the row, -inf outside the tokens with
        p_final >= dola_relative_top * max p_final, plus the mask of those tokens. Everything behind it -- penalties, bias, the other
        masks, the per-row sampler (greedy or sampling), return_logprobs, top_logprobs -- sees the contrasted row; return_logits are the
        model's final rows. Every row chooses its own layer (transformers averages the divergences over the batch): a row gets what it
        gets alone. self.last_dola_layers: int64 [B, n] -- the layer chosen for every emitted token. ValueError before any device work:
        a bad dola_layers, dola_relative_top outside (0, 1]. Refused with NotImplementedError, naming the argument: num_beams > 1,
        penalty_alpha > 0, guidance_scale, padded_batch.
        SynthID text watermark (transformers' watermarking_config = SynthIDTextWatermarkingConfig, its
        SynthIDTextWatermarkLogitsProcessor), taken from **kwargs: a SynthIDTextWatermarkingConfig, a dict of its fields or a
        vitron_amd.watermark.SynthIDWatermark; None is off and the call runs the launches it always ran. transformers runs the
        processor behind every warper, so the tournament lives in the sampler: every step's sampler launch is ONE vt_sample_rows_wm,
        behind everything that shapes the row (guidance, DoLa, bans, automata, bias, the truncation stages). Every sample owns an
        all-zero cell on the device (transformers' fresh state: the context holds generated tokens only); the cells and the B vt_wm_row
        entries are uploaded once before the loop. return_logits, return_logprobs and top_logprobs stay RAW.
        vitron_amd.watermark.SynthIDWatermark(config).mean_g(ids, generated_from=prompt length) scores a reply. ValueError /
        NotImplementedError before any device work: what SynthIDWatermark refuses (the green-list WatermarkingConfig, debug_mode, a
        sampling table that is no power of two in [32, 65536], ...). Refused with NotImplementedError before any page is taken:
        do_sample=False, num_beams > 1, penalty_alpha > 0, padded_batch, vocab_size > 32768.
        Mirostat v2 (Basu et al., ICLR 2021; llama.cpp's `mirostat 2`), mirostat_tau, mirostat_eta (default 0.1) and
        mirostat_mode (default 2) taken from **kwargs: mirostat_tau = the target surprise in bits per token; None or 0 is off and the
        call runs the launches it always ran. Every sample owns a cell {mu, last_surprise} on the device, {2 * tau, 0} at the first pick; every
        step's sampler launch is ONE vt_sample_rows_miro: behind everything that shapes the row (guidance, DoLa, bans, automata, bias,
        top-k, top-p, the truncation stages) the tokens whose surprise under the renormalised row exceeds mu leave, the id is drawn
        from the rest, and mu moves by -eta * (its surprise - tau) -- all on the device, nothing is read back in the loop. Unlike
        llama.cpp, top_k / top_p are NOT switched off by Mirostat: leave them off (top_k=0, top_p=1.0) for its behaviour.
        self.last_generate_stats["mirostat"] = {"mu": [B], "surprise": [B]} is read once behind the loop; the cells are dropped with
        the call. return_logits, return_logprobs and top_logprobs stay RAW. ValueError before any device work: mirostat_tau outside
        [0, 64], mirostat_eta outside [0, 1], a mirostat_mode that is not 0, 1 or 2, mirostat_tau with mirostat_mode=0. Refused with
        NotImplementedError that names mirostat_tau, before any page is taken: mirostat_mode=1 (Mirostat v1), do_sample=False,
        num_beams > 1, penalty_alpha > 0, padded_batch, watermarking_config, vocab_size > 32768."""
        from ...picker import StepPicker, negative_prompt, resolve_generate_args
        guide = {k: kwargs.pop(k, None) for k in ("guidance_scale", "negative_prompt_ids", "negative_attention_mask", "negative_images",
                                                  "negative_regions", "guidance_plausibility")}
        penalty_alpha = kwargs.pop("penalty_alpha", None)
        dola_layers, dola_relative_top = kwargs.pop("dola_layers", None), kwargs.pop("dola_relative_top", 0.1)
        watermarking_config = kwargs.pop("watermarking_config", None)
        miro = {k: kwargs.pop(k, d) for k, d in (("mirostat_tau", None), ("mirostat_eta", 0.1), ("mirostat_mode", 2))}
        a = resolve_generate_args(
            self.config, input_ids.shape[1], do_sample=do_sample, temperature=temperature, top_p=top_p, top_k=top_k,
            max_new_tokens=max_new_tokens, max_length=max_length, stopping_criteria=stopping_criteria, eos_token_id=eos_token_id,
            pad_token_id=pad_token_id, num_beams=num_beams, seed=seed, return_logits=return_logits, padded_batch=padded_batch,
            repetition_penalty=repetition_penalty, return_logprobs=return_logprobs, suppress_tokens=suppress_tokens,
            begin_suppress_tokens=begin_suppress_tokens, min_new_tokens=min_new_tokens, bad_words_ids=bad_words_ids,
            allowed_token_ids=allowed_token_ids, num_return_sequences=num_return_sequences, length_penalty=length_penalty,
            early_stopping=early_stopping, no_repeat_ngram_size=no_repeat_ngram_size, sequence_bias=sequence_bias,
            presence_penalty=presence_penalty, frequency_penalty=frequency_penalty, min_p=min_p, typical_p=typical_p,
            epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff, top_logprobs=top_logprobs, automaton=automaton, choices=choices,
            batch_size=input_ids.shape[0], penalty_alpha=penalty_alpha, dola_layers=dola_layers, dola_relative_top=dola_relative_top,
            watermarking_config=watermarking_config, **miro, **guide)
        self.last_dola_layers = None
        dev = self.device
        neg_ids = neg_mask = None
        if a.guided and a.num_beams == 1:
            neg_ids, neg_mask = negative_prompt(input_ids, attention_mask, guide["negative_prompt_ids"], guide["negative_attention_mask"])
        input_ids = input_ids.to(dev)
        B, L0 = input_ids.shape
        max_new_tokens, eos_ids = a.max_new_tokens, sorted(a.eos)
        reuse = B == 1 and bool(getattr(self.config, "kv_prefix_reuse", True))
        embeds, mask_host, embeds_spliced = self._embed_prompt(input_ids, attention_mask, images, regions, use_vis_cache=reuse)
        S = embeds.shape[1]
        flat, flat_lo, lens, _ = self._pack_rows(embeds, mask_host)
        seqs = [SequenceState() for _ in range(B)]
        # (a beam call and a contrastive call neither reuse nor leave a KV prefix)
        sig, kept = self._take_prefix(reuse and a.num_beams == 1 and not a.contrastive, input_ids, mask_host, embeds_spliced, seqs[0])
        if a.num_beams > 1:
            return self._generate_beams(a, input_ids, seqs, flat, flat_lo, lens)
        if a.contrastive:
            return self._generate_contrastive(a, input_ids, seqs, flat, flat_lo, lens, stopping_criteria)
        pad_mode, ids_valid = self._padded_batch_rules(a.padded_batch, input_ids, attention_mask, embeds_spliced, S, lens)
        tower_items = self.last_tower_items
        nseqs, nlens = [], []
        if a.guided:     # the negative prompts: B more sequences, embedded without the feature cache (they leave no prefix signature)
            n_img, n_reg = guide["negative_images"], guide["negative_regions"]
            if guide["negative_prompt_ids"] is not None and guide["negative_prompt_ids"].shape[0] == 1 and B > 1:
                n_img = None if n_img is None else list(n_img) * B
                n_reg = None if n_reg is None else list(n_reg) * B
            nemb, nmask_host, _ = self._embed_prompt(neg_ids.to(dev), neg_mask, n_img, n_reg, use_vis_cache=False)
            nflat, nflat_lo, nlens, _ = self._pack_rows(nemb, nmask_host)
            nseqs = [SequenceState() for _ in range(B)]
        kept = self._ensure_generate_pages(seqs, lens + nlens, max_new_tokens, kept, S if pad_mode else None)
        self.last_generate_stats = {"prompt_rows": int(sum(lens)), "reused_tokens": int(kept),
                                    "prefill_rows": int(sum(lens) - kept), "tower_items": tower_items}
        if a.guided:
            self.last_generate_stats["negative_rows"] = int(sum(nlens))
        if kept:
            flat, lens = flat[kept:], [lens[0] - kept]
            flat_lo = None if flat_lo is None else flat_lo[kept:]
        picker = StepPicker(a, input_ids, attention_mask, int(self.config.vocab_size))
        # ---- decode loop: device-resident step state, the next pass is enqueued before the host has seen the token it consumes
        llama = self.model.llama
        out_host = torch.empty((B, L0 + max_new_tokens), dtype=torch.long)
        out_host[:, :L0] = input_ids.cpu()
        n_out = L0
        all_logits = []
        state = None
        try:   # (the prefill is inside: pages it took before a failure go back to the pool / the kept prefix below)
            dola = None
            if a.dola:       # the prefill also leaves the candidate layers' streams at its B logit rows
                logits, trace0 = llama_forward(llama, self.kv, seqs, flat, lens, embeds_lo=flat_lo, trace_rows_layers=a.dola_layers)
                dola = _DolaHead(llama, a.dola_layers, B, trace0)
            else:
                logits = llama_forward(llama, self.kv, seqs, flat, lens, embeds_lo=flat_lo) # [B, V]: last position of every sequence
            picker.check_width(logits)
            if pad_mode:
                from ...engine import padded_batch_fixup
                fix = padded_batch_fixup(llama, self.kv, seqs, S, ids_valid, L0)
                logits = logits.clone()
                for b, lg in fix["pad_logits"].items():       # shorter samples: the first token comes from their last PAD row
                    logits[b] = lg
                self.last_generate_stats["padded_batch"] = {"pad_rows": {b: S - lens[b] for b in fix["pad_logits"]}, "masked_rows": fix["holes"]}
            bufs = None
            if a.guided:     # a pass of their own; the steps' vt_cfg_row arrays name these rows and the two decode buffers: one upload
                ulogits = llama_forward(llama, self.kv, nseqs, nflat, nlens, embeds_lo=nflat_lo)
                if max_new_tokens > 1:
                    bufs = [torch.empty((2 * B, llama.V_pad), dtype=torch.float32, device=dev) for _ in range(2)]
                picker.attach_guidance(logits, ulogits, bufs)
            if dola is not None:     # the candidates of step 0; the steps' vt_dola_row arrays name these rows and the decode buffers: one upload
                prem0 = dola.head(torch.empty((len(a.dola_layers), B, llama.V_pad), dtype=torch.float32, device=dev))
                if max_new_tokens > 1:
                    bufs = [torch.empty((B, llama.V_pad), dtype=torch.float32, device=dev) for _ in range(2)]
                    pbufs = [torch.empty_like(prem0) for _ in range(2)]
                picker.attach_dola(logits, prem0, bufs, pbufs if max_new_tokens > 1 else None)
            for step in range(max_new_tokens):
                if a.return_logits:
                    all_logits.append(logits.clone())
                nxt = picker.pick(step, logits)
                last = step + 1 == max_new_tokens
                scores = logits
                if state is None and last:    # single-token call (prefill benchmarks, scoring): no decode state to set up
                    toks = nxt.tolist()
                    fin = [t in a.eos for t in toks]
                else:
                    if state is None:
                        state = DecodeState(llama, self.kv, seqs + nseqs, max_new_tokens, eos_ids, a.pad)
                    slot = state.feed(torch.cat((nxt, nxt)) if a.guided else nxt)
                    if not last:                          # speculative: rolled back below if this token ends the run
                        if dola is not None:
                            logits = state.forward(bufs[(step + 1) & 1], trace_rows_layers=a.dola_layers, trace_rows_out=dola.trace)
                            dola.head(pbufs[(step + 1) & 1])
                        else:
                            logits = state.forward(bufs[(step + 1) & 1])[:B] if a.guided else state.forward()
                    toks, fin = state.read(slot)
                    toks, fin = toks[:B], fin[:B]
                out_host[:, n_out] = torch.tensor(toks, dtype=torch.long)
                n_out += 1
                stop = all(fin)
                if not stop and stopping_criteria is not None:
                    stop = any(c(out_host[:, :n_out], scores) for c in stopping_criteria)    # StoppingCriteriaList: any()
                if stop:
                    if state is not None and not last:
                        state.rollback()
                    break
        finally:
            self._leave_prefix(sig, seqs, out_host[0, L0:n_out])
            for s in nseqs:
                self.kv.release(s.pages)
        out = out_host[:, :n_out].to(dev)
        if a.mirostat_tau > 0:       # read once, behind the loop; the cells end with the call
            state_m = picker.mirostat_state()
            if state_m is not None:
                self.last_generate_stats["mirostat"] = state_m
            picker.drop_mirostat()
        if picker.dola_choice is not None:
            self.last_dola_layers = torch.tensor(a.dola_layers, dtype=torch.long, device=dev)[picker.dola_choice[:n_out - L0].long().t()]
        res = (out,) + ((all_logits,) if a.return_logits else ()) + ((picker.logprobs(n_out - L0),) if a.return_logprobs else ()) \
            + ((picker.top(n_out - L0),) if a.top_logprobs else ())
        return res if len(res) > 1 else out

    # ---- log-probabilities of GIVEN tokens -----------------------------------------------------------
    @torch.no_grad()
    def score(self, input_ids, images=None, regions=None, top_logprobs=0, return_logits=False, attention_mask=None,
              packed_prefill=False):
        """The log-probability and the rank of every token of `input_ids` given what stands before it -- prompt scoring.
        input_ids: LongTensor [B, L] (or [L]) with the <image> / <objs> sentinels as generate() takes them, right-padded where
        attention_mask is 0; or a list of B 1-D id tensors of any lengths (padded here). images / regions: as for generate().
        Towers, splice and decoder prefill run as generate()'s prefill does (through the encoded-image cache); llama_forward's logit
        rows are the spliced rows whose NEXT row is a text token (scoring.score_targets: the rule, decided from the splice plan), each
        with that token as its target, followed by ONE vt_logprob_rows launch over the rows of the whole batch.
        packed_prefill=False (default): every sequence of a batch gets a decoder pass of its own, so its numbers are those of the
        same sequence scored alone, bit for bit, whatever else is in the batch (ServingEngine's default admission makes the same
        choice). True: ONE packed pass over all sequences, as generate() prefills a batch -- larger GEMMs; the logits then differ from
        a solo call's by 16-bit GEMM noise (other tiles), as with ServingEngine(batch_prefill=True). Returns a dict of
        device tensors, one value per position of input_ids:
          "logprobs" fp32 [B, L], "rank" int32 [B, L] (1: the most likely token). A position without a target -- the first token, an
          <image> / <objs> sentinel, padding, a token truncated away -- holds NaN / 0;
          with top_logprobs = N in [1, 20]: "top_ids" int32 [B, L, N] and "top_logprobs" fp32 [B, L, N], the N most likely tokens at that
          position (larger logit first, ties by the lower id) -- -1 / NaN where there is no target;
          with return_logits: "logits" fp32 [n, V], the rows that were scored, and "logit_index" int64 [n, 3]: (sample, position of the
          scored token in input_ids, spliced row that was read) of each.
        The call takes its KV pages privately -- from the pool's free pages when they suffice, else from a pool of its own that lives for
        the call -- and gives them back before it returns: the pool, the kept conversation (the KV prefix of generate()) and the
        encoded-image cache's contents other than newly encoded items are what they were."""
        from ...sampling import check_top_logprobs
        from ...scoring import score_targets
        check_top_logprobs(top_logprobs, "score")
        n_top = int(top_logprobs)
        dev = self.device
        if isinstance(input_ids, (list, tuple)):
            if attention_mask is not None:
                raise ValueError("score: a list of sequences brings its own lengths; attention_mask is for a padded tensor")
            seqs_in = [torch.as_tensor(t).reshape(-1).to(torch.long) for t in input_ids]
            if not seqs_in or any(t.numel() == 0 for t in seqs_in):
                raise ValueError("score: every sequence needs at least one token")
            L = max(int(t.numel()) for t in seqs_in)
            input_ids = torch.zeros((len(seqs_in), L), dtype=torch.long)
            attention_mask = torch.zeros((len(seqs_in), L), dtype=torch.long)
            for b, t in enumerate(seqs_in):
                input_ids[b, :t.numel()] = t.cpu()
                attention_mask[b, :t.numel()] = 1
        elif input_ids.dim() == 1:
            input_ids = input_ids.unsqueeze(0)
        input_ids = input_ids.to(dev)
        B, L = input_ids.shape
        self._last_plan = None
        embeds, mask_host, spliced = self._embed_prompt(input_ids, attention_mask, images, regions, use_vis_cache=True)
        S = embeds.shape[1]
        flat, flat_lo, lens, _ = self._pack_rows(embeds, mask_host)
        ids_host = input_ids.cpu().tolist()
        am_host = attention_mask.to(torch.int32).cpu().tolist() if attention_mask is not None else [[1] * L] * B
        plan = self._last_plan if spliced else None
        logit_rows, targets, where = [], [], []       # packed row read, its target, (sample, position, spliced row)
        per_seq = []                                  # (first packed row, rows, the sequence's own rows to read)
        row0 = 0
        for b in range(B):
            pos_of = [j for j in range(L) if am_host[b][j]]
            ids_b = [ids_host[b][j] for j in pos_of]
            kinds = [0] * lens[b] if plan is None else [int(plan[b, s, 0]) for s in range(S) if mask_host[b][s]]
            rows_b, tg_b, at_b = score_targets(ids_b, kinds)
            logit_rows += [row0 + r for r in rows_b]
            targets += tg_b
            where += [(b, pos_of[j], r) for j, r in zip(at_b, rows_b)]
            per_seq.append((row0, lens[b], rows_b))
            row0 += lens[b]
        res = {"logprobs": torch.full((B, L), float("nan"), dtype=torch.float32, device=dev),
               "rank": torch.zeros((B, L), dtype=torch.int32, device=dev)}
        if n_top:
            res["top_ids"] = torch.full((B, L, n_top), -1, dtype=torch.int32, device=dev)
            res["top_logprobs"] = torch.full((B, L, n_top), float("nan"), dtype=torch.float32, device=dev)
        if not logit_rows:
            if return_logits:
                res["logits"] = torch.empty((0, int(self.config.vocab_size)), dtype=torch.float32, device=dev)
                res["logit_index"] = torch.empty((0, 3), dtype=torch.long)
            return res
        pages = [(l + 63) // 64 + 1 for l in lens]
        need = sum(pages) if packed_prefill else max(pages)
        kv = self.kv if (self.kv is not None and self.kv.kv_dtype == self._kv_format() and len(self.kv.free) >= need) \
            else self.new_kv_pool(need)
        llama = self.model.llama

        def prefill(rows_from, n_rows, q_lens, read):
            seqs = [SequenceState() for _ in q_lens]
            try:
                return llama_forward(llama, kv, seqs, flat[rows_from:rows_from + n_rows], q_lens, logit_rows=read,
                                     embeds_lo=None if flat_lo is None else flat_lo[rows_from:rows_from + n_rows])
            finally:                                  # the pages go back whatever happened
                for s in seqs:
                    if s.pages:
                        kv.release(s.pages)
                    s.pages, s.length = [], 0
        if packed_prefill or B == 1:
            logits = prefill(0, int(sum(lens)), lens, logit_rows)                                        # [n, V]
        else:
            logits = torch.cat([prefill(r0, l, [l], rows_b) for r0, l, rows_b in per_seq if rows_b], 0)
        got = ops.logprob_rows(logits, torch.tensor(targets, dtype=torch.int32).to(dev), n_top, return_rank=True)
        flat_at = torch.tensor([b * L + j for b, j, _ in where], dtype=torch.long).to(dev)
        res["logprobs"].view(-1).index_copy_(0, flat_at, got["logprob"])
        res["rank"].view(-1).index_copy_(0, flat_at, got["rank"])
        if n_top:
            res["top_ids"].view(B * L, n_top).index_copy_(0, flat_at, got["top_ids"])
            res["top_logprobs"].view(B * L, n_top).index_copy_(0, flat_at, got["top_logprobs"])
        if return_logits:
            res["logits"] = logits
            res["logit_index"] = torch.tensor(where, dtype=torch.long)
        return res

    @torch.no_grad()
    def rank_options(self, prompt_ids, options, images=None, regions=None, normalize="sum", packed_prefill=False):
        """Rank the answer options of a multiple-choice question by the log-probability the model gives their tokens behind the prompt.
        prompt_ids: 1-D ids (sentinels as for generate()); options: non-empty id sequences; images / regions: the prompt's own (one
        entry per <image> of the prompt), shared by all options. prompt + option is built for every option and the lot is scored as
        ONE batch through score() (packed_prefill: as there -- by default an option's score does not depend on which other options
        stand beside it); the image is encoded once: it enters the encoded-image cache with the first option and every
        other option finds it there. An option's score is the sum of its tokens' log-probabilities (normalize="sum") or their mean
        ("mean"). Returns (order, scores): the option indices by descending score -- ties keep option order -- and the fp64 scores
        in option order. (Every option prefills the prompt again: sharing the prompt's KV pages is left open)"""
        from ...scoring import option_score, rank_order
        if normalize not in ("sum", "mean"):
            raise ValueError(f"rank_options: normalize must be 'sum' or 'mean', got {normalize!r}")
        prompt = torch.as_tensor(prompt_ids).reshape(-1).to(torch.long).cpu()
        opts = [torch.as_tensor(o).reshape(-1).to(torch.long).cpu() for o in options]
        if not opts or any(o.numel() == 0 for o in opts):
            raise ValueError("rank_options: at least one option, and no empty one")
        if any(int(o.min()) < 0 for o in opts):
            raise ValueError("rank_options: an option holds a sentinel; options are text")
        n = len(opts)
        imgs = regs = None
        if images is not None:
            one = list(images)
            if len(one) and n > 1:       # encode the prompt's items ONCE: the first option alone fills the cache, the batch then hits it
                self._prime_visual_cache(prompt, one, regions)
            imgs = one * n
            regs = None if regions is None else list(regions) * n
        out = self.score([torch.cat([prompt, o]) for o in opts], images=imgs, regions=regs, packed_prefill=packed_prefill)
        lp = out["logprobs"].double().cpu()
        P = int(prompt.numel())
        scores = [option_score(lp[i, P:P + int(o.numel())].tolist(), normalize) for i, o in enumerate(opts)]
        return rank_order(scores), torch.tensor(scores, dtype=torch.float64)

    def _prime_visual_cache(self, prompt, images, regions):
        """Run the prompt's images / clips through the towers as a batch of ONE sample, so that they sit in the encoded-image cache."""
        if int(getattr(self.config, "vis_cache_entries", 16)) <= 0:
            return
        self._embed_prompt(prompt.unsqueeze(0).to(self.device), None, images, regions, use_vis_cache=True)

    # ---- the phases of generate() -------------------------------------------------------------------------------
    def _embed_prompt(self, input_ids, attention_mask, images, regions, use_vis_cache):
        """The prompt's embeddings with the visual rows spliced in (through the encoded-image cache for a batch of one): returns
        (embeds [B, S, H], the host 0 / 1 mask of their valid rows, whether anything was spliced)."""
        cache = None
        if use_vis_cache and int(getattr(self.config, "vis_cache_entries", 16)) > 0:
            if self._vis_cache is None:
                from ...prefix_cache import VisualFeatureCache
                self._vis_cache = VisualFeatureCache(int(getattr(self.config, "vis_cache_entries", 16)))
            cache = self._vis_cache
        self._last_row_sig = None
        self.last_tower_items = None
        (_, _, _, _, embeds, _) = self.prepare_inputs_labels_for_multimodal(input_ids, None, attention_mask, None, None,
                                                                            images, regions, feature_cache=cache)
        if embeds is not None:
            return embeds, self._last_splice[0], True
        B, L = input_ids.shape
        mask_host = attention_mask.to(torch.int32).tolist() if attention_mask is not None else [[1] * L] * B
        return self.model.embed_tokens(input_ids), mask_host, False

    def _take_prefix(self, reuse, input_ids, mask_host, embeds_spliced, seq):
        """Multi-turn KV reuse (batch 1): `seq` takes over the pages of the longest common whole-page prefix of the last call, the rest of
        the kept conversation goes back to the pool. Returns (the per-row signature of this prompt, or None when the call neither reuses
        nor leaves a prefix; the number of tokens taken over). A call that does not reuse drops the kept conversation."""
        if not reuse:
            if self._prefix is not None:
                self.reset_prefix_cache()
            return None, 0
        import numpy as np

        from ...prefix_cache import reusable_tokens
        valid = np.asarray(mask_host[0], dtype=bool)
        if self._last_row_sig is not None:
            sig = self._last_row_sig[0][valid]
        elif embeds_spliced:
            # visual rows were spliced in without the feature cache (config.vis_cache_entries = 0): there is no per-row
            # signature of the spliced sequence, so this call neither reuses nor leaves a KV prefix
            if self._prefix is not None:
                self.reset_prefix_cache()
            return None, 0
        else:
            sig = input_ids[0].cpu().numpy().astype(np.int64)[valid]
        kept = 0
        if self._prefix is not None:
            kept = reusable_tokens(self._prefix.sig, sig) if self.kv is not None else 0
            seq.pages = self._prefix.pages[:kept // 64]
            seq.length = kept
            self.kv.release(self._prefix.pages[kept // 64:])
            self._prefix = None
        return sig, kept

    def _leave_prefix(self, sig, seqs, new_ids):
        """The end of a generate() call, failed or not: a batch-1 call with a signature keeps its pages as the next call's prefix (the
        signature extended by the ids it generated), every other call gives its pages back."""
        if sig is not None and seqs[0].length > 0:
            import numpy as np

            from ...prefix_cache import PrefixKV
            full = np.concatenate([sig, new_ids.numpy().astype(np.int64)])[:seqs[0].length]      # the last sampled token was never fed back
            self._prefix = PrefixKV(full, seqs[0].pages)
        else:
            for s in seqs:
                self.kv.release(s.pages)

    def _padded_batch_rules(self, padded_batch, input_ids, attention_mask, embeds_spliced, S, lens):
        """Which padded_batch=True calls are admitted (B > 1): returns (pad_mode, the samples' numbers of valid ids). A
        right-padded multimodal batch runs the reference's padded loop (pad_mode True). A left-padded one whose padding is the same in
        the id space and in the spliced space IS the packed batch (pad_mode False). Everything else is refused."""
        B = input_ids.shape[0]
        if not (bool(padded_batch) and B > 1):
            return False, None
        if not embeds_spliced:
            # a text-only batch never reaches the reference's decode-step fix-up (llava_arch.py:196 returns early when images is
            # None); transformers then reads a shorter sample's first token from embed(pad_token_id) at position 1 -- another behaviour than
            # the one reproduced here (a ZERO row at position 0), so refuse instead of returning different ids silently
            raise NotImplementedError("generate(padded_batch=True) reproduces the reference's B > 1 result for MULTIMODAL (spliced) batches; a "
                                      "text-only batch takes another path in the reference (llava_arch.py:196-205) -- use the default packed batch")
        am_rows = attention_mask.to(torch.int32).tolist() if attention_mask is not None else [[1] * input_ids.shape[1]] * B
        side = getattr(self.config, "tokenizer_padding_side", "right")
        if side == "left":
            # LEFT-padded batches (llava_arch.py:379-386): the first token comes from the last column, which is a real row; at a decode step
            # the fix-up (:196-205) extends the ids-length mask with ones, so sample i is denied the first p_ids[i] rows of its padded cache
            # (its padding in ID space) and gets position sum(mask) - 1. When every sample's padding in ID space equals its padding in
            # the SPLICED space -- the same number of <image> / <objs> rows in every sample, what a batched app.py turn looks like -- those
            # are exactly its pad rows and the position is its own length + step: the reference's ids ARE the ids each sample gets alone,
            # i.e. the packed batch. Any other left-padded batch attends pad rows / loses real rows in the reference; not reproduced.
            if any(any(x > y for x, y in zip(r, r[1:])) for r in am_rows):
                raise NotImplementedError("generate(padded_batch=True): with tokenizer_padding_side = 'left' the attention_mask must be left-padded (zeros, then ones)")
            p_ids = [len(r) - sum(r) for r in am_rows]
            p_sp = [S - l for l in lens]
            if p_ids != p_sp:
                raise NotImplementedError(f"generate(padded_batch=True), left-padded: the samples' padding differs between the id space {p_ids} and the "
                                          f"spliced space {p_sp} (unequal numbers of visual rows): the reference then attends pad rows / masks real rows "
                                          "at decode steps (llava_arch.py:196-205); not reproduced -- use the default packed batch")
            return False, None
        if side != "right":
            raise NotImplementedError(f"generate(padded_batch=True): tokenizer_padding_side = {side!r}")
        if any(any(x < y for x, y in zip(r, r[1:])) for r in am_rows):
            raise NotImplementedError("generate(padded_batch=True): attention_mask must be right-padded (ones, then zeros)")
        return True, [sum(r) for r in am_rows]

    def _ensure_generate_pages(self, seqs, lens, max_new_tokens, kept, padded_S=None):
        """Make the pool hold the pages of prompt + max_new_tokens for every sequence, less the `kept` tokens' pages seqs[0] took over;
        in the padded mode (padded_S: the padded length) the pad rows join the cache and the compaction needs a second set of pages for a
        moment. The pool cannot grow around live pages: when it is too small the taken-over prefix is given up. Returns `kept` (then 0)."""
        packed = sum((l + max_new_tokens + 63) // 64 + 1 for l in lens)
        need = packed - kept // 64
        if padded_S is not None:
            need = sum(2 * ((padded_S + 63) // 64 + 2) + (max_new_tokens + 63) // 64 + 1 for _ in lens)
        if self.kv is None or len(self.kv.free) < need:
            if kept:
                self.kv.release(seqs[0].pages)
                seqs[0].pages, seqs[0].length, kept, need = [], 0, 0, packed
            self._ensure_kv(need)
        return kept

    # ---- beam search ---------------------------------------------------------------------------
    def _generate_beams(self, a, input_ids, seqs, flat, flat_lo, lens):
        """The beam branch of generate(): `seqs` are fresh SequenceStates, `flat` the packed prompt rows. One host round trip per step."""
        from ...beam import BeamGroup, BeamScorer
        k, n_return, max_new_tokens, pad = a.num_beams, a.num_return_sequences, int(a.max_new_tokens), a.pad
        if max_new_tokens < 1:
            raise ValueError(f"generate(num_beams > 1): max_new_tokens must be >= 1, got {max_new_tokens}")
        dev = self.device
        llama = self.model.llama
        B = len(seqs)
        need = sum((l + 63) // 64 + 1 + k * ((l + max_new_tokens + 63) // 64 - l // 64) for l in lens)
        if self.kv is None or len(self.kv.free) < need:
            self._ensure_kv(need)
        self.last_generate_stats = {"prompt_rows": int(sum(lens)), "reused_tokens": 0, "prefill_rows": int(sum(lens)),
                                    "tower_items": self.last_tower_items, "num_beams": k, "beam_steps": 0}
        scorer = BeamScorer(B, k, max_new_tokens, sorted(a.eos), a.length_penalty, a.early_stopping)
        n_cand = scorer.num_candidates
        groups = []

        def read_back(res):     # one copy of the 3 * n_cand values per group: scores (as bits), tokens, beams
            host = res.cpu()
            return host[0].view(torch.float32).tolist(), host[1].tolist(), host[2].tolist()

        try:
            logits = llama_forward(llama, self.kv, seqs, flat, lens, embeds_lo=flat_lo)       # [B, V]: the prefill, as in every mode
            # the first step: one row per prompt (transformers starts its k identical beams at [0, -1e9, ...]: only beam 0 counts)
            cs, ct, _ = read_back(ops.beam_step(logits, torch.zeros((B,), dtype=torch.float32, device=dev), B, 1, n_cand, packed=True))
            groups = [BeamGroup(llama, self.kv, seqs[g], k, max_new_tokens) for g in range(B)]
            slot_tokens, slot_scores, slot_of_child = {}, {}, {}
            for g in range(B):
                toks, _, scs = scorer.process(g, cs[g], [0] * n_cand, ct[g])
                slot_of_child[g] = list(range(len(toks)))      # every slot holds the prompt alone: child c takes slot c, no copy
                slot_tokens[g], slot_scores[g] = toks, scs
            self.last_generate_stats["beam_steps"] = 1
            while True:
                live = [g for g in range(B) if not scorer.is_done(g)]
                if not live:
                    break
                plan = torch.tensor([[0, t] for g in live for t in slot_tokens[g]], dtype=torch.int32).to(dev)
                x = ops.embed_splice(llama.embed, None, None, plan)
                logits = llama_forward(llama, self.kv, [s for g in live for s in groups[g].seqs], x, [1] * (len(live) * k))
                scores_t = torch.tensor([v for g in live for v in slot_scores[g]], dtype=torch.float32).to(dev)
                cs, ct, cb = read_back(ops.beam_step(logits, scores_t, len(live), k, n_cand, packed=True))
                self.last_generate_stats["beam_steps"] += 1
                for j, g in enumerate(live):
                    child_of_slot = {s: c for c, s in enumerate(slot_of_child[g])}
                    toks, parents, scs = scorer.process(g, cs[j], [child_of_slot[s] for s in cb[j]], ct[j])
                    if scorer.is_done(g) or not toks:
                        continue
                    new_slots = groups[g].reorder([slot_of_child[g][p] for p in parents])
                    slot_of_child[g] = new_slots
                    slot_tokens[g], slot_scores[g] = [0] * k, [0.0] * k
                    for c, s in enumerate(new_slots):
                        slot_tokens[g][s], slot_scores[g][s] = toks[c], scs[c]
        finally:
            for grp in groups:
                grp.release()
            for s in seqs:          # prompts no group took over (a failure before or inside the prefill)
                self.kv.release(s.pages)
                s.pages, s.length = [], 0
        best = scorer.finalize(n_return)
        L0 = input_ids.shape[1]
        longest = L0 + max(len(h) for grp in best for _, h in grp)
        out = torch.full((B * n_return, longest), int(pad), dtype=torch.long)
        ids_host = input_ids.cpu()
        for g, grp in enumerate(best):
            for r, (_, h) in enumerate(grp):
                out[g * n_return + r, :L0] = ids_host[g]
                out[g * n_return + r, L0:L0 + len(h)] = torch.tensor(h, dtype=torch.long)
        self.last_beam_scores = torch.tensor([sc for grp in best for sc, _ in grp], dtype=torch.float32).to(dev)
        return out.to(dev)

    # ---- contrastive search -------------------------------------------------------------------
    def _generate_contrastive(self, a, input_ids, seqs, flat, flat_lo, lens, stopping_criteria):
        """The contrastive branch of generate(): `seqs` are fresh SequenceStates, `flat` the packed prompt rows. One host round trip per
        step: the selections and the chosen ids of the live sequences, in one copy."""
        from ...contrastive import CandidateGroup
        k, alpha, max_new_tokens, pad = int(a.top_k), float(a.penalty_alpha), int(a.max_new_tokens), a.pad
        if max_new_tokens < 1:
            raise ValueError(f"generate(penalty_alpha > 0): max_new_tokens must be >= 1, got {max_new_tokens}")
        dev = self.device
        llama = self.model.llama
        B, L0 = input_ids.shape
        need = sum((l + 63) // 64 + 1 + k + (l + max_new_tokens) // 64 - l // 64 for l in lens)
        if self.kv is None or len(self.kv.free) < need:
            self._ensure_kv(need)
        self.last_generate_stats = {"prompt_rows": int(sum(lens)), "reused_tokens": 0, "prefill_rows": int(sum(lens)),
                                    "tower_items": self.last_tower_items, "top_k": k, "penalty_alpha": alpha, "contrastive_steps": 0,
                                    "pages_copied": 0}
        out_host = torch.full((B, L0 + max_new_tokens), int(pad), dtype=torch.long)
        out_host[:, :L0] = input_ids.cpu()
        n_out = L0
        groups = {}
        try:
            # the prefill, with the stream behind the last layer for EVERY row: the context bank holds the prompt's rows, visual ones included
            cur, hidden = llama_forward(llama, self.kv, seqs, flat, lens, embeds_lo=flat_lo, return_hidden=True)
            banks, at = [], 0
            for b in range(B):
                bank = torch.zeros((lens[b] + max_new_tokens, llama.H), dtype=llama.dtype, device=dev)
                ops.unit_rows(hidden[at:at + lens[b]], llama.final_norm, out=bank[:lens[b]])
                banks.append(bank)
                at += lens[b]
            self.last_generate_stats["bank_len"] = list(lens)
            del hidden
            for b in range(B):
                groups[b] = CandidateGroup(llama, self.kv, seqs[b], k, max_new_tokens)
            live = list(range(B))
            d_t = torch.empty((B, k), dtype=torch.float32, device=dev)
            score_t = torch.empty((B, k), dtype=torch.float32, device=dev)
            sel_t = torch.empty((B,), dtype=torch.int32, device=dev)
            ws = ops.contrast_workspace(B, max(lens) + max_new_tokens, dev)
            for step in range(max_new_tokens):
                n = len(live)
                top = ops.logprob_rows(cur, None, k)                       # the k most probable ids of every current row, exact order
                ids = top["top_ids"].reshape(-1)
                plan = torch.stack((torch.zeros_like(ids), ids), 1).contiguous()
                x = ops.embed_splice(llama.embed, None, None, plan)
                logits, hid = llama_forward(llama, self.kv, [s for b in live for s in groups[b].seqs], x, [1] * (n * k), return_hidden=True)
                cand = ops.unit_rows(hid, llama.final_norm, dtype=llama.dtype)
                ops.contrast_rows([{"bank": banks[b], "bank_len": lens[b] + step, "k": k, "first": j * k, "alpha": alpha,
                                    "lp": top["top_logprobs"][j], "d": d_t[j], "score": score_t[j], "sel": sel_t[j:j + 1]}
                                   for j, b in enumerate(live)], cand, ws)
                sel_dev = sel_t[:n]
                picked = top["top_ids"].gather(1, sel_dev.long().unsqueeze(1)).squeeze(1)
                host = torch.stack((sel_dev, picked)).cpu()               # the step's one read-back
                sels, toks = host[0].tolist(), host[1].tolist()
                self.last_generate_stats["contrastive_steps"] += 1
                keep_rows, nxt_live = [], []
                for j, b in enumerate(live):
                    self.last_generate_stats["pages_copied"] += groups[b].select(sels[j])
                    out_host[b, n_out] = toks[j]
                    if toks[j] not in a.eos:
                        keep_rows.append(j * k + sels[j])
                        nxt_live.append(b)
                n_out += 1
                scores = cur
                live = nxt_live
                stop = not live
                if not stop and stopping_criteria is not None:
                    stop = any(c(out_host[:, :n_out], scores) for c in stopping_criteria)    # StoppingCriteriaList: any()
                if stop:
                    break
                if step + 1 < max_new_tokens:
                    cur = logits[torch.tensor(keep_rows, dtype=torch.long).to(dev)]           # the chosen rows: the next current rows
        finally:
            for grp in groups.values():
                grp.release()
            for s in seqs:          # prompts no group took over (a failure before or inside the prefill)
                self.kv.release(s.pages)
                s.pages, s.length = [], 0
        return out_host[:, :n_out].to(dev)


VitronLlamaForCausalLM = LlavaLlamaForCausalLM  # name used by BASELINE.json's north_star; the reference class is LlavaLlamaForCausalLM
