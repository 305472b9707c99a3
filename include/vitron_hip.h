/* vitron_hip.h -- C ABI of libvitron_hip.so: the MI355X (gfx950) implementation of Vitron's multimodal
 * forward pass (LanguageBind ViT image/video tower -> region_extractor -> mm_projector -> Vicuna/LLaMA decoder).
 *
 * The reference (SkyworkAI/Vitron) has no FFI on this path: the boundary is the Python surface of
 * vitron.model. This ABI sits directly below that surface; vitron_amd/ binds it with
 * ctypes and keeps the reference's Python signatures. Each entry point names the reference code it replaces.
 *
 * Conventions
 *   - plain C, no torch types; every tensor is a raw DEVICE pointer owned by the caller (PyTorch's caching
 *     allocator in practice) and valid for the duration of the call. The library never allocates or frees
 *     tensor memory: scratch comes in as (workspace, workspace_bytes); query the size with *_workspace_bytes.
 *   - 16-bit tensors are uint16_t* (raw bits), row-major. Linear weights keep torch's [out][in] layout.
 *   - OPERAND FORMAT. The same sources are built twice with the same ABI: libvitron_hip.so computes with bf16 operands
 *     (BASELINE.json's dtype) and libvitron_hip_f16.so with IEEE fp16 operands -- the reference's own inference dtype
 *     (vitron/model/builder.py:47 torch_dtype=float16; towers :153,161). vt_operand_format() says which one a handle is.
 *     Wherever this header says "bf16" for a tensor (weights, activations, embeddings, K pages, pixel input, outputs) read
 *     "the library's operand format"; the historical names (vt_gemm_bf16, VT_EPI_BF16, VT_DTYPE_BF16) are kept for both.
 *     Everything else is identical in the two libraries: fp32 residual stream / accumulation / softmax statistics / biases,
 *     fp16 V^T pages and softmax weights. The fp16 library saturates operand stores at +-65504 (the reference would
 *     produce inf); bf16 weights of magnitude below 2^-14 lose mantissa bits when repacked to fp16 (absolute error <= 2^-25).
 *   - every function is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream),
 *     re-entrant, and returns 0 on success or a negative vt_status; vt_last_error() gives the message of the
 *     calling thread's last failure. Nothing throws, nothing synchronises the device.
 *   - ONE exception to "never allocates": the head_dim-128 prefill attention keeps, per (device, heads, query blocks, sequences)
 *     shape, its planned block-dispatch order in a small device buffer (heads * blocks * sequences int32) that it allocates the
 *     first time the shape is launched and uploads with hipMemcpyAsync on `stream` (no device synchronisation; other streams are
 *     ordered behind the upload by an event). A HIP graph capture must see a shape for the second time; vt_flash_attn_select(5)
 *     turns the planned order -- and with it the allocation -- off. All cached per-process state is keyed by device ordinal.
 *   - "host struct" arguments (vt_vit_model, vt_llama_model, ...) are read on the host during the call; the
 *     pointers inside them are device pointers.
 */
#ifndef VITRON_HIP_H
#define VITRON_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { VT_STATUS_OK = 0, VT_STATUS_ARG = -1, VT_STATUS_HIP = -2, VT_STATUS_WORKSPACE = -3 } vt_status;

/* GEMM epilogues: C = epi(A.W^T + bias) */
enum {
  VT_EPI_BF16 = 0,        /* bf16 out                                                                     */
  VT_EPI_BF16_GELU = 1,   /* bf16 out, exact-erf GELU   (CLIPMLP 'gelu', mm_projector nn.GELU)               */
  VT_EPI_BF16_QGELU = 2,  /* bf16 out, x*sigmoid(1.702x) (CLIPMLP 'quick_gelu')                              */
  VT_EPI_BF16_RELU = 3,   /* bf16 out, ReLU             (region_extractor MLP / LocationEncoder)            */
  VT_EPI_F32_RESID = 4,   /* fp32 C += A.W^T + bias      (residual stream accumulate)                        */
  VT_EPI_F32 = 5,         /* fp32 out                    (logits)                                            */
  VT_EPI_SWIGLU_BF16 = 6  /* W rows = [gate16|up16|gate16|up16...]; bf16 out [M][N/2] = silu(gate)*up          */
};
/* tile configurations of the MFMA GEMM (VT_GEMM_CFG_AUTO lets the library choose) */
enum {
  VT_GEMM_CFG_AUTO = 0,
  VT_GEMM_CFG_SKINNY = 1,   /* M <= 16 weight-streaming kernel (per-wave LDS-DMA ring -> MFMA, split-K inside the block) */
  VT_GEMM_CFG_128x128 = 2,
  VT_GEMM_CFG_256x128 = 3,
  VT_GEMM_CFG_256x256 = 4,
  VT_GEMM_CFG_64x128 = 5,
  VT_GEMM_CFG_256x256_P8 = 6, /* 256x256 tile, 8 waves, 8-phase pipelined main loop */
  /* 7: reserved (a 4-wave 128x128-register-tile experiment, slower than the 8-phase kernel; removed) */
  VT_GEMM_CFG_256x256_RP = 8, /* 256x256 tile, 8 waves, register-pipelined 32x32x16 main loop, one barrier per K tile */
  VT_GEMM_CFG_SKINNY_REG = 9, /* M <= 16: weight rows loaded straight into MFMA operand registers; fallback when K % 64 != 0 */
  VT_GEMM_CFG_256x256_P4 = 10, /* the 8-phase kernel with its phases merged pairwise: 32 MFMAs per section, half the barriers */
  /* 11: reserved (the 4-phase schedule on v_mfma_f32_32x32x16_bf16: correct, 25 % slower on every decoder shape; removed) */
  /* 12: reserved (2-phase schedule, one 64-MFMA section per K step: correct, 8 % slower than the 4-phase one; removed) */
  VT_GEMM_CFG_256x256_W4 = 13, /* 256x256 tile, 4 waves x (128x128), one wave per SIMD, K step placed by hand (plain-store epilogues) */
  VT_GEMM_CFG_320x256_W4 = 14, /* the same kernel on 320-row tiles (160x128 per wave): rows that fill whole rounds only this way */
  VT_GEMM_CFG_160x128_W4 = 15, /* four waves of 80x64 on a 160x128 tile, four-deep LDS ring: N = 1024 projections (K % 256 == 0) */
  VT_GEMM_CFG_224x256_W4 = 16, /* the four-wave kernel on 224-row tiles (112x128 per wave): row counts a little over a multiple of 224 (1088, 4616) */
};
enum { VT_DTYPE_BF16 = 0, VT_DTYPE_OP16 = 0 /* the 16-bit operand format of the library */, VT_DTYPE_F32 = 1 };
enum { VT_ACT_GELU = 0, VT_ACT_QUICK_GELU = 1 };

#define VT_PAGE_TOKENS 64 /* tokens per KV-cache page == keys per attention tile */

/* 114 also carries the FP8 KV cache entry points (vt_kv8_quant, vt_kv8_dequant, vt_attn_decode_kv8, vt_attn_decode_fused_kv8,
 * vt_llama_workspace_bytes_kv8, vt_llama_forward_kv8 and struct vt_kv_cache8) WITHOUT a bump: the change is purely additive -- new
 * symbols and one new struct, no existing struct gained a field, no existing function a parameter -- so every caller built against
 * the earlier 114 header keeps working unchanged. A caller that needs the new entry points looks the symbols up. */
/* 114 also carries vt_llama_model.last_layer_full and vt_attn_tail_desc WITHOUT a bump. The field sits in what was padding between
 * precise_qk (offset 88) and embeds_lo (offset 96): the struct's size and the offset of every earlier field are unchanged, and BOTH values
 * of the field select a correct pass (0 prunes the last layer of a prefill, anything else runs it on all rows as before), so a caller
 * built against the earlier 114 header keeps working whatever its padding holds. The rule: bump when an existing field moves, the size of
 * a struct changes or a function gains a parameter. */
/* 114 also carries the folded-norm unit entry points vt_gemm_bf16_norm, vt_gemm_bf16_resid_norm and vt_rowscale_finalize WITHOUT a bump:
 * three new symbols that forward to launches vt_llama_forward already makes; no struct and no existing signature changes. */
/* 114 also carries vt_sample_rows and struct vt_sample_row WITHOUT a bump: one new symbol and one new struct; vt_sample_top_p and
 * vt_argmax keep their signatures and return what they returned, bit for bit. */
/* 114 also carries vt_sample_rows_allow WITHOUT a bump: one new symbol; struct vt_sample_row and vt_sample_rows do not change. */
/* 114 also carries vt_beam_step, vt_beam_step_scratch_bytes and vt_kv_copy_pages WITHOUT a bump: three new symbols, no struct and no
 * existing signature changes. */
/* 114 also carries vt_ban_rows and struct vt_ban_row WITHOUT a bump: one new symbol and one new struct; the samplers do not change. */
/* 114 also carries vt_bias_rows, struct vt_bias_row and vt_sample_rows_adj WITHOUT a bump: two new symbols and one new struct; struct
 * vt_sample_row, vt_sample_rows and vt_sample_rows_allow do not change. */
/* 114 also carries the tower unit entry points vt_vit_embed, vt_region_pool and vt_attn_temporal_f32 WITHOUT a bump: three new symbols
 * that forward to launches vt_vit_forward and vt_region_forward already make; no struct and no existing signature changes. */
/* 114 also carries vt_sample_rows_trunc and struct vt_trunc_row WITHOUT a bump: one new symbol and one new struct; struct vt_sample_row,
 * vt_sample_rows, vt_sample_rows_allow and vt_sample_rows_adj do not change. */
/* 114 also carries vt_logprob_rows WITHOUT a bump: one new symbol, no struct and no existing signature changes; the samplers and
 * vt_beam_step do not change. */
/* 114 also carries vt_fsm_rows and struct vt_fsm_row WITHOUT a bump: one new symbol and one new struct; vt_ban_rows and the samplers do
 * not change. */
/* 114 also carries vt_cfg_rows and struct vt_cfg_row WITHOUT a bump: one new symbol and one new struct; vt_logprob_rows, vt_ban_rows,
 * vt_fsm_rows and the samplers do not change. */
/* 114 also carries vt_unit_rows, vt_contrast_rows and struct vt_contrast_row WITHOUT a bump: two new symbols and one new struct;
 * vt_logprob_rows and vt_kv_copy_pages do not change. */
/* 114 also carries vt_dola_rows and struct vt_dola_row WITHOUT a bump: one new symbol and one new struct; and two fields appended to the
 * END of struct vt_llama_model (logit_row_trace, logit_row_trace_layers), as hidden_trace was: a caller that zero-initialises the struct
 * gets the launches it got. */
/* 114 also carries vt_gemm_plan_query3 and vt_gemm_bf16_colsplit WITHOUT a bump: two new symbols, no struct and no existing signature
 * changes; vt_gemm_plan_query and vt_gemm_plan_query2 return what they returned, and vt_gemm_bf16 stores what it stored, bit for bit. */
/* 114 also carries vt_sample_rows_wm and struct vt_wm_row WITHOUT a bump (with vt_wm_cell_words): two new symbols and one new struct;
 * struct vt_sample_row, struct vt_trunc_row and the four vt_sample_rows* entry points do not change. */
/* 114 also carries vt_sample_rows_miro and struct vt_miro_row WITHOUT a bump: one new symbol and one new struct; struct vt_sample_row,
 * struct vt_trunc_row, struct vt_wm_row and the five vt_sample_rows* entry points do not change. */
#define VT_ABI_VERSION 114
int vt_version(void); /* == VT_ABI_VERSION of the header the library was built from */
/* operand format of THIS library (see Conventions): every uint16_t tensor argument carries these bits */
enum { VT_OPERAND_BF16 = 0, VT_OPERAND_FP16 = 1 };
int vt_operand_format(void);
/* copies the calling thread's last error message (NUL terminated) into buf; returns its length */
int vt_last_error(char* buf, size_t buf_len);

/* ------------------------------------------------------------------------------------------------------------
 * Primitive operators (exported for unit parity tests and for composing other models)
 * ---------------------------------------------------------------------------------------------------------- */

/* nn.Linear: C = epi(A[M,K] . W[N,K]^T + bias[N]).  bias may be NULL. C is bf16 or fp32 per `epi`.
 * `row_scale` (optional, fp32 [M], device): the accumulator of row m is multiplied by row_scale[m] before bias and activation
 * -- a per-row scalar commutes with the contraction, so a GEMM on x .* w followed by this factor is Linear(RMSNorm(x)) with the
 * normalisation folded in (what vt_llama_forward does for rows > 64). Rows with a scale run on the MFMA tile kernels whatever M
 * is. NULL = no scaling.
 * Replaces every torch.nn.Linear on the path (transformers-4.31 CLIPAttention/CLIPMLP/LlamaAttention/LlamaMLP,
 * reference call sites modeling_video.py:69,71,81; llava_llama.py:49,91-102; multimodal_projector/builder.py:33-51). */
int vt_gemm_bf16(const uint16_t* A, int lda, const uint16_t* W, int ldw, void* C, int ldc, const float* bias, int M,
                 int N, int K, int epi, int cfg, const float* row_scale, void* stream);

/* Which tile configuration vt_gemm_bf16(.., cfg = VT_GEMM_CFG_AUTO, row_scale = NULL) runs for this shape and epilogue (host logic
 * only, no launch): *cfg = the VT_GEMM_CFG_* of the first launch, *rows_first = 0 when that launch covers all M rows, else the
 * number of leading rows it covers (the remaining rows are planned again, as a GEMM of their own). Introspection for tests and
 * tools; no reference counterpart (torch.nn.Linear hides cuBLAS's heuristics the same way). */
int vt_gemm_plan_query(int M, int N, int K, int epi, int* cfg, int* rows_first);
/* the same with the column split of round 5: *cols_first > 0 means columns [0, *cols_first) run on *cfg (whole rounds of 256-row tiles) and the
 * remaining columns are planned again (a few row blocks x many column tiles that spill just over whole rounds: 768 x 22016) */
int vt_gemm_plan_query2(int M, int N, int K, int epi, int* cfg, int* rows_first, int* cols_first);
/* the plan the dispatcher RUNS, with the mixed-height column split: *cols_first > 0 means columns [0, *cols_first) run on *cfg -- any of the
 * 256-, 320- or 224-row four-wave configurations, whole rounds of it -- and the remaining columns on *cfg_rest (the first configuration of
 * their own plan). *cfg_rest = VT_GEMM_CFG_AUTO without a column split. vt_gemm_plan_query and _query2 keep reporting the plan without that
 * split, whose first launch is always on 256-row tiles: on the shapes where it applies (gate/up at 5120, 2560 and 768 rows) they name the
 * plan that ran before, this query names the two launches that run now. */
int vt_gemm_plan_query3(int M, int N, int K, int epi, int* cfg, int* rows_first, int* cols_first, int* cfg_rest);

/* vt_gemm_bf16 (row_scale = NULL) as two launches over column ranges, whatever the planner would do: columns [0, cols_first) on cfg_first,
 * columns [cols_first, N) on cfg_rest (VT_GEMM_CFG_AUTO: planned as a GEMM of their own). cols_first: a multiple of 256 inside (0, N); each
 * range must be legal for its configuration (the four-wave tiles: K % 128 == 0, K >= 256, N % 32 == 0). The result is the single launch's
 * bit for bit. The dispatcher's own column splits run through the same code; exported for tests and tools. */
int vt_gemm_bf16_colsplit(const uint16_t* A, int lda, const uint16_t* W, int ldw, void* C, int ldc, const float* bias, int M, int N, int K,
                          int epi, int cfg_first, int cols_first, int cfg_rest, void* stream);

/* y_bf16[rows][D] = LayerNorm(x_f32) * gamma + beta. If temb != NULL first x[row] += temb[(row / tokens_per_frame) % T]
 * (written back): the video tower's temporal_embedding add (reference modeling_video.py:110-114) fused with
 * temporal_layer_norm1 (:117). */
int vt_layernorm(float* x, const float* temb, int T, int tokens_per_frame, const float* gamma, const float* beta,
                 uint16_t* y, int rows, int D, float eps, void* stream);

/* y_bf16[r] = w * x[idx ? idx[r] : r] * rsqrt(mean(x^2) + eps) : transformers-4.31 LlamaRMSNorm. */
int vt_rmsnorm(const float* x, const int* idx, const float* w, uint16_t* y, int rows, int D, float eps, void* stream);

/* ---- the RMSNorm folded into the decoder's 16-bit GEMMs, as vt_llama_forward runs it (no reference counterpart: the reference calls
 * LlamaRMSNorm and nn.Linear separately; W (w .* x) * rstd == W (x * rstd .* w)). Exported for unit parity tests.
 * Decode flavour (1 <= M <= 16, N % 32 == 0, K % 64 == 0; epi = VT_EPI_BF16 / F32 / F32_RESID / SWIGLU_BF16; no bias), the tail as vt_gemm_nf4:
 *   consumer (in_partials != NULL, fp32 [M][in_n], in_n % 64 == 0, in_n <= 512): row m is scaled by
 *   rsqrt(sum(in_partials[m][0..in_n)) * inv_dim + eps) before the activation;
 *   producer (out_partials != NULL, VT_EPI_F32_RESID only): also out_xw[m][n] = op16(x_new * out_w[n]) and out_partials[m][n / 16] = the sum
 *   of x_new^2 over each 16 columns. NULL pointers = no fold. */
int vt_gemm_bf16_norm(const uint16_t* A, int lda, const uint16_t* W, int ldw, void* C, int ldc, int M, int N, int K, int epi,
                      const float* in_partials, int in_n, float inv_dim, float eps, const float* out_w, uint16_t* out_xw, int ld_xw,
                      float* out_partials, void* stream);
/* Tile flavour, producer: C[M,N] (fp32) += A W^T + bias on the MFMA tile kernels (N % 32 == 0, K % 64 == 0), which also store
 * out_xw[m][n] = op16(x_new * out_w[n]) (ld_xw % 4 == 0) and out_partials[n / 32][m] = the sum of x_new^2 over each 32 columns (group-major:
 * out_np >= N / 32 groups of out_ldp >= M floats). ksplit < 0: vt_gemm_bf16's dispatcher with the configuration `cfg` (AUTO or one of the
 * 128x128 / 256x128 / 256x256 / 64x128 / 256x256_P8 / 256x256_P4 tiles); ksplit >= 0: the residual GEMM's route with its split-K workspace, as
 * vt_gemm_bf16_resid_splitk (cfg ignored; when K is split the reduce pass writes out_xw and out_partials). */
int vt_gemm_bf16_resid_norm(const uint16_t* A, int lda, const uint16_t* W, int ldw, float* C, int ldc, const float* bias, int M, int N, int K,
                            int cfg, int ksplit, float* workspace, size_t workspace_bytes, const float* out_w, uint16_t* out_xw, int ld_xw,
                            float* out_partials, int out_np, int out_ldp, void* stream);
/* Tile flavour, between producer and consumer: out[m] = rsqrt(sum_g partials[g][m] * inv_dim + eps), g < np, m < rows (partials fp32
 * [np][ldp], ldp >= rows) -- the row_scale of the consuming vt_gemm_bf16. */
int vt_rowscale_finalize(const float* partials, int np, int ldp, int rows, float inv_dim, float eps, float* out, void* stream);

/* ---- NF4 weight-only Linears: load_pretrained_model(..., load_4bit=True) (reference vitron/model/builder.py:36-45: bitsandbytes
 * BitsAndBytesConfig(load_in_4bit=True, bnb_4bit_quant_type="nf4", bnb_4bit_compute_dtype=float16)), restated from bitsandbytes' algorithm:
 *   - the weight W [N][K] (K % 64 == 0) is taken as fp16 (an fp32 or operand-format source is rounded to fp16 first), in blocks of 64
 *     consecutive elements of a row; absmax[b] = fp32 max |x| of block b; x * (1.0f / absmax) goes to the NF4 code whose bitsandbytes
 *     midpoints (dQuantizeNF4) it lies strictly above; an all-zero block stores absmax 0 and code 7 (0.0) everywhere;
 *   - codes uint8 [N][K/2]: element 2j in the HIGH nibble of byte j, 2j+1 in the low one; absmax fp32 [N][K/64] (bitsandbytes' layout);
 *   - dequantised weight = op16(fp32(NF4[code]) * absmax) -- in the fp16 library bit-equal to bitsandbytes' fp16 dequantisation;
 *   - DEVIATION: absmax stays exact fp32. The reference also sets bnb_4bit_use_double_quant=True (absmax 8-bit quantised); not done here.
 * The GEMM reads this layout as it is (there is no separate kernel layout). */
int vt_nf4_quant(const void* W, int src_dtype /* VT_DTYPE_OP16 | VT_DTYPE_F32 */, int ldw, int N, int K, uint8_t* codes, float* absmax,
                 void* stream);
/* W [N][ldw] op16 = dequant(codes, absmax) */
int vt_nf4_dequant(const uint8_t* codes, const float* absmax, int N, int K, uint16_t* W, int ldw, void* stream);
/* C = epi(A[M,K] . dequant(W)[N,K]^T), fp32 accumulation, the weights streamed once at 4 bits and dequantised in registers (never a 16-bit copy):
 * 1 <= M <= 32, N % 32 == 0, K % 128 == 0; epi = VT_EPI_BF16 / VT_EPI_F32 / VT_EPI_F32_RESID (C += ...) / VT_EPI_SWIGLU_BF16 (W rows interleaved
 * in blocks of 16, C [M][N/2]). The folded RMSNorm of the decode step, as in vt_llama_forward:
 *   consumer (in_partials != NULL): row m is scaled by rsqrt(sum(in_partials[m][0..in_n)) * inv_dim + eps) (in_n % 16 == 0);
 *   producer (out_partials != NULL, VT_EPI_F32_RESID only): also out_xw[m][n] = op16(x_new * out_w[n]) and out_partials[m][n / 16] = the sum
 *   of x_new^2 over each 16 columns. NULL pointers = no fold. */
int vt_gemm_nf4(const uint16_t* A, int lda, const uint8_t* codes, const float* absmax, void* C, int ldc, int M, int N, int K, int epi,
                const float* in_partials, int in_n, float inv_dim, float eps, const float* out_w, uint16_t* out_xw, int ld_xw,
                float* out_partials, void* stream);

/* ---- precise level 3: the rounding remainder of a GEMM's A operand on the MX-FP4 pipe (no reference counterpart: the reference computes
 * every Linear in ONE 16-bit format, vitron/model/builder.py:47; north_star's 1e-3 against its fp32 CPU path is what these serve) ----------
 * A Linear of level 3 is  C = epi(A.W^T + (A4 2^ea).(W4 2^ew)^T + bias): A = op16(v) against the 16-bit weights on the 16-bit MFMA, plus
 * A4 = the MX-FP4 image (OCP e2m1 elements, power-of-two block scales) of lo = v - f32(A) against the weights' MX-FP4 image on
 * v_mfma_scale_f32_16x16x128_f8f6f4, in ONE launch and one fp32 accumulator.
 *   W4   uint8 [N][K/2]: element k of row n in byte k/2 (even k in bits 3:0);  wexp uint8 [N]: one biased (e8m0) exponent per row
 *   A4   uint8 [M][K/2]: same element order;  aexp uint8 [vt_mx4_aexp_bytes(M, K)]: one biased exponent per row and 32 consecutive k, at
 *        aexp[((m / 64) * (K / 32) + kb) * 64 + (m % 16) * 4 + (m % 64) / 16]  (the order the GEMM's lanes fetch them; rows padded to 256)
 * Quantisation: scale 2^e with the smallest e for which the block's largest magnitude is <= 6, elements to the nearest e2m1 value
 * {0, .5, 1, 1.5, 2, 3, 4, 6}, ties to the even mantissa (oracle/vitron_oracle.py mx4_quant restates it; tests compare bit for bit). */
size_t vt_mx4_aexp_bytes(int M, int K);
/* weights (K % 8 == 0) */
int vt_mx4_quant_weights(const uint16_t* W, int ldw, int N, int K, uint8_t* W4, uint8_t* wexp, void* stream);
/* a 16-bit remainder lo [M][K] (the second output of the precise level 2 operators), K % 32 == 0 */
int vt_mx4_quant_lo(const uint16_t* lo, int ld, int M, int K, uint8_t* A4, uint8_t* aexp, void* stream);
/* vt_rmsnorm with the level 3 operand out: y = op16(v), (A4, aexp) = MX-FP4 image of v - f32(y); D % 512 == 0 */
int vt_rmsnorm_mx(const float* x, const int* idx, const float* w, uint16_t* y, uint8_t* A4, uint8_t* aexp, int rows, int D, float eps,
                  void* stream);
/* the GEMM: 256 x 256 tiles of the four-wave kernel, K % 128 == 0, K >= 256, N % 4 == 0; epi = VT_EPI_BF16 / _GELU / _QGELU / F32_RESID /
 * F32 / SWIGLU_BF16 */
int vt_gemm_mx(const uint16_t* A, int lda, const uint8_t* A4, const uint8_t* aexp, const uint16_t* W, int ldw, const uint8_t* W4,
               const uint8_t* wexp, void* C, int ldc, const float* bias, int M, int N, int K, int epi, void* stream);

/* gate/up of level 3: C [M][N/2] = op16(v), v = silu(gate) * up over the 16-interleaved columns, and (out4 [M][N/4], oexp) = the MX-FP4 image of
 * v - f32(C) -- down_proj's second operand, written by the same launch. N % 128 == 0. */
int vt_gemm_mx_swiglu(const uint16_t* A, int lda, const uint8_t* A4, const uint8_t* aexp, const uint16_t* W, int ldw, const uint8_t* W4,
                      const uint8_t* wexp, uint16_t* C, int ldc, uint8_t* out4, uint8_t* oexp, int M, int N, int K, void* stream);
/* the towers' fc1 in their precise level 1: C [M][N] = op16(v), v = gelu(acc + bias) (quick = 0: erf form, 1: x sigmoid(1.702 x)), and
 * (out4 [M][N/2], oexp) = the MX-FP4 image of v - f32(C) -- fc2's second operand. N % 64 == 0. */
int vt_gemm_mx_gelu(const uint16_t* A, int lda, const uint8_t* A4, const uint8_t* aexp, const uint16_t* W, int ldw, const uint8_t* W4,
                    const uint8_t* wexp, const float* bias, uint16_t* C, int ldc, uint8_t* out4, uint8_t* oexp, int M, int N, int K, int quick,
                    void* stream);
/* vt_layernorm (without the temporal-embedding add) with the level 3 operand out, as vt_rmsnorm_mx; D % 256 == 0 */
int vt_layernorm_mx(const float* x, const float* gamma, const float* beta, uint16_t* y, uint8_t* A4, uint8_t* aexp, int rows, int D, float eps,
                    void* stream);
/* x += A.W^T + A4.W4^T (o_proj, down_proj of level 3). A grid that spills a fraction of a round over whole rounds of the chip's 256
 * multiprocessors runs its trailing row blocks as K ranges on the idle ones (fp32 partial slabs in `partials`, then an ordered reduce);
 * partials may be NULL (one plain launch). */
int vt_gemm_mx_resid(const uint16_t* A, int lda, const uint8_t* A4, const uint8_t* aexp, const uint16_t* W, int ldw, const uint8_t* W4,
                     const uint8_t* wexp, float* C, int ldc, int M, int N, int K, float* partials, size_t partial_bytes, void* stream);
/* vt_flash_attn (causal, head_dim 128, dense output: ldo == heads * 128) that also writes (O4 [rows][heads * 64], oexp) = the MX-FP4 image of
 * the output's rounding remainder -- o_proj's second operand in level 3. */
int vt_flash_attn_mx(const uint16_t* Q, int ldq, const uint16_t* k_tiles, const uint16_t* vt_tiles, const int* tile_table,
                     const int* seq_desc, int nseq, int max_q_len, uint16_t* O, int ldo, uint8_t* O4, uint8_t* oexp, int heads, float scale,
                     void* stream);

/* Attention over 64-key tiles. seq_desc: device int32 [nseq][4] = {q_row0, q_len, kv_len, table_off};
 * tile_table: device int32, tile_table[table_off + t] = index of the sequence's t-th K / V^T tile.
 * K tile = [64 keys][HD] bf16, V^T tile = [HD][64 keys] holding IEEE fp16 bits (the bf16 values of the projection converted
 * exactly, saturating at +-65504: the P.V product of the prefill kernel runs on the f16 MFMA with P at 11 mantissa bits; only
 * vt_kv_tiles / vt_attn_decode_fused / the fused QKV epilogue write these tiles); tile i of head h starts at (i*heads + h)*64*HD
 * elements.
 * q_len > 1 anywhere -> MFMA flash kernel (causal: query i sees keys <= kv_len - q_len + i); all q_len == 1 is
 * routed to the single-query kernel by vt_llama_forward. Replaces CLIPAttention (non-causal, modeling_video.py:136-146)
 * and LlamaAttention's softmax(QK^T/sqrt(d) + mask)V (reference restatement: llama_flash_attn_monkey_patch.py:30-66). */
int vt_flash_attn(const uint16_t* Q, int ldq, const uint16_t* k_tiles, const uint16_t* vt_tiles, const int* tile_table,
                  const int* seq_desc, int nseq, int max_q_len, uint16_t* O, int ldo, int heads, int head_dim,
                  int causal, float scale, void* stream);
/* Which prefill kernel vt_flash_attn (and the composite operators) run for head_dim 128 -- a process-wide switch for A/B measurements
 * and for the tests that hold the kernels to each other; results are the same contract either way. 0 = automatic (the one-wave-per-SIMD
 * kernel on 256-row blocks once heads x sequences x blocks fills the 256 CUs, else the two-waves-per-SIMD kernel on 128-row blocks),
 * 1 = always the two-waves-per-SIMD kernel, 2 = always the one-wave-per-SIMD kernel, 3 = that kernel with its pipeline stages run one
 * after the other instead of the hand-placed schedule (its reference), 4 = the one-wave-per-SIMD kernel in its persistent form (one
 * workgroup per CU walking the block list, K / V^T stream running on across block seams; `kernel = 4 | (n << 8)` caps it at n
 * workgroups -- a test hook that forces many blocks per workgroup). The persistent form keeps its block tickets in device globals:
 * one launch of it at a time per library (launches on one stream are ordered). 5 = kernel 2 dispatched in the grid's natural block order
 * instead of the planned one (next entry). No reference counterpart. */
int vt_flash_attn_select(int kernel);
/* Host logic only (no device work): the order in which a CAUSAL launch of the one-wave-per-SIMD kernel hands its (head, 256-row block,
 * sequence) blocks to the hardware dispatcher. order[i] = head + heads * (y + q_blocks * sequence) for workgroup i, y = 0 the last (heaviest)
 * block of a sequence. The dispatcher gives workgroup i to the first CU that frees up, so the order IS the schedule: the natural order
 * (heaviest first) is LPT; for a single long sequence a bin packing at a target makespan + "list by planned start time" ends 2.9 % above
 * the mean CU load instead of 11.8 % (S = 5120, 32 heads, 256 CUs). Planned per XCD (entry i runs on XCD i % 8 and only names heads = i mod
 * 8). Returns the number of entries written (heads * q_blocks * nseq), or 0 when the natural order is kept (one round, very many blocks, or
 * a plan that does not beat it by 2 % under the cost model). No reference counterpart. */
int vt_flash_attn_block_order(int heads, int q_blocks, int nseq, int multiprocessors, int* order, int capacity);
/* Residual GEMM C[M,N] (fp32) += A[M,K] W[N,K]^T + bias with an optional split-K workspace: when the 256x256 tile grid would
 * cover at most half of the chip (M ~ 1000 rows at N = 4096, the ViT's N = 1024 projections) the K loop is split over up to 8
 * workgroups per tile, fp32 partial products go to `partials` and a second kernel adds them in split order (deterministic).
 * ksplit: 0 = decide (may not split), >= 2 = force; partial_bytes >= ksplit*M*N*4 when it splits. */
int vt_gemm_bf16_resid_splitk(const uint16_t* A, int lda, const uint16_t* W, int ldw, float* C, int ldc, const float* bias,
                              int M, int N, int K, int ksplit, float* partials, size_t partial_bytes, void* stream);

/* One decode step's attention in one launch (every sequence has q_len == 1; kv_len counts the new token): rotary
 * embedding of the new q/k rows (rope tables may be NULL), append of the new k row / v column to the paged tiles (a tile
 * that starts with the new token is zero-filled around it), single-query attention over the cache. qkv is not modified.
 * Equivalent to vt_kv_tiles + vt_attn_decode; replaces LlamaAttention's cached single-token step
 * (transformers 4.31 LlamaAttention.forward as called from vitron/model/language_model/llava_llama.py:91-102). */
int vt_attn_decode_fused(const uint16_t* qkv, int ldqkv, int q_col0, int k_col0, int v_col0, uint16_t* k_tiles,
                         uint16_t* vt_tiles, const int* tile_table, const int* seq_desc, int nseq, uint16_t* O, int ldo,
                         int heads, int head_dim, float scale, const float* rope_cos, const float* rope_sin,
                         const int* positions, void* stream);

/* single-query (q_len == 1) attention, split over the KV tiles; scratch >= vt_attn_decode_scratch_bytes(...) */
size_t vt_attn_decode_scratch_bytes(int nseq, int heads, int head_dim, int max_kv_len);
int vt_attn_decode(const uint16_t* Q, int ldq, const uint16_t* k_tiles, const uint16_t* vt_tiles, const int* tile_table,
                   const int* seq_desc, int nseq, uint16_t* O, int ldo, int heads, int head_dim, float scale,
                   int max_kv_len, void* scratch, size_t scratch_bytes, void* stream);
/* fused-QKV rows -> K tiles / V^T tiles for the NEW tokens of each sequence; when rope_cos != NULL applies the
 * half-split rotary embedding (tables [rope_len][HD/2] fp32, row = positions[row]) to k and, in place, to q.
 * Replaces apply_rotary_pos_emb + the torch.cat KV-cache append of transformers-4.31 LlamaAttention. */
int vt_kv_tiles(uint16_t* qkv, int ldqkv, int q_col0, int k_col0, int v_col0, uint16_t* k_tiles, uint16_t* vt_tiles,
                const int* tile_table, const int* seq_desc, int nseq, int max_new_tiles, int heads, int head_dim,
                const float* rope_cos, const float* rope_sin, const int* positions, void* stream);
/* The single-query problems of the pruned last layer (vt_llama_model.last_layer_full == 0): out [n][4] int32, one descriptor per logit
 * row r = logit_rows[i] of the sequence s that holds it: {q_row0 = i, q_len = 1, kv_len = kv_len_s - (q_row0_s + q_len_s - 1 - r),
 * table_off = table_off_s} -- the keys row r sees in the causal pass. Rows in any order, repeats allowed; a row of no sequence gets kv_len 0.
 * All pointers are device pointers; nothing is read on the host. */
int vt_attn_tail_desc(const int* seq_desc, int nseq, const int* logit_rows, int n, int* out, void* stream);
/* temporal attention of the video tower: qkv bf16 [B*T*N][3*heads*64] (row (b*T+t)*N+n, q pre-scaled) ->
 * out bf16 [B*T*N][heads*64]; attends over the T frames at each (b, n). Reference modeling_video.py:105-127. */
int vt_attn_temporal(const uint16_t* qkv, uint16_t* out, int B, int T, int N, int heads, void* stream);
/* The same attention on fp32 q | k | v (the pair projection of vt_vit_model.precise >= 2; vt_vit_forward's own launch, exported for unit
 * tests): qkv fp32 [B*T*N][ld], ld >= 3*heads*64, columns q | k | v; everything in fp32; the output as an operand pair: out = the
 * 16-bit rounding of o, out_lo = the 16-bit rounding of o - out, both [B*T*N][heads*64]. T in 1..8. */
int vt_attn_temporal_f32(const float* qkv, int ld, uint16_t* out, uint16_t* out_lo, int B, int T, int N, int heads, void* stream);

/* CLIPVisionEmbeddings assembly + pre_layrnorm (vt_vit_forward's own launch, exported for unit tests): with R = G2 + 1 rows per frame,
 * x[f*R] = LN(cls + pos[0]) and x[f*R + 1 + p] = LN(patch_out[f*G2 + p] + pos[1 + p]), LN over D with gamma g, beta b and eps. All fp32:
 * patch_out [F*G2][D], cls [D], pos [R][D], g / b [D], x [F*R][D]. D % 4 == 0, D <= 4096; rows 16-byte aligned. */
int vt_vit_embed(const float* patch_out, const float* cls, const float* pos, const float* g, const float* b, float* x, int F, int G2,
                 int D, float eps, void* stream);

/* CLIPVisionEmbeddings patch gather: pixels ([F][3][H][W] or, video_layout=1, [B][3][T][H][W]; bf16 or fp32) ->
 * patches bf16 [B*T*(H/P)*(W/P)][k_pad], K order (c,py,px), zero padded. */
int vt_im2col(const void* pixels, int pix_dtype, uint16_t* patches, int B, int T, int H, int W, int P, int k_pad,
              int video_layout, void* stream);

/* Pre-processing of decoded frames on the device, fused: short-side resize to S (bicubic = torchvision tensor Resize,
 * reference image/processing_image.py:15-25; bilinear = pytorchvideo ShortSideScale, video/processing_video.py:45-53),
 * centre crop SxS, *1/255 for uint8 sources, (x - mean) / std, optional horizontal flip.
 * src: F frames, [F][H][W][3] (hwc=1) or [F][3][H][W]; uint8 (src_u8=1) or fp32. mean/std: HOST float[3].
 * dst element (c, f, y, x) at c*dst_stride_c + f*dst_stride_f + y*S + x  (images: sc=S*S, sf=3*S*S; clips [3][T][S][S]:
 * sc=T*S*S, sf=S*S); bf16 or fp32. */
int vt_preprocess(const void* src, int src_u8, int hwc, int F, int H, int W, int bicubic, int S, const float* mean,
                  const float* std, int flip, void* dst, int dst_dtype, long dst_stride_c, long dst_stride_f, void* stream);

/* embed_tokens gather + visual / region splice (reference llava_arch.py:306-398, 479-558).
 * plan: device int32 [rows][2] = {kind, index}; kind 0 = token id, 1 = row of vis, 2 = row of reg, 3 = zero row.
 * tok_table has `vocab` rows, vis `vis_rows`, reg `reg_rows` (0 with a NULL table): an index outside its table gives a
 * zero row instead of an out-of-bounds read (the host mirror raises before it gets that far). */
int vt_embed_splice(const uint16_t* tok_table, int vocab, const uint16_t* vis, int vis_rows, const uint16_t* reg, int reg_rows,
                    const int* plan, int rows, int H, uint16_t* out, void* stream);

/* greedy next token: first index of the row maximum (GenerationMixin greedy search). */
int vt_argmax(const float* logits, int rows, int V, int ldl, int* out_ids, void* stream);

/* Decode-loop feedback, one launch per generated token (the body of GenerationMixin's sampling loop that
 * model.generate runs between two forward passes, reference app.py:562-571 / inference_image.py:60-70 via
 * transformers; here without the host round trip). For every sequence i < nseq:
 *   t = finished[i] ? pad_id : next_ids[i];  finished[i] |= (t in eos_ids[0..n_eos));
 *   tokens_out[i] = t;  tokens_out[nseq + i] = finished[i];          (int32 [2][nseq], for the asynchronous read-back)
 *   x[i][0..H) = tok_table[t][0..H)                                  (input row of the next vt_llama_forward)
 *   seq_desc[i].kv_len += 1;  positions[i] += 1                      (device-side step metadata of that pass)
 * so the next decoder pass can be enqueued before the host has seen the token. */
int vt_decode_feed(const uint16_t* tok_table, int H, int vocab, const int* next_ids, int* finished, const int* eos_ids, int n_eos,
                   int pad_id, int* tokens_out, uint16_t* x, int* seq_desc, int* positions, int nseq, void* stream);
/* Mean cross entropy over the rows whose label is not `ignore_index`: loss[0] = mean_r(logsumexp(logits[r]) - logits[r][labels[r]]).
 * The caller shifts (row r scores the token at position r + 1). row_nll: fp32 scratch [rows] (per-row losses, -1 = skipped).
 * Replaces the CrossEntropyLoss of LlamaForCausalLM.forward when `labels` are passed (reference llava_llama.py:91-102). */
int vt_cross_entropy(const float* logits, int rows, int V, int ldl, const int* labels, int ignore_index, float* row_nll,
                     float* loss, void* stream);

/* one sampled token per row, the warper chain of GenerationMixin.sample in transformers' order: logits / temperature,
 * TopKLogitsWarper (top_k > 0: everything below the k-th largest value is removed, ties stay; 0 = off), softmax,
 * TopPLogitsWarper keep-set (top_p >= 1 keeps all), inverse-CDF draw with a counter-based uniform of (seed, step, row).
 * kept_count (optional) = size of the final keep-set per row.
 * Replaces GenerationMixin.sample's temperature / top-k / top-p / multinomial step (reference app.py:562-571, do_sample=True). */
int vt_sample_top_p(const float* logits, int rows, int V, int ldl, float temperature, int top_k, float top_p, uint64_t seed,
                    uint64_t step, int* out_ids, int* kept_count, void* stream);

/* One token per row with PER-ROW parameters, one launch: greedy and sampled rows, rows of different requests, in one batch.
 * params: DEVICE array of `rows` vt_sample_row (48 bytes each, 8-byte aligned; the offsets are part of the ABI):
 *    0 float    temperature         > 0 samples (TemperatureLogitsWarper); 0 -- anything not > 0 -- is a greedy row
 *    4 float    top_p               TopPLogitsWarper; >= 1 keeps all
 *    8 int32    top_k               TopKLogitsWarper; <= 0 is off
 *   12 float    repetition_penalty  RepetitionPenaltyLogitsProcessor; 1 is off
 *   16 uint64   seed                \
 *   24 uint64   counter              > the uniform is splitmix64(seed ^ splitmix64(counter * 0x632be59bd9b4e019 + stream)): the roles of
 *   44 uint32   stream              /  vt_sample_top_p's (seed, step, row index), so its draw can be reproduced from any batch position
 *   32 const int* history           DEVICE token ids the penalty applies to (may be NULL)
 *   40 int32    history_len         <= 0: no history
 * Per row, in transformers' order (LogitsProcessorList, then the warpers of GenerationMixin.sample, 4.31):
 *   1. penalty: every DISTINCT id of history with 0 <= id < V:  x = x < 0 ? x * penalty : x / penalty  (fp32, correctly rounded divide:
 *      torch's fp32 result bit for bit). Ids outside [0, V) -- the negative image / region sentinels of a multimodal prompt, ids of a
 *      larger vocabulary -- are skipped and index nothing.
 *   2. greedy row: out_ids = first index of the maximum of the penalised row (vt_argmax's answer on that row), kept_count = 1.
 *      sampled row: exactly vt_sample_top_p's arithmetic on the penalised row with the row's temperature, top_k, top_p and uniform.
 *   3. logprob (optional) = raw[id] - (max(raw) + logf(sum expf(raw - max))) over the RAW row (before penalty and temperature): the
 *      chosen token's log_softmax, without a [rows][V] copy to the host.
 * The kernel is total: no field value leads to an out-of-bounds access (history must be readable for history_len ints when both are set).
 * kept_count, logprob: optional [rows]. V <= 32768 with 16-byte aligned rows runs with the row in registers; anything else streams the row
 * and needs V <= VT_SAMPLE_ROWS_MAX_V (its V-bit history mask lives in LDS); a larger V is refused with a message.
 * 114 carries this entry point WITHOUT a bump: one new symbol and one new struct, nothing existing changes (see the note at VT_ABI_VERSION). */
#define VT_SAMPLE_ROWS_MAX_V 262144
typedef struct vt_sample_row {
  float temperature;
  float top_p;
  int32_t top_k;
  float repetition_penalty;
  uint64_t seed;
  uint64_t counter;
  const int* history;
  int32_t history_len;
  uint32_t stream;
} vt_sample_row;
int vt_sample_rows(const float* logits, int rows, int V, int ldl, const vt_sample_row* params, int* out_ids, int* kept_count,
                   float* logprob, void* stream);

/* vt_sample_rows with a PER-ROW ALLOW MASK: which token ids a row may emit at all (constrained decoding; the role of transformers'
 * SuppressTokens / BeginSuppressTokens / MinNewTokensLength / single-token NoBadWords / PrefixConstrained logits processors, which all
 * write -inf at the ids they forbid).
 * allow: DEVICE array of `rows` device pointers (8-byte aligned); allow[r] points to ceil(V / 32) uint32 words, or is NULL.
 *   Word / bit layout: token i may be chosen iff bit (i & 31) of word (i >> 5) is set. Bits at positions >= V in the last word are
 *   ignored. A NULL entry means every token of that row is allowed. A mask must be readable for ceil(V / 32) words; no word outside
 *   [0, ceil(V / 32)) and no logit outside the row is read.
 * A token whose bit is clear is treated as if its logit were -inf in steps 1 and 2 of the vt_sample_rows contract (-inf is unchanged by
 * the penalty and by the temperature; the mask is applied before the row maximum and the top-k threshold are computed). out_ids and
 * kept_count are bit-equal to what vt_sample_rows returns on a copy of the logits with -inf written at the banned positions; that also
 * defines a row with nothing allowed (what an all -inf row returns). Step 3 is unchanged: logprob stays raw[id] - logsumexp(raw) over
 * the RAW row, banned positions included.
 * allow == NULL behaves exactly like vt_sample_rows (the same launch). The argument checks, the two forms and VT_SAMPLE_ROWS_MAX_V are
 * vt_sample_rows's; the mask stays in global memory in both forms.
 * 114 carries this entry point WITHOUT a bump: one new symbol, nothing existing changes (see the note at VT_ABI_VERSION). */
int vt_sample_rows_allow(const float* logits, int rows, int V, int ldl, const vt_sample_row* params,
                         const uint32_t* const* allow /* DEVICE array of `rows` device pointers, entries may be NULL */,
                         int* out_ids, int* kept_count, float* logprob, void* stream);

/* HISTORY-DEPENDENT BANS: the allow mask of every row's COMING pick, built on the device from what the row has seen so far,
 * in front of vt_sample_rows_allow (the role of transformers' NoRepeatNGramLogitsProcessor and of NoBadWordsLogitsProcessor with
 * multi-token entries, which both write -inf at ids that depend on input_ids). Nothing is read on the host.
 * rows: DEVICE array of n_rows vt_ban_row (48 bytes each, 8-byte aligned; the offsets are part of the ABI):
 *    0 const int32_t*  history      DEVICE ids seen so far (prompt, then generated); may be NULL
 *    8 const uint32_t* base         DEVICE allow mask to start from, ceil(V / 32) words; NULL = every id of [0, V) allowed
 *   16 uint32_t*       out          DEVICE mask to write, ceil(V / 32) words; NULL = this row is skipped entirely
 *   24 const int32_t*  seqs         DEVICE ban sequences, flattened as {L, id_0 .. id_{L-1}} repeated; may be NULL
 *   32 int32_t         history_len  <= 0: empty history
 *   36 int32_t         ngram        no_repeat_ngram_size; <= 0 is off
 *   40 int32_t         n_seqs
 *   44 int32_t         seqs_len     ints readable at seqs
 * Word / bit layout: vt_sample_rows_allow's (token i is bit (i & 31) of word (i >> 5)). Per row, with h = history[0 .. n):
 *   - out starts as a copy of base, words copied as they are (bits at positions >= V included). With base NULL it starts with the bits
 *     [0, V) set and the bits >= V of the last word clear. After that bits are only ever cleared.
 *   - n-gram rule (ngram = g >= 1, n >= g - 1): for every i in [0, n - g + 1), if h[i .. i + g - 2] == h[n - g + 1 .. n - 1] the bit of
 *     h[i + g - 1] is cleared. Plain int32 equality: the negative image / region sentinels of a multimodal prompt take part like any other
 *     id (as they do in the processor, which sees the reference's own input_ids). g == 1 bans every id of h.
 *   - sequence rule, for every sequence s of length L: L == 1 clears the bit of s[0]; L >= 2 with n >= L - 1 and
 *     h[n - L + 1 .. n - 1] == s[0 .. L - 2] clears the bit of s[L - 1].
 *   - an id to clear outside [0, V) is skipped and indexes nothing. A malformed seqs (an L <= 0, an entry that runs past seqs_len) ends
 *     the parsing of that row's sequences; the sequences before it count.
 * The kernel is total: no field value leads to an access outside history[0 .. history_len), seqs[0 .. seqs_len) or the ceil(V / 32)
 * words of base and out (history and seqs must be readable for those lengths when set); words of a larger buffer behind out are not
 * touched. out must NOT alias base or another row's out. The result does not depend on the order of the clears: it is deterministic.
 * Refused with VT_STATUS_ARG and a message before any launch: V <= 0, V > VT_SAMPLE_ROWS_MAX_V, n_rows < 0, rows == NULL with n_rows > 0.
 * n_rows == 0 is a success that launches nothing. One launch, one 1024-thread block per row: the mask is built in LDS (atomicAnd) and
 * written once.
 * 114 carries this entry point WITHOUT a bump: one new symbol and one new struct, nothing existing changes (see the note at VT_ABI_VERSION). */
typedef struct vt_ban_row {
  const int32_t* history;
  const uint32_t* base;
  uint32_t* out;
  const int32_t* seqs;
  int32_t history_len;
  int32_t ngram;
  int32_t n_seqs;
  int32_t seqs_len;
} vt_ban_row;
int vt_ban_rows(const vt_ban_row* rows /* DEVICE */, int n_rows, int V, void* stream);

/* TOKEN AUTOMATA: guided decoding. A row carries a state of a finite automaton over token ids; the state decides which
 * ids the row's COMING pick may be, the ids the row has emitted move the state. Built on the device in front of vt_sample_rows_allow, as
 * vt_ban_rows is (the role of transformers' PrefixConstrainedLogitsProcessor and of vLLM's / outlines' guided decoding by regex or by
 * choices). Nothing is read on the host.
 * rows: DEVICE array of n_rows vt_fsm_row (96 bytes each, 8-byte aligned; the offsets are part of the ABI):
 *    0 const int32_t*  gen          DEVICE ids this row has GENERATED so far (not the prompt); NULL = gen_len counts as 0
 *    8 int32_t*        cell         DEVICE two int32 {state, consumed}, read and written; NULL = this row is skipped entirely
 *   16 const uint32_t* base         DEVICE allow mask to intersect with, ceil(V / 32) words; NULL = every id of [0, V)
 *   24 uint32_t*       out          DEVICE mask to write, ceil(V / 32) words; NULL = this row is skipped entirely
 *   32 const int32_t*  offsets      DEVICE [n_states + 1]: state s lists the edges [offsets[s], offsets[s + 1]); NULL = n_states counts as 0
 *   40 const int32_t*  edge_tok     DEVICE [n_edges] token ids, ascending and unique inside each state; NULL = n_edges counts as 0
 *   48 const int32_t*  edge_next    DEVICE [n_edges] next state of the edge, or -1 = this token is forbidden here; NULL = n_edges counts as 0
 *   56 const int32_t*  state_info   DEVICE [n_states][2] = {default_next, accept}; NULL = n_states counts as 0
 *   64 int32_t         gen_len      ids readable at gen; <= 0: none
 *   68 int32_t         n_states
 *   72 int32_t         n_edges
 *   76 int32_t         n_eos        clamped into [0, 4]
 *   80 int32_t         eos[4]       the row's EOS ids, eos[0 .. n_eos)
 * Word / bit layout: vt_sample_rows_allow's (token i is bit (i & 31) of word (i >> 5)).
 * step(s, t), with plain int32 equality throughout:
 *   - s outside [0, n_states) gives -1 (dead).
 *   - the edges of s are the indices [lo, hi) with lo = offsets[s] and hi = offsets[s + 1] clamped into [0, n_edges] (hi not below lo).
 *     If t == edge_tok[j] for one of them (found by binary search: the ids must ascend) the result is edge_next[j].
 *   - else, if t is one of eos[0 .. n_eos): s when accept[s] != 0, and -1 otherwise. A default edge never covers an EOS id.
 *   - else default_next[s].
 *   - any result outside [0, n_states) is -1.
 * Advance: consumed = max(cell[1], 0); for i in [consumed, gen_len): state = step(state, gen[i]), starting from state = cell[0]; then
 *   cell = {state, max(consumed, gen_len)} (a state that consumed nothing is written back as it was). Launching the same row twice
 *   therefore advances once (the launch is idempotent) and a row whose cell is k ids behind catches up.
 * Mask: token t of [0, V) is allowed iff step(state after the advance, t) >= 0; out = (base, or the bits [0, V) when base is NULL) AND
 *   allowed. Bits at positions >= V of the last word are CLEAR whatever base holds there. A dead state yields an all-zero mask (what
 *   the sampler returns for a row with nothing allowed is defined at vt_sample_rows_allow).
 * The kernel is total: no field value leads to an access outside gen[0 .. gen_len), the two ints of cell, offsets[0 .. n_states],
 * edge_tok / edge_next[0 .. n_edges), state_info[0 .. 2 * n_states) or the ceil(V / 32) words of base and out (the inputs must be
 * readable for those lengths when set); words of a larger buffer behind out are not touched. out must NOT alias base or another row's
 * out; two rows must not share a cell. Edge ids that do not ascend, or that repeat inside a state, give a mask and a step that need not
 * agree with each other, and nothing worse. The result does not depend on the order of the LDS atomics: it is deterministic.
 * Refused with VT_STATUS_ARG and a message before any launch: V <= 0, V > VT_SAMPLE_ROWS_MAX_V, n_rows < 0, rows == NULL with n_rows > 0.
 * n_rows == 0 is a success that launches nothing. One launch, one 1024-thread block per row: one thread advances the state, the mask is
 * built in LDS (from ones under a default edge, else from zeros; atomicOr / atomicAnd per listed edge) and written once.
 * 114 carries this entry point WITHOUT a bump: one new symbol and one new struct, nothing existing changes (see the note at VT_ABI_VERSION). */
typedef struct vt_fsm_row {
  const int32_t* gen;
  int32_t* cell;
  const uint32_t* base;
  uint32_t* out;
  const int32_t* offsets;
  const int32_t* edge_tok;
  const int32_t* edge_next;
  const int32_t* state_info;
  int32_t gen_len;
  int32_t n_states;
  int32_t n_edges;
  int32_t n_eos;
  int32_t eos[4];
} vt_fsm_row;
int vt_fsm_rows(const vt_fsm_row* rows /* DEVICE */, int n_rows, int V, void* stream);

/* ADDITIVE ADJUSTMENTS: logit_bias / single-token sequence_bias and the presence / frequency penalties (the role of
 * transformers' SequenceBiasLogitsProcessor and of the OpenAI / vLLM penalties). A row's adjustment `adj` is V pairs (pre, post) of fp32:
 * adj[2t] = pre[t], adj[2t + 1] = post[t]. The value the sampler uses for token t, every arithmetic step rounded to fp32 separately (no
 * fused multiply-add anywhere):
 *     x = raw[t];  if the allow bit of t is clear: x = -inf                       (vt_sample_rows_allow)
 *     x = x + pre[t]                                                              (logit_bias / sequence_bias)
 *     if t is in the penalty history and penalty != 1: x = x < 0 ? x * penalty : x / penalty     (vt_sample_rows step 1, bit for bit)
 *     x = x + post[t]                                                             (presence / frequency)
 * -- transformers runs SequenceBiasLogitsProcessor in front of RepetitionPenaltyLogitsProcessor; vLLM applies logit_bias, then the
 * repetition penalty, then frequency and presence. Everything after that (greedy pick, temperature, top-k, top-p, the draw, kept_count)
 * is vt_sample_rows_allow's arithmetic on x. logprob stays raw[id] - logsumexp(raw) over the RAW row.
 *
 * vt_bias_rows builds the adjustments on the device, nothing is read on the host. rows: DEVICE array of n_rows vt_bias_row (48 bytes
 * each, 8-byte aligned; the offsets are part of the ABI):
 *   @0  const int32_t* history      DEVICE ids the counts are taken over: the tokens the row has GENERATED so far (not the prompt); may be NULL
 *   @8  const int32_t* bias_ids     DEVICE, n_bias distinct ids; may be NULL
 *   @16 const float*   bias_vals    DEVICE, n_bias values
 *   @24 float*         out          DEVICE fp32 [V][2] to write; NULL = this row is skipped entirely
 *   @32 int32_t        history_len  <= 0: empty history
 *   @36 int32_t        n_bias       <= 0: none (also when bias_ids or bias_vals is NULL)
 *   @40 float          presence
 *   @44 float          frequency
 * Per row:
 *   - pre[t] = bias_vals[j] if bias_ids[j] == t for some j < n_bias, else 0.0f. Ids outside [0, V) are skipped and index nothing. The
 *     caller guarantees distinct ids; with a duplicate one of its values lands and nothing else is affected.
 *   - post[t], with c = the number of i < history_len with history[i] == t:  c == 0 ? 0.0f : -(frequency * (float)c + presence), the
 *     product and the sum rounded separately. History ids outside [0, V) are skipped. Counting is over generated tokens only (OpenAI's
 *     and vLLM's definition); the repetition penalty keeps its own prompt + reply history in vt_sample_row.
 *   - counts are 16-bit integers in LDS: a row with history_len > 65535 counts its LAST 65535 entries only. Integer counts make the
 *     result independent of the order of the atomics: it is deterministic.
 * The kernel is total: no field value leads to an access outside history[0 .. history_len), bias_ids / bias_vals[0 .. n_bias) or the
 * 2 * V floats of out (the inputs must be readable for those lengths when set); floats of a larger buffer behind out are not touched.
 * out must NOT alias another row's out. An out that is 8-byte aligned is written with 8-byte stores.
 * Refused with VT_STATUS_ARG and a message before any launch: V <= 0, V > VT_BIAS_ROWS_MAX_V, n_rows < 0, rows == NULL with n_rows > 0.
 * n_rows == 0 is a success that launches nothing. One launch, one 1024-thread block per row: the counts live in dynamic LDS sized by V
 * (two 16-bit counters per word, 128 KiB at the limit, plus V bits).
 * 114 carries these entry points WITHOUT a bump: two new symbols and one new struct, nothing existing changes (see the note at VT_ABI_VERSION). */
#define VT_BIAS_ROWS_MAX_V 65536
typedef struct vt_bias_row {
  const int32_t* history;
  const int32_t* bias_ids;
  const float* bias_vals;
  float* out;
  int32_t history_len;
  int32_t n_bias;
  float presence;
  float frequency;
} vt_bias_row;
int vt_bias_rows(const vt_bias_row* rows /* DEVICE */, int n_rows, int V, void* stream);

/* vt_sample_rows_allow with a PER-ROW ADJUSTMENT, applied as stated above.
 * adjust: DEVICE array of `rows` device pointers (8-byte aligned); adjust[r] points to fp32 [V][2] (8-byte aligned, what vt_bias_rows
 *   writes), or is NULL: no adjustment for that row. No float outside the 2 * V of a row's adjustment is read.
 * adjust == NULL is the vt_sample_rows_allow launch itself (and with allow == NULL too, vt_sample_rows'). allow may be NULL with adjust
 * set. out_ids and kept_count are bit-equal to what vt_sample_rows_allow returns, with repetition_penalty 1, on a copy of the logits
 * holding the values x above. Both forms (row in registers; streaming), the argument checks and VT_SAMPLE_ROWS_MAX_V are
 * vt_sample_rows's; the adjustment stays in global memory in both forms. */
int vt_sample_rows_adj(const float* logits, int rows, int V, int ldl, const vt_sample_row* params,
                       const uint32_t* const* allow /* DEVICE array of `rows` device pointers, entries and the array may be NULL */,
                       const float* const* adjust /* DEVICE array of `rows` device pointers to fp32 [V][2], entries and the array may be NULL */,
                       int* out_ids, int* kept_count, float* logprob, void* stream);

/* vt_sample_rows_adj with PER-ROW TRUNCATION: transformers' MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper
 * and EtaLogitsWarper, which follow top-k and top-p in GenerationMixin's warper chain. trunc: DEVICE array of `rows` vt_trunc_row (16
 * bytes each, 4-byte aligned; the offsets are part of the ABI):
 *   @0  float min_p            active iff min_p > 0
 *   @4  float typical_p        active iff 0 < typical_p < 1
 *   @8  float epsilon_cutoff   active iff 0 < epsilon_cutoff < 1
 *   @12 float eta_cutoff       active iff 0 < eta_cutoff < 1
 * Anything else in a field (0, a negative value, NaN, a typical_p or a cutoff >= 1) means that stage is off. A row whose four stages
 * are off returns, bit for bit, the out_ids, kept_count and logprob vt_sample_rows_adj returns for it; a greedy row (temperature not
 * > 0) ignores its entry; trunc == NULL is the vt_sample_rows_adj launch itself.
 * The stages run on a sampled row after the top-k and top-p steps, in this order. A is the set of survivors so far and
 * q_i = exp(s_i) / sum_{j in A} exp(s_j) the softmax of the scaled, penalised, masked, adjusted logits s over A -- renormalised after
 * every stage, as every warper sees -inf at the ids removed before it:
 *   1. min_p: i leaves when q_i < min_p * max_A q. Tokens tied with the maximum of A stay.
 *   2. typical_p (mass m): H = -sum_A q log q, d_i = |-log q_i - H|; d* = the smallest of the d_i with sum_{d_j <= d*} q_j >= m; i
 *      stays when d_i <= d*. No such d*: all stay. This stage may remove the arg-max token.
 *   3. epsilon_cutoff: i leaves when q_i < epsilon_cutoff. Tokens tied with the maximum of the CURRENT A stay.
 *   4. eta_cutoff (e): H = the entropy over the current A, eta = min(e, sqrt(e) * exp(-H)); i leaves when q_i < eta. Tokens tied with
 *      the maximum of the current A stay.
 * kept_count is the size of the final A; the draw is vt_sample_rows' inverse CDF over the final A in index order, the row's uniform
 * scaled by the mass of A. logprob stays over the RAW row. The statistics are fp32 (one fast exponential and one fast logarithm per
 * token, tree sums); d* is found exactly among the fp32 d_i by bisection on their bit patterns. The kernel is total: no field value leads
 * to an access outside the row. Both forms, the argument checks and VT_SAMPLE_ROWS_MAX_V are vt_sample_rows's; trunc must be 4-byte
 * aligned.
 * 114 carries this entry point WITHOUT a bump: one new symbol and one new struct, nothing existing changes (see the note at VT_ABI_VERSION). */
typedef struct vt_trunc_row {
  float min_p;
  float typical_p;
  float epsilon_cutoff;
  float eta_cutoff;
} vt_trunc_row;
int vt_sample_rows_trunc(const float* logits, int rows, int V, int ldl, const vt_sample_row* params,
                         const uint32_t* const* allow /* DEVICE array of `rows` device pointers, entries and the array may be NULL */,
                         const float* const* adjust /* DEVICE array of `rows` device pointers to fp32 [V][2], entries and the array may be NULL */,
                         const vt_trunc_row* trunc /* DEVICE array [rows], or NULL */,
                         int* out_ids, int* kept_count, float* logprob, void* stream);

/* vt_sample_rows_trunc with a PER-ROW SYNTHID TEXT WATERMARK: transformers' SynthIDTextWatermarkLogitsProcessor
 * (SynthIDTextWatermarkingConfig; Dathathri et al., Nature 2024), which GenerationMixin runs last, behind every warper -- so it lives in
 * the sampler, behind the truncation stages. wm: DEVICE array of `rows` vt_wm_row (48 bytes each, 8-byte aligned; the offsets are part of
 * the ABI):
 *   @0  uint64_t* cell              DEVICE state of this sequence, vt_wm_cell_words(history_size) words; NULL: the row is not watermarked
 *   @8  const uint64_t* layer_add   DEVICE [depth]: k_i * M + 1 (mod 2^64) for key k_i, M = 6364136223846793005
 *   @16 const uint32_t* table       DEVICE bit array of the sampling table, table_size / 32 words, bit t = table[t]
 *   @24 int32_t depth               1..32 (the number of keys)
 *   @28 int32_t table_size          a power of two, 32..65536
 *   @32 int32_t ngram_len           2..8
 *   @36 int32_t history_size        1..4096 (context_history_size)
 *   @40 int32_t skip_first          skip_first_ngram_calls (0: off)
 *   @44 int32_t reserved            0
 * The cell, in uint64 words: [0] num_calls; [1] the head of the history ring; [2] the context hash of the last call; [3] the flags of
 * the last call (bit 0 watermarked, bit 1 repeated context, bit 2 skipped); [4..11) the context ids, ngram_len - 1 used; [12..) the
 * history ring. An all-zero cell is transformers' fresh SynthIDTextWatermarkState: the context holds GENERATED tokens only, zero-padded
 * at the start. Per sampled row with a cell, where p holds the kept probabilities of vt_sample_rows_trunc and `kept` their sum:
 *   1. num_calls += 1. With skip_first and num_calls < ngram_len the draw is vt_sample_rows_trunc's and the ring is not touched.
 *   2. H = the hash of the context: h <- (h + id) * M + 1 from h = 1, in wrapping 64-bit arithmetic.
 *   3. repeated = one of ALL history_size ring entries equals H (the zero entries of a fresh ring take part); then ring[head] = H,
 *      head = (head + 1) % history_size. A repeated context is drawn as vt_sample_rows_trunc draws it.
 *   4. otherwise q = p / kept and, for layer i in [0, depth): q_v *= 1 + g_iv - sum_v g_iv q_v, where g_iv is bit
 *      (((H + v) * M + 1 + k_i) * M + 1) mod table_size of the table -- fp32, tree sums, a token with q = 0 stays 0.
 *   5. the draw: vt_sample_rows' inverse CDF over q in index order, the row's uniform (seed, counter, stream) scaled by sum(q).
 *   6. an id >= 0 is shifted into the context -- on skipped and repeated calls too.
 * kept_count stays the truncation's survivors, logprob stays over the RAW row. A greedy row (temperature not > 0) ignores its entry and
 * does not touch its cell; a row whose cell is NULL returns, bit for bit, what vt_sample_rows_trunc returns for it (its other fields are
 * not read); wm == NULL is the vt_sample_rows_trunc launch itself. allow, adjust and trunc may each be NULL.
 * The register form only: with wm != NULL a launch that vt_sample_rows would run in the streaming form (V > 32768, ldl % 4 != 0, logits
 * not 16-byte aligned) is refused with VT_STATUS_ARG and a message. Refused likewise, before any launch: wm not 8-byte aligned, and for a
 * row with a cell a field outside its range, a table_size that is no power of two, reserved != 0, a NULL or misaligned layer_add / table.
 * For that the array is read back on `stream` in front of the launch (rows * 48 bytes and a wait for the copy); on a stream that is being
 * captured it is not, and the kernel treats such an entry as a row without a watermark. Nothing a cell can hold indexes out of bounds:
 * the head is reduced mod history_size, the context ids are data only.
 * 114 carries vt_sample_rows_wm and struct vt_wm_row WITHOUT a bump: two new symbols and one new struct, nothing existing changes (see
 * the note at VT_ABI_VERSION). */
#define VT_WM_MAX_DEPTH 32
#define VT_WM_MAX_TABLE 65536
#define VT_WM_MAX_NGRAM 8
#define VT_WM_MAX_HISTORY 4096
typedef struct vt_wm_row {
  uint64_t* cell;
  const uint64_t* layer_add;
  const uint32_t* table;
  int32_t depth;
  int32_t table_size;
  int32_t ngram_len;
  int32_t history_size;
  int32_t skip_first;
  int32_t reserved;
} vt_wm_row;
size_t vt_wm_cell_words(int history_size); /* 12 + history_size */
int vt_sample_rows_wm(const float* logits, int rows, int V, int ldl, const vt_sample_row* params,
                      const uint32_t* const* allow /* DEVICE array of `rows` device pointers, entries and the array may be NULL */,
                      const float* const* adjust /* DEVICE array of `rows` device pointers to fp32 [V][2], entries and the array may be NULL */,
                      const vt_trunc_row* trunc /* DEVICE array [rows], or NULL */,
                      const vt_wm_row* wm /* DEVICE array [rows], or NULL */,
                      int* out_ids, int* kept_count, float* logprob, void* stream);

/* vt_sample_rows_trunc with PER-ROW MIROSTAT v2: the adaptive truncation of Basu et al., "Mirostat: A Neural Text
 * Decoding Algorithm that Directly Controls Perplexity" (ICLR 2021), in the form of llama.cpp's mirostat_v2 sampler (`--mirostat 2`): a
 * cutoff mu on the surprise of a token moves after every pick so that the surprise of the emitted text stays near a target tau. It
 * stands behind the truncation stages. miro: DEVICE array of `rows` vt_miro_row (16 bytes each, 8-byte aligned; the offsets are part of
 * the ABI):
 *   @0  float* cell     DEVICE state of this sequence, two fp32 words {mu, last_surprise}, 8-byte aligned; NULL: the row runs no Mirostat
 *   @8  float tau       the target surprise in bits; <= 0 (or NaN): the row runs no Mirostat
 *   @12 float eta       the learning rate, >= 0
 * A fresh cell is {2 * tau, 0}, written by the host once; after that only the kernel writes it. Per sampled row with tau > 0 and a cell,
 * where p holds the kept probabilities of vt_sample_rows_trunc (0 elsewhere) and `kept` their sum:
 *   1. q_v = p_v / kept (p_v times the fp32 reciprocal of kept); s_v = -log2f(q_v) for q_v > 0 (the accurate log2f).
 *   2. token v survives iff s_v <= mu. The most probable kept token always survives: when its own surprise exceeds mu (or mu is a NaN)
 *      it is the only survivor, the first index on a tie (the (value, index) order of the greedy rows).
 *   3. kept2 = the sum of the surviving q_v; the draw is vt_sample_rows' inverse CDF over the survivors in index order, the row's
 *      uniform (seed, counter, stream) scaled by kept2. No new random number is drawn.
 *   4. e = -log2f(q_x / kept2) for the drawn id x (a correctly rounded divide), mu <- mu - eta * (e - tau) with the difference, the
 *      product and the last difference each rounded on its own (no fma); the cell becomes {mu, e}. This is the only write, by one
 *      thread, behind every read of the cell. A row that draws nothing (id < 0: nothing was kept) leaves its cell as it is.
 *   5. kept_count reports the survivors of step 2; logprob stays over the RAW row.
 * `kept` and kept2 are tree sums: 32 consecutive slots of a thread serially, 6 shuffle levels over a wave, then the 16 wave totals in
 * wave order; the maximum of step 2 is taken over the same tree. mu is data only: whatever a cell holds indexes nothing.
 * A greedy row (temperature not > 0) ignores its entry and does not touch its cell; a row with tau <= 0 or a NULL cell returns, bit for
 * bit, what vt_sample_rows_trunc returns for it; miro == NULL is the vt_sample_rows_trunc launch itself. allow, adjust and trunc may each
 * be NULL. llama.cpp skips top-k and top-p when Mirostat is on; here every stage in front keeps working, and a caller who wants
 * llama.cpp's behaviour leaves them off. Mirostat v1 and Mirostat together with the watermark (vt_sample_rows_wm) are not built.
 * The register form only: with miro != NULL a launch that vt_sample_rows would run in the streaming form (V > 32768, ldl % 4 != 0, logits
 * not 16-byte aligned) is refused with VT_STATUS_ARG and a message. Refused likewise, before any launch: miro not 8-byte aligned, and for
 * a row with a cell a cell that is not 8-byte aligned, a tau or eta that is not finite, eta < 0. For that the array is read back on
 * `stream` in front of the launch (rows * 16 bytes and a wait for the copy); on a stream that is being captured it is not, and the kernel
 * treats an entry it would have refused as a row without Mirostat.
 * 114 carries vt_sample_rows_miro and struct vt_miro_row WITHOUT a bump: one new symbol and one new struct, nothing existing changes (see
 * the note at VT_ABI_VERSION). */
typedef struct vt_miro_row {
  float* cell;
  float tau;
  float eta;
} vt_miro_row;
int vt_sample_rows_miro(const float* logits, int rows, int V, int ldl, const vt_sample_row* params,
                        const uint32_t* const* allow /* DEVICE array of `rows` device pointers, entries and the array may be NULL */,
                        const float* const* adjust /* DEVICE array of `rows` device pointers to fp32 [V][2], entries and the array may be NULL */,
                        const vt_trunc_row* trunc /* DEVICE array [rows], or NULL */,
                        const vt_miro_row* miro /* DEVICE array [rows], or NULL */,
                        int* out_ids, int* kept_count, float* logprob, void* stream);

/* BEAM SEARCH (the role of transformers' GenerationMixin beam search: log_softmax + running scores + torch.topk over
 * num_beams * vocab, and the cache reorder behind it).
 *
 * vt_beam_step: row g * beams_in + b of `logits` (fp32, row stride ldl >= V) belongs to beam b of group g. The candidate score of token t is
 *     s = (logits[r][t] - (m + logf(sum_i expf(logits[r][i] - m)))) + beam_scores[r],   m = the row maximum,   all in fp32
 * -- vt_sample_rows' logprob plus one addition. Per group the n_out largest candidates over all beams_in * V are written in descending
 * score: out_scores / out_tokens / out_beams, each [groups][n_out]. Exact ties are broken by the lower flat index b * V + t (this
 * library's rule; torch.topk promises none). Nothing is read on the host and `logits` is not modified. A row needs a finite maximum; a
 * NaN score is never selected, and a group with fewer than n_out selectable candidates ends with (-inf, -1, -1) entries.
 * Limits, refused with VT_STATUS_ARG before any launch: 1 <= beams_in <= 16, 1 <= n_out <= 32, n_out <= V, V <= VT_SAMPLE_ROWS_MAX_V.
 * scratch: vt_beam_step_scratch_bytes(groups, beams_in, n_out) bytes of device memory, 4-byte aligned (VT_STATUS_WORKSPACE when short).
 * Two launches: one 1024-thread block per row (log-sum-exp, then the row's own n_out best; up to 32 * 1024 columns the row is held in
 * registers, above that a thread re-reads its part of it when it looks for its next candidate), then one wave per group that merges the
 * beams_in * n_out survivors. */
size_t vt_beam_step_scratch_bytes(int groups, int beams_in, int n_out);
int vt_beam_step(const float* logits, int ldl, int V, int groups, int beams_in, const float* beam_scores /* [groups*beams_in] */,
                 int n_out, float* out_scores, int* out_tokens, int* out_beams /* each [groups][n_out] */,
                 void* scratch, size_t scratch_bytes, void* stream);

/* LOG-PROBABILITIES OF LOGIT ROWS (the role of torch.log_softmax + torch.topk + a gather on rows read back to the host).
 *
 * vt_logprob_rows: per row r of `logits` (fp32, row stride ldl >= V), over the RAW row -- no penalty, temperature or mask, as the samplers'
 * logprob output -- in one launch of one 1024-thread block per row; `logits` is only read:
 *     lse[r]         = m + logf(sum_i expf(x_i - m)),   m = max_i x_i,   all in fp32  (vt_sample_rows' expression; the summation order may
 *                      differ from the sampler's, so the two agree within their two bounds, not bit for bit)
 *     a token's log-probability is  x_t - lse[r]
 *     ORDER            a larger RAW logit comes first, exact ties go to the lower index. Selection compares x, never x - lse: it is exact.
 *     top_ids[r][p]  = the p-th token in that order, p < n_top;   top_lp[r][p] = its log-probability
 *     target_lp[r]   = the log-probability of target[r];   target_rank[r] = 1 + the number of tokens strictly ahead of target[r] in the
 *                      order (exact integer arithmetic; the best token has rank 1)
 * target == NULL, or target[r] outside [0, V): target_lp[r] = NaN, target_rank[r] = 0, and row[target[r]] is not read; when neither the
 * top lists (n_top == 0) nor lse are asked for either, the row is not read at all.
 * Edge rules:
 *   * a NaN logit is never taken and never counted as ahead. A row that holds one has lse = NaN, hence NaN log-probabilities everywhere; its
 *     top_ids still follow the order over the values that are not NaN. A target whose own logit is NaN stands behind every value that is not
 *     a NaN: its rank is 1 + their number.
 *   * -inf logits are ordinary candidates with log-probability -inf (+inf likewise: the row's lse is then +inf or NaN as IEEE gives it).
 *   * fewer than n_top takeable values (V < n_top, or NaNs): the remaining slots hold id -1 and a NaN log-probability.
 *   * total: no input value reaches an index unchecked, and nothing but the outputs named here is written.
 * lse, target_lp, target_rank may each be NULL (not written); top_ids / top_lp are [rows][n_top] and may be NULL when n_top == 0.
 * Refused with VT_STATUS_ARG and a message before any launch: logits == NULL, rows <= 0, V <= 0, V > VT_LOGPROB_MAX_V, ldl < V, n_top outside
 * [0, VT_LOGPROB_MAX_TOP], n_top > 0 with top_ids or top_lp NULL, n_top == 0 with lse, target_lp and target_rank all NULL, a pointer that is
 * not 4-byte aligned.
 * Two forms, chosen by the launcher: V <= 32 * 1024 with a 16-byte aligned base and ldl % 4 == 0 -- the row is read once, 32 values per
 * thread, and everything runs over registers; any other V or alignment -- a thread re-reads its part of the row (L2) for the sum, the count
 * and whenever it looks for its next candidate. No scratch memory and no workspace in either form.
 * 114 carries this entry point WITHOUT a bump: one new symbol, nothing existing changes (see the note at VT_ABI_VERSION). */
#define VT_LOGPROB_MAX_TOP 20
#define VT_LOGPROB_MAX_V (1 << 30)
int vt_logprob_rows(const float* logits, int rows, int V, int ldl,
                    const int* target /* DEVICE int32 [rows], or NULL */, int n_top /* 0 .. VT_LOGPROB_MAX_TOP */,
                    float* lse /* [rows] or NULL */, float* target_lp /* [rows] or NULL */, int* target_rank /* [rows] or NULL */,
                    int* top_ids /* [rows][n_top] */, float* top_lp /* [rows][n_top] */, void* stream);

/* CLASSIFIER-FREE GUIDANCE (the role of transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor -- guidance_scale /
 * negative_prompt_ids -- and of contrastive decoding: two torch.log_softmax and a blend over rows, five or six launches and three [B, V]
 * temporaries as torch ops). A row names the logits of the same step under two contexts; the guided row goes in front of every other
 * logits processor and of the samplers. Nothing is read on the host.
 * rows: DEVICE array of n_rows vt_cfg_row (56 bytes each, 8-byte aligned; the offsets are part of the ABI):
 *    0 const float*    cond         DEVICE conditional logit row, fp32 [V]; NULL = this row is skipped entirely, nothing is written
 *    8 const float*    uncond       DEVICE unconditional logit row, fp32 [V]
 *   16 float*          out          DEVICE guided row, fp32 [V]; MAY alias cond (in place); must NOT alias uncond
 *   24 const uint32_t* base         DEVICE allow mask to start from, ceil(V / 32) words; NULL = every id of [0, V) allowed
 *   32 uint32_t*       mask_out     DEVICE plausibility mask to write, ceil(V / 32) words; NULL = none is written
 *   40 float*          lse_out      DEVICE two floats {lse_c, lse_u}; NULL = not written
 *   48 fp32            scale        the guidance scale s
 *   52 fp32            log_beta     log(beta), computed on the host; -inf = no plausibility cut
 * Per row, everything in fp32, c = cond, u = uncond:
 *     lse_c = m_c + logf(sum_i expf(c_i - m_c)),  m_c = max_i c_i        (vt_logprob_rows' expression and reduction order; lse_u likewise)
 *     cl = c_i - lse_c;  ul = u_i - lse_u;  out_i = ul + s * (cl - ul)   -- the two subtractions, the inner subtraction, the product and
 *       the sum are each rounded to nearest on their own (no fused multiply-add anywhere), so out follows BIT FOR BIT from the inputs and
 *       the two values written to lse_out
 *     mask_out bit i = base bit i AND (c_i >= m_c + log_beta), i in [0, V)   (beta in (0, 1]: a token stays iff p_cond >= beta max p_cond)
 * Word / bit layout: vt_sample_rows_allow's (token i is bit (i & 31) of word (i >> 5)). Bits at positions >= V of the last word follow
 * vt_ban_rows: copied from base as they are, clear when base is NULL. A NaN c_i fails the comparison (its bit is clear); the maxima skip
 * NaNs (fmaxf) while the sums do not, so a row that holds a NaN has a NaN lse and a NaN guided row. +-inf and NaN propagate by IEEE
 * rules, nothing is special-cased (log_beta = -inf with m_c = +inf gives a NaN threshold, which clears every bit).
 * No value read from a row is used as an index. cond, uncond and out must be readable / writable for V floats and 4-byte aligned, base
 * and mask_out for ceil(V / 32) words; words and floats of larger buffers behind them are not touched. out must not alias another row's
 * input or output, mask_out must NOT alias base.
 * Refused with VT_STATUS_ARG and a message before any launch: rows == NULL, n_rows <= 0, V <= 0, V > VT_LOGPROB_MAX_V, rows not 8-byte
 * aligned.
 * One launch, one 1024-thread block per row, no workspace, no atomics. Two forms, chosen per ROW: V <= 32 * 1024 with cond, uncond and
 * out 16-byte aligned -- both rows are read once with 16-byte loads, 2 x 32 values per thread, and everything runs over registers; any
 * other V or alignment -- a thread re-reads its elements (L2) for the sums and again for the write. In place is safe in both: a thread
 * writes only elements it has read itself, after the block-wide reductions.
 * 114 carries this entry point WITHOUT a bump: one new symbol and one new struct, nothing existing changes (see the note at VT_ABI_VERSION). */
typedef struct vt_cfg_row {
  const float* cond;
  const float* uncond;
  float* out;
  const uint32_t* base;
  uint32_t* mask_out;
  float* lse_out;
  float scale;
  float log_beta;
} vt_cfg_row;
int vt_cfg_rows(const vt_cfg_row* rows /* DEVICE */, int n_rows, int V, void* stream);

/* DOLA (Chuang et al. 2023, "DoLa: Decoding by Contrasting Layers Improves Factuality in Large Language Models";
 * transformers 4.4x' generate(dola_layers=...): GenerationMixin._dola_decoding with _dola_select_contrast and _relative_top_filter). A
 * row names the final layer's logit row and n_cand rows of earlier layers' residual streams put through the bare lm_head; the kernel picks
 * the candidate whose distribution is furthest from the final one and writes the contrast of the two log-softmaxes, restricted to the
 * tokens the final layer finds plausible. It goes in front of every other logits processor and of the samplers. Nothing is read on the host.
 * rows: DEVICE array of n_rows vt_dola_row (80 bytes each, 8-byte aligned; the offsets are part of the ABI):
 *    0 const float*    final             DEVICE final-layer logit row, fp32 [V]; NULL = this row is skipped entirely, nothing is written
 *    8 const float*    prem              DEVICE candidate rows, fp32: candidate j is the V floats at prem + j * prem_stride
 *   16 float*          out               DEVICE contrasted row, fp32 [V]; MAY alias final (in place); must NOT overlap a candidate
 *   24 const uint32_t* base              DEVICE allow mask to start from, ceil(V / 32) words; NULL = every id of [0, V) allowed
 *   32 uint32_t*       mask_out          DEVICE mask of the kept tokens to write, ceil(V / 32) words; NULL = none is written
 *   40 int*            layer_out         DEVICE one int: the chosen candidate j*; NULL = not written
 *   48 float*          div_out           DEVICE n_cand floats: the divergences; NULL = not written
 *   56 float*          lse_out           DEVICE 1 + n_cand floats {lse_final, lse_0, ..}; NULL = not written
 *   64 int64           prem_stride       elements between candidates
 *   72 int             n_cand            1 .. VT_DOLA_MAX_LAYERS
 *   76 fp32            log_relative_top  log(relative_top), computed on the host; -inf = nothing is filtered
 * Per row, everything in fp32, f = final, x = candidate j:
 *     lse_f = m_f + logf(sum_i expf(f_i - m_f)),  m_f = max_i f_i      (vt_logprob_rows' expression and reduction order; lse_j likewise)
 *     lpf = f_i - lse_f;  lpj = x_i - lse_j;  M = 0.5 (expf(lpf) + expf(lpj))
 *     div_j = 0.5 * sum_i [ M (logf(M) - lpf) + M (logf(M) - lpj) ],  a term with M == 0 counting 0
 *       -- F.kl_div(input = log_softmax, target = the average distribution) summed, KL(M || p) twice: what transformers computes under the
 *       name of the Jensen-Shannon divergence; unbounded (a token with p_f = 0 < p_j contributes +inf). With n_cand == 1 no divergence
 *       is computed and div_out[0] = 0.
 *     j* = 0; for j = 1 .. n_cand - 1: if (div_j > div_j*) j* = j       -- the largest divergence; exact ties and NaNs go to the lower j
 *     keep_i = f_i >= m_f + log_relative_top                             -- _relative_top_filter with min_tokens_to_keep = 1 in vt_cfg_rows' form
 *     out_i = keep_i ? (f_i - lse_f) - (x*_i - lse_j*) : -inf            -- the three subtractions each rounded to nearest on their own,
 *       so out follows BIT FOR BIT from the inputs, lse_out[0], lse_out[1 + j*] and j*
 *     mask_out bit i = base bit i AND keep_i, i in [0, V); word / bit layout and the bits at positions >= V as in vt_cfg_rows
 * Two bitwise equal candidate rows of one row get bitwise equal lse and div (same form, same reduction order), so the tie rule is exact.
 * The maxima skip NaNs (fmaxf), the sums do not: a row that holds a NaN has NaN lse and NaN divergences (j* = 0), out is NaN where
 * keep_i holds and -inf elsewhere (a NaN f_i fails the comparison). +-inf propagate by IEEE rules, nothing is special-cased.
 * Bad row content: a live row whose n_cand is outside [1, VT_DOLA_MAX_LAYERS] reads and writes nothing except layer_out = -1 (when
 * given); the other rows of the launch are served.
 * No value read from a row is used as an index. final, out and every candidate must be readable / writable for V floats and 4-byte
 * aligned; floats and words of larger buffers behind them are not touched. mask_out must NOT alias base.
 * Refused with VT_STATUS_ARG and a message before any launch: rows == NULL, n_rows <= 0, V <= 0, V > VT_LOGPROB_MAX_V, rows not 8-byte
 * aligned.
 * One launch, one 1024-thread block per row, no workspace, no atomics. Two forms, chosen per ROW: V <= 32 * 1024 with final, prem and out
 * 16-byte aligned and prem_stride % 4 == 0 -- the final row stays in registers, every candidate is read once (the chosen one a second
 * time for the write); any other V or alignment -- a thread re-reads its elements (L2) for each reduction.
 * 114 carries this entry point WITHOUT a bump: one new symbol and one new struct, nothing existing changes (see the note at VT_ABI_VERSION). */
#define VT_DOLA_MAX_LAYERS 16
typedef struct vt_dola_row {
  const float* final;
  const float* prem;
  float* out;
  const uint32_t* base;
  uint32_t* mask_out;
  int* layer_out;
  float* div_out;
  float* lse_out;
  long long prem_stride;
  int n_cand;
  float log_relative_top;
} vt_dola_row;
int vt_dola_rows(const vt_dola_row* rows /* DEVICE */, int n_rows, int V, void* stream);

/* CONTRASTIVE SEARCH (Su et al. 2022, "A Contrastive Framework for Neural Text Generation"; transformers'
 * generate(penalty_alpha=, top_k=), whose contrastive_search / _ranking_fast are no longer part of its core). Each of a sequence's k most
 * probable next tokens is run as a decode row; its final hidden state is compared, by cosine similarity, with the final hidden state of
 * EVERY earlier position (the context bank, visual rows included); the candidate with the largest (1 - alpha) p - alpha max_j cos wins.
 *
 * vt_unit_rows: out[r][i] = op16(y_i * rnorm), y_i = w[i] * x[r][i] (w == NULL: y_i = x[r][i]), rnorm = 1 / sqrt(sum_i y_i^2), everything
 * in fp32 (the sum by fused multiply-adds), one rounding to the operand format at the store. A row whose sum is 0 gives zeros. With
 * w = the final RMSNorm weight and x = the fp32 stream behind the last layer this is the direction of the final-normed state: RMSNorm's
 * per-row scalar cancels in a cosine. x: fp32 [rows][ldx], out: operand format [rows][ldo], ldx, ldo >= H; `out` must not alias `x`.
 * Refused with VT_STATUS_ARG: x or out NULL, rows <= 0, H <= 0, ldx < H, ldo < H. One 256-thread block per row; H <= 4096 with 16-byte
 * aligned rows is read once, anything else twice. */
int vt_unit_rows(const float* x, int ldx, const float* w /* fp32 [H] or NULL */, uint16_t* out, int ldo, int rows, int H, void* stream);

/* vt_contrast_rows: rows is a HOST array of n_groups vt_contrast_row (64 bytes each; the offsets are part of the ABI), one per sequence.
 * It is read before the call returns and travels to the kernels by value: nothing is uploaded, and every field is checked first.
 *    0 uint16_t*       bank         DEVICE operand format [bank_cap][H], contiguous rows: the unit vectors of the context, rows [0, bank_len)
 *    8 const float*    cand_lp      DEVICE fp32 [k]: the candidates' log-probabilities, as vt_logprob_rows wrote them (top_lp)
 *   16 float*          d_out        DEVICE fp32 [k]
 *   24 float*          score_out    DEVICE fp32 [k]
 *   32 int*            sel_out      DEVICE int32 [1]
 *   40 int             bank_len     T: 1 <= T < bank_cap
 *   44 int             bank_cap     rows the bank holds
 *   48 int             k            candidates of this sequence, 1 <= k <= VT_CONTRAST_MAX_K
 *   52 int             first        its candidates are the rows [first, first + k) of cand
 *   56 fp32            alpha        in [0, 1]
 *   60 int             reserved     0
 * cand: DEVICE operand format [n_cand][ld] unit rows (vt_unit_rows), ld >= H, ld % 8 == 0, H % 32 == 0, 16-byte aligned.
 * Per group, c in [0, k):
 *     d[c]     = max_{j < T} dot(bank[j], cand[first + c])     fp32 accumulation of the exact products of the 16-bit values (MFMA)
 *     score[c] = fmaf(-alpha, d[c], t),  t = (1 - alpha) * __expf(cand_lp[c])     1 - alpha and t rounded to fp32 on their own
 *     sel      = the arg-max of those score values, exact ties to the lower c. sel starts at 0 and moves only on a strictly greater
 *                score: it lies in [0, k) whatever the inputs (inputs are expected finite)
 *     bank[T]  = cand[first + sel], bit for bit the vector that was compared: the bank grows on the device; bank_len is the caller's
 * Bank rows at and beyond T are never read; rows beyond T are not written. workspace: DEVICE, at least
 * VT_CONTRAST_WORKSPACE_BYTES(n_groups, the largest bank_len) bytes, 4-byte aligned; it holds the chunk maxima between the two stages.
 * Refused with VT_STATUS_ARG and a message before any launch: rows or cand NULL, n_groups <= 0, n_cand <= 0, H not a positive multiple of
 * 32, ld < H or ld % 8 != 0, cand misaligned, and per group: a NULL pointer, a misaligned bank, k outside [1, VT_CONTRAST_MAX_K],
 * bank_len < 1, bank_len >= bank_cap, [first, first + k) outside [0, n_cand), alpha outside [0, 1]; a workspace that is NULL or too small.
 * Two stages per 32 groups, no atomics: grid (chunks of VT_CONTRAST_CHUNK bank rows, groups) x 512 threads -- the chunk's rows are the
 * 16-row operand of v_mfma_f32_16x16x32_{bf16,f16}, the candidates its 16 columns, both loaded from global memory straight into the
 * fragments with 16-byte loads, K sliced over the 8 waves (80 VGPRs, no scratch, 9 KiB of LDS) -- then one 512-thread block per group:
 * maxima, scores, selection, append.
 * 114 carries these two entry points WITHOUT a bump: two new symbols and one new struct, nothing existing changes. */
#define VT_CONTRAST_MAX_K 16
#define VT_CONTRAST_CHUNK 16
#define VT_CONTRAST_WORKSPACE_BYTES(n_groups, max_bank_len) \
  ((size_t)(n_groups) * (size_t)(((max_bank_len) + VT_CONTRAST_CHUNK - 1) / VT_CONTRAST_CHUNK) * 16 * sizeof(float))
typedef struct vt_contrast_row {
  uint16_t* bank;
  const float* cand_lp;
  float* d_out;
  float* score_out;
  int* sel_out;
  int bank_len;
  int bank_cap;
  int k;
  int first;
  float alpha;
  int reserved;
} vt_contrast_row;
int vt_contrast_rows(const vt_contrast_row* rows /* HOST */, int n_groups, const uint16_t* cand, int n_cand, int ld, int H,
                     void* workspace, size_t workspace_bytes, void* stream);

/* vt_kv_copy_pages: for every layer and every i < n, page src_pages[i] is copied onto page dst_pages[i] in both the K pool and the V^T
 * pool (k / vt: [num_layers][num_pages][page_bytes] each). It counts in bytes -- page_bytes = heads * 64 * head_dim * element size, a
 * multiple of 16 -- so one kernel serves the 16-bit pool and the e4m3 pool. src_pages / dst_pages: DEVICE int32 [n]. n == 0 is a no-op that
 * returns OK. A pair with a page id outside [0, num_pages) is skipped on the device. The caller guarantees that no destination page is
 * also a source (beam.plan_beam_reorder). Grid (pair, layer, K | V^T), 16-byte loads and stores. */
int vt_kv_copy_pages(void* k, void* vt, int num_layers, int num_pages, size_t page_bytes /* heads*64*head_dim*element size */,
                     const int* src_pages, const int* dst_pages /* device int32 [n] */, int n, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * mm_projector: Linear(Din,Dh) -> GELU(erf) -> Linear(Dh,Dout)   ('mlp2x_gelu';  w2 == NULL -> 'linear')
 * reference vitron/model/multimodal_projector/builder.py:33-51, called at llava_arch.py:175,186
 * ---------------------------------------------------------------------------------------------------------- */
size_t vt_projector_workspace_bytes(int M, int Dh);
/* precise level 2 (mlp2x_gelu only): features in and embeddings out as operand pairs (x + x_lo, out + out_lo: hi = op(v), lo = op(v - hi)),
 * both Linear layers as A_hi.W^T + A_lo.W^T in fp32, GELU on the fp32 value. reference multimodal_projector/builder.py:40-46 */
size_t vt_projector_precise_workspace_bytes(int M, int Dh, int Dout);
int vt_projector_forward_precise(const uint16_t* x, const uint16_t* x_lo, int M, int Din, const uint16_t* w1, const float* b1, int Dh,
                                 const uint16_t* w2, const float* b2, int Dout, uint16_t* out, uint16_t* out_lo, void* workspace,
                                 size_t workspace_bytes, void* stream);
int vt_projector_forward(const uint16_t* x, int M, int Din, const uint16_t* w1, const float* b1, int Dh,
                         const uint16_t* w2, const float* b2, int Dout, uint16_t* out, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * region_extractor (reference vitron/model/region_extractor/layer.py:58-130), one box per image.
 *   feats   bf16 [B][G*G][D]      patch features of the image tower (pre-projector)
 *   slices  int32 [B][4]          {row_start,row_stop,col_start,col_stop} = Python slice(int(x1),int(x2)) /
 *                                  slice(int(y1),int(y2)) resolved against image_size on the host (x -> rows, :83)
 *   coords  fp32 [B][4]           raw box {x1,y1,x2,y2} (LocationEncoder input, :126; fp32 so that canvas coordinates above 256,
 *                                  which bf16 cannot hold, reach the K = 4 layer unrounded -- the reference casts them to the
 *                                  model dtype, where fp16 holds integers to 2048)
 *   mlp_w[2]/mlp_b[2]             first two layers of region_linear (D->H, H->H, ReLU after each; layer.py:17-20)
 *   loc_w0 / loc_b0               LocationEncoder layer 0, bf16 [H/2][8] (zero padded from [H/2][4]) / fp32 [H/2]
 *   final_w / final_b             [H][H + H/2] = [ region_linear.layers.2.weight | loc_encoder.2.weight ] and the SUM of their
 *                                  biases: MLP output + location embedding (layer.py:129) is one contraction over the
 *                                  concatenated K, accumulated in fp32 and rounded to bf16 once
 *   out     bf16 [B][H]; cell_mask int32 [B][G*G] and cell_count int32 [B] are optional outputs (may be NULL)
 *   B <= 16 per call, G <= 64. Four launches: pool (+ mask, count, LocationEncoder layer 0) and three weight-streaming GEMMs.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct vt_region_weights {
  int in_dim, out_dim;
  const uint16_t* mlp_w[2];
  const float* mlp_b[2];
  const uint16_t* loc_w0;
  const float* loc_b0;
  const uint16_t* final_w;
  const float* final_b;
} vt_region_weights;
size_t vt_region_workspace_bytes(int B, int in_dim, int out_dim);
int vt_region_forward(const vt_region_weights* w, const uint16_t* feats, const int* slices, const float* coords,
                      int B, int G, int image_size, uint16_t* out, int* cell_mask, int* cell_count, void* workspace,
                      size_t workspace_bytes, void* stream);
/* The first launch of vt_region_forward on its own (exported for unit tests; any B >= 1: the 16-box limit belongs to the GEMMs that
 * follow): feats / slices / coords as above with D = in_dim (D % 64 == 0), G <= 64, image_size >= G.
 *   pooled     16-bit [B][D]       masked mean of the box's cells, sum_cells x * fl32(1 / count) in fp32; an empty box gives zeros
 *   cell_mask  int32 [B][G*G], cell_count int32 [B]: optional (may be NULL), bit-exact
 *   loc_out    16-bit [B][ld_loc]  optional: columns 0 .. loc_n - 1 of row b = relu(coords[b] . loc_w0[n][0..3] + loc_b0[n]) with
 *                                  loc_w0 16-bit [loc_n][8] and loc_b0 fp32 [loc_n]; the D / 64 channel slabs of a box share the
 *                                  loc_n outputs, ceil(loc_n / slabs) each. NULL skips the layer (coords / loc_w0 / loc_b0 unused). */
int vt_region_pool(const uint16_t* feats, const int* slices, int B, int G, int image_size, int D, uint16_t* pooled, int* cell_mask,
                   int* cell_count, const float* coords, const uint16_t* loc_w0, const float* loc_b0, int loc_n, uint16_t* loc_out,
                   int ld_loc, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * LanguageBind ViT tower (CLIP ViT + optional per-layer temporal attention)
 * reference CLIPVisionTransformer.forward / CLIPEncoderLayer.forward
 *   vitron/model/multimodal_encoder/languagebind/video/modeling_video.py:65-158,596-675 (image twin: image/modeling_image.py)
 * and the tower wrappers' feature_select (languagebind/__init__.py:96-121,182-204): the library runs `num_layers`
 * encoder layers (= n_hidden + 1 + select_layer, 23 of 24 for select_layer = -2) and returns the patch tokens
 * (CLS dropped) of that hidden state.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct vt_vit_layer {
  /* temporal block -- all NULL unless add_time_attn */
  const float *t_ln_g, *t_ln_b;
  const float* t_embed;   /* [num_frames][D]; NULL when num_frames == 1 (reference skips the add, :110) */
  const uint16_t* t_wqkv; /* [3D][D], q rows pre-scaled by head_dim^-0.5 */
  const float* t_bqkv;    /* [3D], q part pre-scaled */
  const uint16_t* t_wo;
  const float* t_bo;
  /* spatial block */
  const float *ln1_g, *ln1_b;
  const uint16_t* wqkv;
  const float* bqkv;
  const uint16_t* wo;
  const float* bo;
  const float *ln2_g, *ln2_b;
  const uint16_t* w1; /* fc1 [I][D] */
  const float* b1;
  const uint16_t* w2; /* fc2 [D][I] */
  const float* b2;
  /* temporal MLP -- the IMAGE tower's add_time_attn variant only (reference image/modeling_image.py:83-84,129-134: after the temporal
     attention, x += temporal_mlp(temporal_layer_norm2(x))); all NULL for the video tower (video/modeling_video.py has no such block) */
  const float *t_ln2_g, *t_ln2_b;
  const uint16_t* t_w1;
  const float* t_b1;
  const uint16_t* t_w2;
  const float* t_b2;
  /* precise level 1 only, else NULL: MX-FP4 images of fc1 / fc2 (vt_mx4_quant_weights) and their per-row exponents -- with them the MLP runs
     as two launches of vt_gemm_mx's kernel (hidden % 256 == 0, intermediate % 128 == 0); without them level 1 falls back to 16-bit operand pairs */
  const uint8_t* w14; const uint8_t* w1_e;
  const uint8_t* w24; const uint8_t* w2_e;
} vt_vit_layer;

typedef struct vt_vit_model {
  int image_size, patch, hidden, heads, intermediate;
  int num_layers;    /* encoder layers to run */
  int num_frames;    /* T of the temporal attention (config.num_frames) */
  int add_time_attn; /* 1 = video tower */
  int act;           /* VT_ACT_* */
  float ln_eps;
  int k_pad;               /* padded K of the patch GEMM (multiple of 64, >= 3*patch*patch) */
  const uint16_t* w_patch; /* [D][k_pad] */
  const float* cls;        /* [D] */
  const float* pos;        /* [G*G+1][D] */
  const float *pre_ln_g, *pre_ln_b;
  const vt_vit_layer* layers; /* host array [num_layers] */
  int precise;             /* 2: precise level 2 -- EVERY GEMM A operand of the tower travels as an operand pair (hi + lo), every product as
                              two launches accumulating in fp32: the norm outputs, q and k through the attention scores (the decoder's
                              precise kernels at head_dim 64; v goes from fp32 straight into the V^T tiles' fp16), the attention outputs,
                              the temporal attention in fp32, the activation outputs; with out_feats_lo the selected patch tokens leave
                              as a pair too. The hidden state is then within ~1e-5 of fp32 in both operand builds.
                              1: the MLPs' operands (layer_norm2 -> fc1, activation -> fc2: what carries the tower's distance from fp32)
                              with their rounding remainders -- as MX-FP4 images in the same launch when the layers carry w14 / w24
                              (else as 16-bit operand pairs, two launches) -- and out_feats as a pair; the attention paths standard:
                              the towers' share of the decoder's precise level 3.
                              0 (default): standard. */
  uint16_t* out_feats_lo;  /* optional DEVICE buffer [B*T*G*G][D]: the low half of out_feats (precise >= 1 only) */
} vt_vit_model;

size_t vt_vit_workspace_bytes(const vt_vit_model* m, int B, int T);
/* pixels: image tower [B][3][H][W] (T = 1, video_layout = 0); video tower [B][3][T][H][W] (video_layout = 1).
 * out_feats  bf16 [B*T*G*G][D]  patch tokens of the selected hidden state (required)
 * out_hidden fp32 [B*T*(G*G+1)][D] the full selected hidden state incl. CLS (optional, NULL to skip) */
int vt_vit_forward(const vt_vit_model* m, const void* pixels, int pix_dtype, int B, int T, int video_layout,
                   uint16_t* out_feats, float* out_hidden, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * LLaMA decoder (Vicuna-7B shape class): prefill and decode through one entry point, paged KV cache.
 * reference LlavaLlamaForCausalLM.forward -> transformers-4.31 LlamaForCausalLM.forward
 *   vitron/model/language_model/llava_llama.py:57-102 ; decode-step plumbing llava_arch.py:196-205
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct vt_llama_layer {
  const float* rms1;     /* input_layernorm.weight [H] */
  const uint16_t* wqkv;  /* [3H][H] rows = q | k | v */
  const uint16_t* wo;    /* [H][H] */
  const float* rms2;     /* post_attention_layernorm.weight */
  const uint16_t* wgu;   /* [2I][H], rows interleaved in blocks of 16: gate | up | gate | up ... */
  const uint16_t* wdown; /* [H][I] */
  /* precise level 3 (precise_qk = 3) only, else NULL: the MX-FP4 images of the four weight matrices (vt_mx4_quant_weights on the packed
   * matrices above: same row order) and their per-row exponents */
  const uint8_t* wqkv4;  const uint8_t* wqkv_e;
  const uint8_t* wo4;    const uint8_t* wo_e;
  const uint8_t* wgu4;   const uint8_t* wgu_e;
  const uint8_t* wdown4; const uint8_t* wdown_e;
  /* NF4 weights (load_4bit; vt_nf4_quant on the packed matrices above, same row order), else NULL. A layer with these set and wqkv / wo / wgu /
   * wdown NULL runs its Linears on vt_gemm_nf4 when a launch has <= 32 rows (with the decode step's norm folding), and otherwise dequantises
   * each matrix into one reusable workspace buffer in front of the unchanged tile GEMMs (prefill logits bit-equal to a 16-bit model built from
   * the dequantised weights). Precise levels 1-3 refuse NF4 layers. */
  const uint8_t* wqkv_nf4;  const float* wqkv_absmax;
  const uint8_t* wo_nf4;    const float* wo_absmax;
  const uint8_t* wgu_nf4;   const float* wgu_absmax;
  const uint8_t* wdown_nf4; const float* wdown_absmax;
} vt_llama_layer;

typedef struct vt_llama_model {
  int hidden, heads, head_dim, intermediate, num_layers, vocab;
  float rms_eps;
  const float* final_norm;    /* [H] */
  const uint16_t* lm_head;    /* [V][H] */
  const float* rope_cos;      /* [rope_len][head_dim/2] */
  const float* rope_sin;
  int rope_len;
  const vt_llama_layer* layers; /* host array [num_layers] */
  int prefill_norm_fold;        /* 1: prefills (rows > 64) fold RMSNorm into the MFMA tile GEMMs (residual epilogues emit bf16(x .* w)
                                   and partial sums of x^2, the consumer GEMMs scale their rows); same accuracy, measured no faster:
                                   default 0. Decode steps (<= 16 rows) always fold. */
  int qkv_fuse;                 /* 1: prefills write rotated q / K pages / V^T pages from the QKV projection's epilogue instead of the
                                   separate vt_kv_tiles pass. Bit-identical results; measured 20 us per launch SLOWER at S = 5120 (the
                                   epilogue of a one-workgroup-per-CU kernel overlaps with nothing: 455 vs 386 + 48.5 us): default 0. */
  int precise_qk;               /* 3: precise level 3 (head_dim 128, hidden % 512 == 0, intermediate % 128 == 0; the layers' *4 / *_e images set):
                                   PREFILLS run every decoder Linear as ONE launch that adds, to the 16-bit product, the product of the MX-FP4
                                   image of the A operand's rounding remainder with the weights' MX-FP4 image on the 4x-rate MX pipe (vt_gemm_mx;
                                   RMSNorm, the attention kernels and the SwiGLU epilogue emit the remainder's image beside the 16-bit operand);
                                   the lm_head's operand is a 16-bit pair as in level 2; q / k / v / P / V^T are stored as in the standard mode.
                                   The mode north_star's 1e-3 is met in at ~1.25x of the standard step. A request the shapes
                                   cannot serve is an ERROR, never a silent standard-mode pass.
                                   2: precise level 2 -- level 1 below plus EVERY other GEMM A operand of a prefill as a pair (v projection,
                                   attention output -> o_proj, post-attention norm -> gate/up with the SwiGLU as its own fp32 -> pair pass,
                                   SwiGLU output -> down_proj, final norm -> lm_head): each product runs
                                   as two launches accumulating in fp32. A verification mode: ~2x the GEMM work.
                                   1 (head_dim 128): PREFILLS carry everything that reaches the softmax's argument as operand PAIRS
                                   (hi + lo, 2 x 16 bit): the input-norm output feeds the q / k projection as A_hi.W^T + A_lo.W^T into fp32,
                                   the rotary embedding runs in fp32, and the attention scores are K_hi.(Q_hi + Q_lo)^T + K_lo.Q_hi^T -- so the
                                   scores see ~2^-20 of operand rounding instead of 2^-12 (fp16) / 2^-9 (bf16). Removes the five storage points
                                   the softmax amplifies: fp16 full-depth logits 1.3e-3 -> below 1e-3 of the reference's fp32.
                                   Costs two extra GEMM launches, +2 MFMAs per score k-step and the workspace for the pairs; the K pages hold
                                   K_hi (decode steps and later passes are unchanged). Default 0. */
  int last_layer_full;          /* 0 (default): a standard-mode prefill (max_q_len > 1, rows > 32; prefill_norm_fold and precise_qk 0; with
                                   qkv_fuse = 1 the layers in front of the last one fuse their page writes, the last one is pruned all the
                                   same, so qkv_fuse stays bit-identical to the default) that returns no hidden stream (out_hidden NULL) and reads at most 16 logit rows runs its LAST layer on
                                   those rows only: K | V projection and page writes for every row as before (the KV pool is bit-identical,
                                   so are the decode steps that follow), but q, the attention, o_proj, the second norm and the MLP only for
                                   the logit rows, on the weight-streaming GEMMs and the split-KV single-query attention of a decode step
                                   (same rounding model, a decode step's summation order: logits are as close to the fp32 reference, not
                                   bit-equal). Any other value: the last layer runs on all rows like the others (A/B, tests). */
  const uint16_t* embeds_lo;    /* optional DEVICE buffer [rows][H] in the operand format: the LOW half of the input embeddings when the caller
                                   carries them as a pair (precise level 2: the projector's output is not rounded to 16 bits on its way into the
                                   residual stream); added to x_embeds in fp32. NULL (default): x_embeds alone. */
  float* hidden_trace;          /* optional DEVICE buffer fp32 [num_layers][rows][H]: when non-NULL every layer's INPUT residual stream is
                                   copied there (entry 0 = the input embeddings) -- what `output_hidden_states=True` of the reference's
                                   LlamaModel collects before each decoder layer (llava_llama.py:69, transformers 4.31 LlamaModel.forward).
                                   NULL (default): nothing is copied. */
  uint16_t* logit_row_trace;    /* optional DEVICE buffer in the operand format, [num_layers][n_logit_rows][H]: when non-NULL entry [l][i] is the
                                   INPUT residual stream of decoder layer l (what hidden_trace holds) at row logit_rows[i], rounded ONCE to the
                                   operand format (round to nearest even; the fp16 build saturates at +-65504 like every operand store): the A
                                   operand of an lm_head over an early layer (DoLa) without the [L][rows][H] fp32 trace. One
                                   small gather launch per written layer; every pass shape and precise level, both pools, NF4 layers (the
                                   stream is fp32 [rows][H] at the top of every layer in all of them). No logit and no page bit changes.
                                   NULL (default), or n_logit_rows == 0: nothing is launched. ABI 114 carries the two fields WITHOUT a bump,
                                   appended at the end as hidden_trace was. */
  const uint8_t* logit_row_trace_layers; /* HOST array [num_layers], or NULL for all layers: only layers with a non-zero flag are written, the
                                   other entries of logit_row_trace are left untouched. */
} vt_llama_model;

/* KV pool: k  [num_layers][num_pages][heads][64][head_dim]   (K rows, rotary applied)
 *          vt [num_layers][num_pages][heads][head_dim][64]   (V transposed inside the page) */
typedef struct vt_kv_cache {
  uint16_t* k;
  uint16_t* vt;
  int num_pages;
} vt_kv_cache;

size_t vt_llama_workspace_bytes(const vt_llama_model* m, int rows, int n_logit_rows, int nseq, int max_kv_len);
/* x_embeds    bf16 [rows][H]   packed input embeddings of all sequences (no padding rows)
 * positions   int32 [rows]     rotary position of every row
 * seq_desc    int32 [nseq][4]  {q_row0, q_len, kv_len, table_off} ; kv_len = past + q_len
 * tile_table  int32            page ids, tile_table[table_off + t] = page of positions [64t, 64t+64)
 * logit_rows  int32 [n_logit_rows] rows whose logits are wanted (generate: the last row of every sequence)
 * logits      fp32 [n_logit_rows][V]
 * The new tokens' K/V are appended to the cache pages; attention is causal over past + new tokens. */
int vt_llama_forward(const vt_llama_model* m, const vt_kv_cache* kv, const uint16_t* x_embeds, int rows,
                     const int* positions, const int* seq_desc, int nseq, int max_q_len, int max_new_tiles, int max_kv_len,
                     const int* tile_table, const int* logit_rows, int n_logit_rows, float* logits,
                     float* out_hidden, void* workspace, size_t workspace_bytes, void* stream);

/* ---- FP8 KV CACHE (opt-in: config.kv_cache_dtype = "fp8"; no reference counterpart) -----------------------------------
 * Page format: the 16-bit layouts with 1-byte elements -- k [num_layers][num_pages][heads][64][head_dim], vt [num_layers][num_pages]
 * [heads][head_dim][64]; VT_PAGE_TOKENS stays 64, so tile tables and page counts carry over. Element: OCP e4m3fn (gfx950's native fp8;
 * bias 7, no infinity, 0x7f / 0xff = NaN, largest finite 448), no scale factors. A byte is e4m3_rne(clamp(x16, -448, +448)) where
 * x16 is exactly what the 16-bit cache holds at that position (K: rotated in fp32, rounded once to the operand format; V: the fp16
 * page value): for the same inputs  fp8 page == vt_kv8_quant(16-bit page)  byte for byte. Padding rows / columns of a tile are 0x00.
 * Half the pool bytes per token and half the bytes a decode step streams; the price is e4m3's 3 mantissa bits on K and V. */
typedef struct vt_kv_cache8 {
  uint8_t* k;
  uint8_t* vt;
  int num_pages;
} vt_kv_cache8;
/* whole tiles: 16-bit tile src_table[i] (of k_tiles / vt_tiles, one layer) -> fp8 page dst_table[i] (of k8 / vt8), K and V^T in one launch;
 * and back. Dequantisation is exact in both operand formats; quantising a dequantised tile is the identity on every finite code. */
int vt_kv8_quant(const uint16_t* k_tiles, const uint16_t* vt_tiles, const int* src_table, uint8_t* k8, uint8_t* vt8,
                 const int* dst_table, int ntiles, int heads, int head_dim, void* stream);
int vt_kv8_dequant(const uint8_t* k8, const uint8_t* vt8, const int* src_table, uint16_t* k_tiles, uint16_t* vt_tiles,
                   const int* dst_table, int ntiles, int heads, int head_dim, void* stream);
/* vt_attn_decode on fp8 pages (same arguments, same scratch: vt_attn_decode_scratch_bytes) */
int vt_attn_decode_kv8(const uint16_t* Q, int ldq, const uint8_t* k8, const uint8_t* vt8, const int* tile_table,
                       const int* seq_desc, int nseq, uint16_t* O, int ldo, int heads, int head_dim, float scale,
                       int max_kv_len, void* scratch, size_t scratch_bytes, void* stream);
/* vt_attn_decode_fused on fp8 pages: the new k row / v column are quantised, stored, and the new token is SCORED FROM ITS QUANTISED
 * VALUE (what every later step reads), so the step equals vt_attn_decode_kv8 on the cache it leaves behind. */
int vt_attn_decode_fused_kv8(const uint16_t* qkv, int ldqkv, int q_col0, int k_col0, int v_col0, uint8_t* k8, uint8_t* vt8,
                             const int* tile_table, const int* seq_desc, int nseq, uint16_t* O, int ldo, int heads, int head_dim,
                             float scale, const float* rope_cos, const float* rope_sin, const int* positions, void* stream);
/* vt_llama_forward on an fp8 pool. n_table_tiles = number of entries of tile_table. Decode steps (max_q_len == 1) run
 * vt_attn_decode_fused_kv8 in place of the 16-bit kernel, nothing else differs. Prefills run the unchanged 16-bit kernels on a
 * staging pool of n_table_tiles K + V^T tiles of ONE layer carved from the workspace (identity tile table), per layer: dequantise the
 * past tiles of sequences with kv_len > q_len, vt_kv_tiles + vt_flash_attn on the staging pool, quantise tiles [past / 64, ntiles)
 * back into the pages. A prefill without a past therefore returns logits bit-equal to the 16-bit cache's; a pass that mixes a chunk
 * with long decoding sequences stages every sequence's whole past per layer (correct, costly: keep them in separate passes).
 * precise_qk >= 1 and qkv_fuse == 1 are refused (status -1), never run as a silent 16-bit pass. */
size_t vt_llama_workspace_bytes_kv8(const vt_llama_model* m, int rows, int n_logit_rows, int nseq, int max_kv_len, int n_table_tiles);
int vt_llama_forward_kv8(const vt_llama_model* m, const vt_kv_cache8* kv, const uint16_t* x_embeds, int rows,
                         const int* positions, const int* seq_desc, int nseq, int max_q_len, int max_new_tiles, int max_kv_len,
                         const int* tile_table, int n_table_tiles, const int* logit_rows, int n_logit_rows, float* logits,
                         float* out_hidden, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Per-kernel-class timing (the reference has no tracing on this path). Between vt_profile_begin and
 * vt_profile_end every launch of the instrumented kernel classes is bracketed by hipEvents recorded on the SAME
 * stream as the kernel, so the durations are device-side launch durations inside the caller's timed region.
 * vt_profile_end synchronises on the recorded events and fills, per class: launches, total milliseconds, total
 * algorithmic work (FLOP for MFMA kernels, bytes for the weight-streaming kernel). Arrays hold VT_PROF_CLASSES items.
 * ---------------------------------------------------------------------------------------------------------- */
enum { VT_PROF_GEMM_TILE = 0, VT_PROF_FLASH_ATTN = 1, VT_PROF_GEMM_SKINNY = 2, VT_PROF_ATTN_DECODE = 3, VT_PROF_CLASSES = 4 };
int vt_profile_begin(void);
int vt_profile_end(int* launches, double* total_ms, double* total_work);
/* What the matrix pipe sustains by itself on THIS device (measurement aid for the roofline, no reference counterpart): one wave per SIMD
 * on every CU, operands in registers, nothing but v_mfma_f32_16x16x32 (bf16 or f16: the library's operand format) on a 128 x 128
 * accumulator tile in the loop -- the four-wave GEMM's wave tile without its memory side. a, b: at least 64 Ki 16-byte fragments each
 * (8 operand values: the caller chooses their distribution -- the sustained clock of this part depends on the operand VALUES, zeros
 * run ~19 % faster than N(0,1)); out: multiprocessors x 256 floats. FLOP per launch = 2 * 128*128*64 * iters * 4 * multiprocessors. */
int vt_probe_mfma(const uint16_t* a, const uint16_t* b, float* out, int iters, void* stream);
/* What a kernel that only READS sustains from HBM on THIS device (measurement aid for the roofline of the decode step, whose bytes are
 * weights and KV pages read once; ABI 113): `bytes` (>= 16, p 16-byte aligned) are read once, 16 bytes per lane and load; nt != 0 uses the
 * read-once cache policy of the weight-streaming GEMM. out: one word (never written in practice: it keeps the loads alive). */
int vt_probe_read(const void* p, size_t bytes, int nt, unsigned* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VITRON_HIP_H */
