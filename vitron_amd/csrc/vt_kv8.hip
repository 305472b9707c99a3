// vt_kv8.hip -- the FP8 (OCP e4m3fn) paged KV cache: page conversion and decode attention on 1-byte pages (gfx950 / CDNA4).
//
// Page format (include/vitron_hip.h "FP8 KV CACHE"): the 16-bit layouts with 1-byte elements -- K page [page][head][64 keys][HD],
// V^T page [page][head][HD][64 keys], 64 keys per page. No scale factors. A byte is e4m3_rne(clamp(x16, -448, +448)) where x16 is
// exactly the value the 16-bit cache holds at that position (K: rotated in fp32, rounded once to the operand format; V: the fp16
// page value), so for the same inputs fp8 page == quant(16-bit page) byte for byte. Padding rows / columns of a tile are zero bytes.
//
// Kernels:
//  * kv8_quant_kernel / kv8_dequant_kernel<SEQ>: whole tiles, 16-bit tile <-> fp8 page, K and V^T in one launch, 16-byte accesses.
//    SEQ = false: explicit (src_table, dst_table) pairs (the public entry points). SEQ = true: source and destination derived from
//    (seq_desc, tile_table) on the device, for the staging pool of vt_llama_forward_kv8's prefills (identity staging table).
//  * attn_decode_kv8_kernel<HD> / attn_decode_fused_kv8_kernel<HD, ROPE>: the decode attention bodies of vt_attn_decode.h -- the ones
//    behind attn_decode_kernel / attn_decode_fused_kernel of vt_attn.hip -- instantiated with the e4m3 page format defined here. Same
//    scratch layout; the splits are merged by vt_attn.hip's attn_decode_combine_kernel (vt_attn_decode_combine_launch). The new token
//    is quantised, stored and SCORED from its quantised value (the value every later step reads), so a step equals the split kernel
//    run on the cache it leaves behind.
//
// The file stays its own translation unit; the per-tile arithmetic of decode attention is in the shared header, so a change there
// rebuilds the kernels of both page formats.
#include "vt_attn_decode.h"
#include "vt_kernels.h"

namespace {

// ---- e4m3fn <-> f32 ---------------------------------------------------------------------------------------------------------
// clamp in fp32 first: e4m3fn has no infinity, an overflowing conversion would produce NaN. NaN stays NaN (as vt_clamp_f16).
__device__ __forceinline__ float kv8_clamp(float x) {
  const float c = __builtin_amdgcn_fmed3f(x, -448.f, 448.f);
  return x != x ? x : c;
}
// four floats -> four e4m3 bytes (a in bits 0..7): two v_cvt_pk_fp8_f32
__device__ __forceinline__ uint32_t kv8_pack4(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(a), kv8_clamp(b), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(c), kv8_clamp(d), w, true);
  return (uint32_t)w;
}
// four e4m3 bytes -> four floats: two v_cvt_pk_f32_fp8
__device__ __forceinline__ void kv8_unpack4(uint32_t w, float (&f)[4]) {
  const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  f[0] = lo[0];
  f[1] = lo[1];
  f[2] = hi[0];
  f[3] = hi[1];
}
__device__ __forceinline__ float kv8_byte_to_f32(uint8_t b) { return __builtin_amdgcn_cvt_pk_f32_fp8((int)b, false)[0]; }

// 16 consecutive elements: two 16-byte chunks of 16-bit values -> one 16-byte chunk of e4m3. VFMT: the source is fp16 (V^T pages) in
// both builds; otherwise the operand format (K pages).
template <bool VFMT>
__device__ __forceinline__ u32x4 kv8_quant16(const u32x4 a, const u32x4 b) {
  u32x4 o;
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const uint32_t a0 = a[2 * w], a1 = a[2 * w + 1], b0 = b[2 * w], b1 = b[2 * w + 1];
    if constexpr (VFMT) {
      o[w] = kv8_pack4(f16lo_to_f32(a0), f16hi_to_f32(a0), f16lo_to_f32(a1), f16hi_to_f32(a1));
      o[2 + w] = kv8_pack4(f16lo_to_f32(b0), f16hi_to_f32(b0), f16lo_to_f32(b1), f16hi_to_f32(b1));
    } else {
      o[w] = kv8_pack4(oplo_to_f32(a0), ophi_to_f32(a0), oplo_to_f32(a1), ophi_to_f32(a1));
      o[2 + w] = kv8_pack4(oplo_to_f32(b0), ophi_to_f32(b0), oplo_to_f32(b1), ophi_to_f32(b1));
    }
  }
  return o;
}
// the inverse: exact in both formats (every finite e4m3 value is a bf16 and an fp16 value)
template <bool VFMT>
__device__ __forceinline__ void kv8_dequant16(const u32x4 q, u32x4& a, u32x4& b) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    float f[4];
    kv8_unpack4(q[w], f);
    uint32_t p0, p1;
    if constexpr (VFMT) {
      p0 = pack_f16x2(f[0], f[1]);
      p1 = pack_f16x2(f[2], f[3]);
    } else {
      p0 = pack_op2(f[0], f[1]);
      p1 = pack_op2(f[2], f[3]);
    }
    if (w < 2) {
      a[2 * w] = p0;
      a[2 * w + 1] = p1;
    } else {
      b[2 * (w - 2)] = p0;
      b[2 * (w - 2) + 1] = p1;
    }
  }
}

// source / destination tile of this block. SEQ = false: grid (pair, head), tiles from the two tables. SEQ = true: grid (tile of the
// sequence, sequence, head); the 16-bit side is the staging pool, whose table is the identity (slot = table_off + t); QUANT runs
// over the tiles that hold new rows [past / 64, ntiles), dequantisation over the tiles that hold a past [0, ceil(past / 64)).
template <bool QUANT, bool SEQ>
__device__ __forceinline__ bool kv8_tile_pair(const int* __restrict__ src_table, const int* __restrict__ dst_table,
                                              const VtAttnSeq* __restrict__ seqs, int heads, int& src, int& dst, int& head) {
  if constexpr (!SEQ) {
    head = blockIdx.y;
    src = src_table[blockIdx.x];
    dst = dst_table[blockIdx.x];
    return true;
  } else {
    const VtAttnSeq sq = seqs[blockIdx.y];
    head = blockIdx.z;
    const int past = sq.kv_len - sq.q_len;
    const int* tile_table = src_table;
    if constexpr (QUANT) {
      const int t = (past >> 6) + blockIdx.x;
      if (t >= ((sq.kv_len + 63) >> 6)) return false;
      src = sq.table_off + t;
      dst = tile_table[sq.table_off + t];
    } else {
      const int t = blockIdx.x;
      if (t >= ((past + 63) >> 6)) return false;
      src = tile_table[sq.table_off + t];
      dst = sq.table_off + t;
    }
    return true;
  }
}

template <int HD, bool SEQ>
__global__ __launch_bounds__(256) void kv8_quant_kernel(const bf16_t* __restrict__ Kt, const uint16_t* __restrict__ Vt,
                                                        const int* __restrict__ src_table, uint8_t* __restrict__ K8,
                                                        uint8_t* __restrict__ V8, const int* __restrict__ dst_table,
                                                        const VtAttnSeq* __restrict__ seqs, int heads) {
  int src, dst, head;
  if (!kv8_tile_pair<true, SEQ>(src_table, dst_table, seqs, heads, src, dst, head)) return;
  const size_t soff = ((size_t)src * heads + head) * 64 * HD, doff = ((size_t)dst * heads + head) * 64 * HD;
  constexpr int G = 64 * HD / 16;   // 16-element groups per tile
  for (int g = threadIdx.x; g < G; g += 256) {
    const u32x4* ks = (const u32x4*)(Kt + soff + g * 16);
    const u32x4* vs = (const u32x4*)(Vt + soff + g * 16);
    const u32x4 k0 = ks[0], k1 = ks[1], v0 = vs[0], v1 = vs[1];
    *(u32x4*)(K8 + doff + g * 16) = kv8_quant16<false>(k0, k1);
    *(u32x4*)(V8 + doff + g * 16) = kv8_quant16<true>(v0, v1);
  }
}

template <int HD, bool SEQ>
__global__ __launch_bounds__(256) void kv8_dequant_kernel(const uint8_t* __restrict__ K8, const uint8_t* __restrict__ V8,
                                                          const int* __restrict__ src_table, bf16_t* __restrict__ Kt,
                                                          uint16_t* __restrict__ Vt, const int* __restrict__ dst_table,
                                                          const VtAttnSeq* __restrict__ seqs, int heads) {
  int src, dst, head;
  if (!kv8_tile_pair<false, SEQ>(src_table, dst_table, seqs, heads, src, dst, head)) return;
  const size_t soff = ((size_t)src * heads + head) * 64 * HD, doff = ((size_t)dst * heads + head) * 64 * HD;
  constexpr int G = 64 * HD / 16;
  for (int g = threadIdx.x; g < G; g += 256) {
    const u32x4 k = *(const u32x4*)(K8 + soff + g * 16);
    const u32x4 v = *(const u32x4*)(V8 + soff + g * 16);
    u32x4 a, b;
    kv8_dequant16<false>(k, a, b);
    u32x4* kd = (u32x4*)(Kt + doff + g * 16);
    kd[0] = a;
    kd[1] = b;
    kv8_dequant16<true>(v, a, b);
    u32x4* vd = (u32x4*)(Vt + doff + g * 16);
    vd[0] = a;
    vd[1] = b;
  }
}

__global__ void kv8_iota_kernel(int* __restrict__ t, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) t[i] = i;
}

// ------------------------------------------------------------------------------------------------------------------
// Decode attention on e4m3 pages: the bodies are vt_attn_decode.h's, this is the page format. EPC = 16: a K row is HD bytes = HD / 16
// lanes x 16 B (8 lanes at HD 128, 4 at HD 64), one wave-instruction covers 8 / 16 rows; a V^T row is 64 bytes = 4 lanes x 16 B, 16
// rows per wave-instruction; a whole tile is 8 KiB of K + 8 KiB of V^T at HD 128. The new token is quantised, stored and SCORED
// from its bytes, and its v enters the output as the quantised byte's value.
// ------------------------------------------------------------------------------------------------------------------
struct DecodePagesE4M3 {
  typedef uint8_t elem_t;
  static constexpr int EPC = 16;
  static __device__ __forceinline__ float dot(const u32x4 kv, const float (&qf)[16]) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      float f[4];
      kv8_unpack4(kv[w], f);
#pragma unroll
      for (int j = 0; j < 4; ++j) s = fmaf(f[j], qf[4 * w + j], s);
    }
    return s;
  }
  static __device__ __forceinline__ float pv(float acc, float alpha, const u32x4 vv, const float (&p)[16]) {
    float a = acc * alpha;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      float f[4];
      kv8_unpack4(vv[w], f);
#pragma unroll
      for (int j = 0; j < 4; ++j) a = fmaf(f[j], p[4 * w + j], a);
    }
    return a;
  }
  static __device__ __forceinline__ u32x4 pack_k(const uint32_t (&w)[8]) {
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      o[i] = kv8_pack4(oplo_to_f32(w[2 * i]), ophi_to_f32(w[2 * i]), oplo_to_f32(w[2 * i + 1]), ophi_to_f32(w[2 * i + 1]));
    return o;
  }
  static __device__ __forceinline__ u32x4 pack_v(const uint32_t (&w)[8]) {
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t a0 = op2_to_f16x2(w[2 * i]), a1 = op2_to_f16x2(w[2 * i + 1]);
      o[i] = kv8_pack4(f16lo_to_f32(a0), f16hi_to_f32(a0), f16lo_to_f32(a1), f16hi_to_f32(a1));
    }
    return o;
  }
  static __device__ __forceinline__ float v_to_f32(elem_t b) { return kv8_byte_to_f32(b); }
};

template <int HD>
__global__ __launch_bounds__(256) void attn_decode_kv8_kernel(const bf16_t* __restrict__ Q, int ldq, const uint8_t* __restrict__ K8,
                                                              const uint8_t* __restrict__ V8, const int* __restrict__ tile_table,
                                                              const VtAttnSeq* __restrict__ seqs, int heads, float scale_log2e,
                                                              float* __restrict__ part, int nsplit) {
  attn_decode_split_body<DecodePagesE4M3, HD>(Q, ldq, K8, V8, tile_table, seqs, heads, scale_log2e, part, nsplit);
}

template <int HD, bool ROPE>
__global__ __launch_bounds__(512) void attn_decode_fused_kv8_kernel(
    const bf16_t* __restrict__ qkv, int ldqkv, int q_col0, int k_col0, int v_col0, uint8_t* __restrict__ K8, uint8_t* __restrict__ V8,
    const int* __restrict__ tile_table, const VtAttnSeq* __restrict__ seqs, int heads, const float* __restrict__ rope_cos,
    const float* __restrict__ rope_sin, const int* __restrict__ positions, float scale_log2e, bf16_t* __restrict__ O, int ldo) {
  attn_decode_fused_body<DecodePagesE4M3, HD, ROPE>(qkv, ldqkv, q_col0, k_col0, v_col0, K8, V8, tile_table, seqs, heads, rope_cos,
                                                    rope_sin, positions, scale_log2e, O, ldo);
}

}  // namespace

// ---- launches ---------------------------------------------------------------------------------------------------------------
int vt_kv8_quant_launch(const bf16_t* Kt, const uint16_t* Vt, const int* src_table, uint8_t* K8, uint8_t* V8, const int* dst_table,
                        int ntiles, int heads, int HD, hipStream_t s) {
  VT_REQUIRE(Kt && Vt && src_table && K8 && V8 && dst_table, "vt_kv8_quant: null pointer");
  VT_REQUIRE(HD == 64 || HD == 128, "vt_kv8_quant: head_dim %d unsupported", HD);
  VT_REQUIRE(ntiles >= 0 && heads > 0, "vt_kv8_quant: empty problem");
  if (ntiles == 0) return VT_OK;
  dim3 grid(ntiles, heads), block(256);
  if (HD == 64) hipLaunchKernelGGL((kv8_quant_kernel<64, false>), grid, block, 0, s, Kt, Vt, src_table, K8, V8, dst_table, nullptr, heads);
  else hipLaunchKernelGGL((kv8_quant_kernel<128, false>), grid, block, 0, s, Kt, Vt, src_table, K8, V8, dst_table, nullptr, heads);
  VT_LAUNCH_CHECK();
  return VT_OK;
}

int vt_kv8_dequant_launch(const uint8_t* K8, const uint8_t* V8, const int* src_table, bf16_t* Kt, uint16_t* Vt, const int* dst_table,
                          int ntiles, int heads, int HD, hipStream_t s) {
  VT_REQUIRE(K8 && V8 && src_table && Kt && Vt && dst_table, "vt_kv8_dequant: null pointer");
  VT_REQUIRE(HD == 64 || HD == 128, "vt_kv8_dequant: head_dim %d unsupported", HD);
  VT_REQUIRE(ntiles >= 0 && heads > 0, "vt_kv8_dequant: empty problem");
  if (ntiles == 0) return VT_OK;
  dim3 grid(ntiles, heads), block(256);
  if (HD == 64) hipLaunchKernelGGL((kv8_dequant_kernel<64, false>), grid, block, 0, s, K8, V8, src_table, Kt, Vt, dst_table, nullptr, heads);
  else hipLaunchKernelGGL((kv8_dequant_kernel<128, false>), grid, block, 0, s, K8, V8, src_table, Kt, Vt, dst_table, nullptr, heads);
  VT_LAUNCH_CHECK();
  return VT_OK;
}

// the forward pass's forms: tiles derived from (seq_desc, tile_table); the 16-bit side is the staging pool (identity table)
int vt_kv8_quant_new_launch(const bf16_t* Kt, const uint16_t* Vt, uint8_t* K8, uint8_t* V8, const int* tile_table, const VtAttnSeq* seqs,
                            int nseq, int max_new_tiles, int heads, int HD, hipStream_t s) {
  VT_REQUIRE(Kt && Vt && K8 && V8 && tile_table && seqs, "vt_kv8_quant: null pointer");
  VT_REQUIRE(HD == 64 || HD == 128, "vt_kv8_quant: head_dim %d unsupported", HD);
  dim3 grid(max_new_tiles, nseq, heads), block(256);
  if (HD == 64) hipLaunchKernelGGL((kv8_quant_kernel<64, true>), grid, block, 0, s, Kt, Vt, tile_table, K8, V8, nullptr, seqs, heads);
  else hipLaunchKernelGGL((kv8_quant_kernel<128, true>), grid, block, 0, s, Kt, Vt, tile_table, K8, V8, nullptr, seqs, heads);
  VT_LAUNCH_CHECK();
  return VT_OK;
}

int vt_kv8_dequant_past_launch(const uint8_t* K8, const uint8_t* V8, bf16_t* Kt, uint16_t* Vt, const int* tile_table,
                               const VtAttnSeq* seqs, int nseq, int max_kv_len, int heads, int HD, hipStream_t s) {
  VT_REQUIRE(K8 && V8 && Kt && Vt && tile_table && seqs, "vt_kv8_dequant: null pointer");
  VT_REQUIRE(HD == 64 || HD == 128, "vt_kv8_dequant: head_dim %d unsupported", HD);
  dim3 grid((max_kv_len + 63) / 64, nseq, heads), block(256);
  if (HD == 64) hipLaunchKernelGGL((kv8_dequant_kernel<64, true>), grid, block, 0, s, K8, V8, tile_table, Kt, Vt, nullptr, seqs, heads);
  else hipLaunchKernelGGL((kv8_dequant_kernel<128, true>), grid, block, 0, s, K8, V8, tile_table, Kt, Vt, nullptr, seqs, heads);
  VT_LAUNCH_CHECK();
  return VT_OK;
}

int vt_kv8_iota_launch(int* table, int n, hipStream_t s) {
  VT_REQUIRE(table && n > 0, "vt_kv8: empty staging table");
  hipLaunchKernelGGL(kv8_iota_kernel, dim3((n + 255) / 256), dim3(256), 0, s, table, n);
  VT_LAUNCH_CHECK();
  return VT_OK;
}

int vt_attn_decode_kv8_launch(const bf16_t* Q, int ldq, const uint8_t* K8, const uint8_t* V8, const int* tile_table, const VtAttnSeq* seqs,
                              int nseq, bf16_t* O, int ldo, int heads, int HD, float scale, int max_kv_len, float* scratch,
                              size_t scratch_bytes, hipStream_t s) {
  VT_REQUIRE(Q && K8 && V8 && tile_table && seqs && O && scratch, "vt_attn_decode_kv8: null pointer");
  VT_REQUIRE(HD == 64 || HD == 128, "vt_attn_decode_kv8: head_dim %d unsupported", HD);
  VT_REQUIRE(max_kv_len > 0 && nseq > 0 && heads > 0, "vt_attn_decode_kv8: empty problem");
  VT_REQUIRE(ldq % 8 == 0, "vt_attn_decode_kv8: misaligned q rows");
  const int nsplit = vt_attn_decode_nsplit(max_kv_len);
  const size_t need = vt_attn_decode_scratch_bytes(nseq, heads, HD, max_kv_len);
  if (scratch_bytes < need) {
    vt_set_error("vt_attn_decode_kv8: scratch too small (%zu < %zu)", scratch_bytes, need);
    return VT_ERR_WORKSPACE;
  }
  const float sl2 = scale * 1.4426950408889634f;
  VtProfScope prof(VT_PROF_ATTN_DECODE, 0.0, s);
  dim3 grid(heads, nseq, nsplit), block(256);
  if (HD == 64) hipLaunchKernelGGL((attn_decode_kv8_kernel<64>), grid, block, 0, s, Q, ldq, K8, V8, tile_table, seqs, heads, sl2, scratch, nsplit);
  else hipLaunchKernelGGL((attn_decode_kv8_kernel<128>), grid, block, 0, s, Q, ldq, K8, V8, tile_table, seqs, heads, sl2, scratch, nsplit);
  vt_attn_decode_combine_launch(scratch, seqs, nseq, O, ldo, heads, HD, nsplit, s);
  VT_LAUNCH_CHECK();
  return VT_OK;
}

int vt_attn_decode_fused_kv8_launch(const bf16_t* qkv, int ldqkv, int q_col0, int k_col0, int v_col0, uint8_t* K8, uint8_t* V8,
                                    const int* tile_table, const VtAttnSeq* seqs, int nseq, bf16_t* O, int ldo, int heads, int HD,
                                    float scale, const float* rope_cos, const float* rope_sin, const int* positions, hipStream_t s) {
  VT_REQUIRE(qkv && K8 && V8 && tile_table && seqs && O, "vt_attn_decode_fused_kv8: null pointer");
  VT_REQUIRE(HD == 64 || HD == 128, "vt_attn_decode_fused_kv8: head_dim %d unsupported", HD);
  VT_REQUIRE(nseq > 0 && heads > 0, "vt_attn_decode_fused_kv8: empty problem");
  VT_REQUIRE(ldqkv % 8 == 0 && q_col0 % 8 == 0 && k_col0 % 8 == 0 && v_col0 % 8 == 0, "vt_attn_decode_fused_kv8: misaligned columns");
  if (rope_cos) VT_REQUIRE(rope_sin && positions, "vt_attn_decode_fused_kv8: rope needs sin table and positions");
  const float sl2 = scale * 1.4426950408889634f;
  VtProfScope prof(VT_PROF_ATTN_DECODE, 0.0, s);
  dim3 grid(heads, nseq), block(512);
#define VT_ADF8(HDV, RV)                                                                                                               \
  hipLaunchKernelGGL((attn_decode_fused_kv8_kernel<HDV, RV>), grid, block, 0, s, qkv, ldqkv, q_col0, k_col0, v_col0, K8, V8, tile_table, \
                     seqs, heads, rope_cos, rope_sin, positions, sl2, O, ldo)
  if (HD == 64) {
    if (rope_cos) VT_ADF8(64, true); else VT_ADF8(64, false);
  } else {
    if (rope_cos) VT_ADF8(128, true); else VT_ADF8(128, false);
  }
#undef VT_ADF8
  VT_LAUNCH_CHECK();
  return VT_OK;
}
