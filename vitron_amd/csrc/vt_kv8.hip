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
//  * attn_decode_kv8_kernel (+ attn_decode_combine_kernel's twin): attn_decode_kernel of vt_attn.hip on fp8 pages, same scratch layout.
//  * attn_decode_fused_kv8_kernel<HD, ROPE>: attn_decode_fused_kernel on fp8 pages; the new token is quantised, stored and SCORED from
//    its quantised value (the value every later step reads), so a step equals the split kernel run on the cache it leaves behind.
//
// This is a separate translation unit on purpose: the 16-bit kernels' generated code does not change when this file does.
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

// ---- lane exchanges (as in vt_attn.hip; this file shares no code object with it) ------------------------------------------------
template <int MASK>
__device__ __forceinline__ float lane_xor16(float v) {
  int x = __builtin_bit_cast(int, v);
  if constexpr (MASK == 1) x = __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true);
  else if constexpr (MASK == 2) x = __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true);
  else x = __builtin_amdgcn_ds_swizzle(x, (MASK << 10) | 0x1F);
  return __builtin_bit_cast(float, x);
}
// CH (4 or 8) lanes (c = lane % CH) each hold CH partial sums; on return part[0] is the full sum of value i == c (recursive halving)
template <int CH>
__device__ __forceinline__ float reduce_scatter_lanes(float (&part)[CH], int c) {
#define VT_RS_STEP(N)                                                   \
  if constexpr (CH >= 2 * (N)) {                                        \
    const bool up = (c & (N)) != 0;                                     \
    _Pragma("unroll") for (int j = 0; j < (N); ++j) {                   \
      const float send = up ? part[j] : part[j + (N)];                  \
      const float mine = up ? part[j + (N)] : part[j];                  \
      part[j] = mine + lane_xor16<(N)>(send);                           \
    }                                                                   \
  }
  VT_RS_STEP(4)
  VT_RS_STEP(2)
  VT_RS_STEP(1)
#undef VT_RS_STEP
  return part[0];
}
template <int CH>
__device__ __forceinline__ float allreduce_lanes(float v) {
  if constexpr (CH >= 8) v += lane_xor16<4>(v);
  v += lane_xor16<2>(v);
  v += lane_xor16<1>(v);
  return v;
}

// score partial of one 16-byte K chunk (16 e4m3 keys' elements d = c * 16 ..) against this lane's 16 q values: a chain of 16 fmaf
__device__ __forceinline__ float kv8_dot16(const u32x4 kv, const float (&qf)[16]) {
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
// acc = acc * alpha + sum of 16 keys' p * v of one 16-byte V^T chunk (keys vchk * 16 ..): one product and a chain of 16 fmaf
__device__ __forceinline__ float kv8_pv16(float acc, float alpha, const u32x4 vv, const float (&p)[16]) {
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

// ------------------------------------------------------------------------------------------------------------------
// attn_decode_kv8_kernel: attn_decode_kernel (vt_attn.hip) on e4m3 pages. HBM-bound: stream K and V^T tiles once, 16 B per lane,
// non-temporal, a whole tile (HD = 128: 8 KiB of K + 8 KiB of V^T) requested before anything is consumed.
//   grid (head, sequence, split); 4 waves per block; wave w of split s owns tiles t = 4*s + w, 4*s + w + 4*nsplit, ... (as the 16-bit kernel)
//   scores : a K row is HD bytes = CH = HD / 16 lanes x 16 B (8 lanes at HD 128, 4 at HD 64); one wave-instruction covers KPI = 64 / CH
//            rows (8 / 16), a tile takes CH instructions. Lane (c = lane % CH, g = lane / CH) holds elements d = 16c .. 16c + 15 of rows
//            i * KPI + g; its CH partial sums (16 fmaf each) are reduce-scattered over the CH lanes (CH - 1 exchanges), after which the
//            lane owns key  c * KPI + g.
//   PV     : a V^T row is 64 bytes = 4 lanes x 16 B; one wave-instruction covers 16 rows (16 full 64-B rows = 8 cache lines), a tile
//            takes NACC = HD / 16 instructions. Lane (vchk = lane % 4, vrow = lane / 4) holds keys 16 vchk .. 16 vchk + 15 of rows
//            i * 16 + vrow and keeps NACC accumulators (17 roundings per tile each: the alpha product and 16 fmaf); the 4 lanes of a row meet
//            once after the last tile.
//   partial (m, l, o[HD]) per block in the 16-bit kernel's scratch layout; the combine is the 16-bit kernel's, restated below.
// ------------------------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(256) void attn_decode_kv8_kernel(const bf16_t* __restrict__ Q, int ldq, const uint8_t* __restrict__ K8,
                                                              const uint8_t* __restrict__ V8, const int* __restrict__ tile_table,
                                                              const VtAttnSeq* __restrict__ seqs, int heads, float scale_log2e,
                                                              float* __restrict__ part, int nsplit) {
  constexpr int CH = HD / 16, KPI = 64 / CH, NACC = HD / 16;
  __shared__ float sm_m[4], sm_l[4];
  __shared__ float sm_o[4][HD];
  __shared__ __attribute__((aligned(16))) float sm_p[4][64];
  const VtAttnSeq sq = seqs[blockIdx.y];
  const int head = blockIdx.x, split = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ntiles = (sq.kv_len + 63) >> 6;
  const bf16_t* qp = Q + (size_t)sq.q_row0 * ldq + head * HD;
  const int c = lane % CH;
  float qf[16];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const u32x4 qv = *(const u32x4*)(qp + c * 16 + h * 8);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      qf[8 * h + 2 * w] = oplo_to_f32(qv[w]);
      qf[8 * h + 2 * w + 1] = ophi_to_f32(qv[w]);
    }
  }
  float m_run = -INFINITY, l_run = 0.f, acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.f;
  const int vrow = lane >> 2, vchk = lane & 3;
  const int key_of_lane = c * KPI + lane / CH;

  for (int t = split * 4 + wave; t < ntiles; t += 4 * nsplit) {
    const size_t toff = ((size_t)tile_table[sq.table_off + t] * heads + head) * 64 * HD;
    u32x4 kk[CH], vv[NACC];
#pragma unroll
    for (int i = 0; i < CH; ++i) kk[i] = __builtin_nontemporal_load((const u32x4*)(K8 + toff + (i * KPI + lane / CH) * HD + c * 16));
#pragma unroll
    for (int i = 0; i < NACC; ++i) vv[i] = __builtin_nontemporal_load((const u32x4*)(V8 + toff + (i * 16 + vrow) * 64 + vchk * 16));
    __builtin_amdgcn_sched_barrier(0);
    float ps[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) ps[i] = kv8_dot16(kk[i], qf);
    const float s_mine = reduce_scatter_lanes<CH>(ps, c);
    const int mykey = t * 64 + key_of_lane;
    const float s2 = (mykey < sq.kv_len) ? s_mine * scale_log2e : -INFINITY;
    const float m_new = fmaxf(m_run, wave_max(s2));
    const float alpha = fast_exp2(m_run - m_new);
    const float p = fast_exp2(s2 - m_new);
    l_run = l_run * alpha + wave_sum(p);
    m_run = m_new;
    sm_p[wave][key_of_lane] = p;
    __builtin_amdgcn_wave_barrier();
    float pk[16];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const f32x4 pv = *(const f32x4*)(&sm_p[wave][vchk * 16 + 4 * w]);
#pragma unroll
      for (int j = 0; j < 4; ++j) pk[4 * w + j] = pv[j];
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = kv8_pv16(acc[i], alpha, vv[i], pk);
  }
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    float a = acc[i];
    a += __shfl_xor(a, 1, 64);
    a += __shfl_xor(a, 2, 64);
    if (vchk == 0) sm_o[wave][i * 16 + vrow] = a;
  }
  if (lane == 0) {
    sm_m[wave] = m_run;
    sm_l[wave] = l_run;
  }
  __syncthreads();
  if (wave == 0) {
    const float m = fmaxf(fmaxf(sm_m[0], sm_m[1]), fmaxf(sm_m[2], sm_m[3]));
    float l = 0.f, w4[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      w4[w] = (sm_m[w] == -INFINITY) ? 0.f : fast_exp2(sm_m[w] - m);
      l += sm_l[w] * w4[w];
    }
    float* dst = part + (((size_t)blockIdx.y * heads + head) * nsplit + split) * (HD + 2);
    if (lane == 0) {
      dst[0] = m;
      dst[1] = l;
    }
#pragma unroll
    for (int i = 0; i < HD / 64; ++i) {
      const int d = lane + 64 * i;
      float o = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) o += sm_o[w][d] * w4[w];
      dst[2 + d] = o;
    }
  }
}

// the split combine: attn_decode_combine_kernel of vt_attn.hip, same arithmetic in the same order
template <int HD>
__global__ __launch_bounds__(64) void attn_decode_kv8_combine_kernel(const float* __restrict__ part, const VtAttnSeq* __restrict__ seqs,
                                                                     bf16_t* __restrict__ O, int ldo, int heads, int nsplit) {
  const int head = blockIdx.x, seq = blockIdx.y, lane = threadIdx.x;
  const float* src = part + ((size_t)seq * heads + head) * nsplit * (HD + 2);
  float m = -INFINITY;
  for (int s = 0; s < nsplit; ++s) m = fmaxf(m, src[s * (HD + 2)]);
  float l = 0.f, o[HD / 64];
#pragma unroll
  for (int i = 0; i < HD / 64; ++i) o[i] = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float ms = src[s * (HD + 2)];
    const float w = (ms == -INFINITY) ? 0.f : fast_exp2(ms - m);
    l += src[s * (HD + 2) + 1] * w;
#pragma unroll
    for (int i = 0; i < HD / 64; ++i) o[i] += src[s * (HD + 2) + 2 + lane + 64 * i] * w;
  }
  const float inv = l > 0.f ? 1.f / l : 0.f;
  bf16_t* op = O + (size_t)seqs[seq].q_row0 * ldo + head * HD;
#pragma unroll
  for (int i = 0; i < HD / 64; ++i) op[lane + 64 * i] = f32_to_op(o[i] * inv);
}

// ------------------------------------------------------------------------------------------------------------------
// attn_decode_fused_kv8_kernel: attn_decode_fused_kernel (vt_attn.hip) on e4m3 pages -- one decode step of one layer in ONE launch:
// rotary embedding of the new q and k (same fp32 arithmetic, rounded once to the operand format), the new k row and v column quantised
// and stored, single-query attention over the cache, in-block combine. No scratch.
//   grid (head, sequence), 8 waves per block: wave w owns tiles w, w + 8, ...; lane -> key mapping, reduce-scatter and PV layout are
//   attn_decode_kv8_kernel's (K row = CH = HD / 16 lanes x 16 B, V^T row = 4 lanes x 16 B). The first tile's requests go out before the
//   rotary prologue.
//   The wave that owns the LAST tile owns the new token. The token is SCORED FROM ITS QUANTISED VALUE and its v enters the output as
//   the quantised byte's value: the step computes what attn_decode_kv8_kernel computes on the cache the step leaves behind. As in the
//   16-bit kernel the new token's weight is taken out of the tile's row of probabilities and applied to the value held in LDS, so a
//   step repeated at the same position is idempotent; a tile that STARTS with the new token is zero-filled around it.
// ------------------------------------------------------------------------------------------------------------------
template <int HD, bool ROPE>
__global__ __launch_bounds__(512) void attn_decode_fused_kv8_kernel(
    const bf16_t* __restrict__ qkv, int ldqkv, int q_col0, int k_col0, int v_col0, uint8_t* __restrict__ K8, uint8_t* __restrict__ V8,
    const int* __restrict__ tile_table, const VtAttnSeq* __restrict__ seqs, int heads, const float* __restrict__ rope_cos,
    const float* __restrict__ rope_sin, const int* __restrict__ positions, float scale_log2e, bf16_t* __restrict__ O, int ldo) {
  constexpr int NW = 8;
  constexpr int CH = HD / 16, KPI = 64 / CH, NACC = HD / 16;
  __shared__ float sm_m[NW], sm_l[NW];
  __shared__ float sm_o[NW][HD];
  __shared__ __attribute__((aligned(16))) float sm_p[NW][64];
  __shared__ __attribute__((aligned(16))) uint8_t sm_v[HD];
  const VtAttnSeq sq = seqs[blockIdx.y];
  const int head = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int past = sq.kv_len - 1;
  const int t_last = past >> 6, r_new = past & 63, ntiles = t_last + 1;
  const bf16_t* qrow = qkv + (size_t)sq.q_row0 * ldqkv;
  const int c = lane % CH, ch = c % (CH / 2);
  const bool upper = c >= CH / 2;
  constexpr bool rope = ROPE;
  const int vrow = lane >> 2, vchk = lane & 3;
  const int key_of_lane = c * KPI + lane / CH;
  float m_run = -INFINITY, l_run = 0.f, acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.f;

  u32x4 kk[CH], vv[NACC];
  auto issue = [&](int t) {
    const size_t toff = ((size_t)tile_table[sq.table_off + t] * heads + head) * 64 * HD;
    if (t == t_last && r_new == 0) {   // tile starts with the new token: nothing to read (it is zero-filled below)
#pragma unroll
      for (int i = 0; i < CH; ++i) kk[i] = (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
      for (int i = 0; i < NACC; ++i) vv[i] = (u32x4){0u, 0u, 0u, 0u};
    } else {
#pragma unroll
      for (int i = 0; i < CH; ++i)
        kk[i] = __builtin_nontemporal_load((const u32x4*)(K8 + toff + (i * KPI + lane / CH) * HD + c * 16));
#pragma unroll
      for (int i = 0; i < NACC; ++i)
        vv[i] = __builtin_nontemporal_load((const u32x4*)(V8 + toff + (i * 16 + vrow) * 64 + vchk * 16));
    }
    return toff;
  };
  float cs[16], sn[16];
  if (rope) {
    const int rp = positions[sq.q_row0];
    const float* cp = rope_cos + (size_t)rp * (HD / 2) + ch * 16;
    const float* sp = rope_sin + (size_t)rp * (HD / 2) + ch * 16;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      cs[j] = cp[j];
      sn[j] = sp[j];
    }
  }
  // this lane's 16 elements (d = 16c ..) of a head row as 8 packed operand pairs, rotated (half-split rotary; the arithmetic and the
  // rounding to the operand format are kv_tiles_kernel's)
  auto rotate = [&](const u32x4* lo, const u32x4* hi, uint32_t (&o)[8]) {
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      const uint32_t lw = lo[w >> 2][w & 3], hw = hi[w >> 2][w & 3];
      const float a0 = oplo_to_f32(lw), a1 = ophi_to_f32(lw);
      const float b0 = oplo_to_f32(hw), b1 = ophi_to_f32(hw);
      const float c0 = cs[2 * w], c1 = cs[2 * w + 1], s0 = sn[2 * w], s1 = sn[2 * w + 1];
      o[w] = upper ? pack_op2(rope_hi(a0, b0, c0, s0), rope_hi(a1, b1, c1, s1)) : pack_op2(rope_lo(a0, b0, c0, s0), rope_lo(a1, b1, c1, s1));
    }
  };
  auto head_chunk = [&](const bf16_t* base, uint32_t (&o)[8]) {
    if (!rope) {
      const u32x4 a = *(const u32x4*)(base + c * 16), b = *(const u32x4*)(base + c * 16 + 8);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        o[w] = a[w];
        o[4 + w] = b[w];
      }
    } else {
      const u32x4 lo[2] = {*(const u32x4*)(base + ch * 16), *(const u32x4*)(base + ch * 16 + 8)};
      const u32x4 hi[2] = {*(const u32x4*)(base + HD / 2 + ch * 16), *(const u32x4*)(base + HD / 2 + ch * 16 + 8)};
      rotate(lo, hi, o);
    }
  };
  // raw q chunks first, then the first tile's requests, then the rotary arithmetic: loads complete in issue order, so the prologue
  // only waits for its own small look-ups while the tile is in flight
  const bf16_t* qbase = qrow + q_col0 + head * HD;
  const int qo = (rope ? ch : c) * 16;
  const u32x4 q_lo[2] = {*(const u32x4*)(qbase + qo), *(const u32x4*)(qbase + qo + 8)};
  const u32x4 q_hi[2] = {*(const u32x4*)(qbase + (rope ? HD / 2 : 0) + qo), *(const u32x4*)(qbase + (rope ? HD / 2 : 0) + qo + 8)};
  __builtin_amdgcn_sched_barrier(0);
  int t = wave;
  size_t toff = 0;
  if (t < ntiles) toff = issue(t);
  __builtin_amdgcn_sched_barrier(0);
  uint32_t qv[8];
  if (rope) {
    rotate(q_lo, q_hi, qv);
  } else {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      qv[w] = q_lo[0][w];
      qv[4 + w] = q_lo[1][w];
    }
  }
  float qf[16];
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    qf[2 * w] = oplo_to_f32(qv[w]);
    qf[2 * w + 1] = ophi_to_f32(qv[w]);
  }
  __builtin_amdgcn_sched_barrier(0);

  while (t < ntiles) {
    const bool is_last = t == t_last;
    const bool fresh = is_last && r_new == 0;
    uint8_t* kt = K8 + toff;
    uint8_t* vt = V8 + toff;
    float ps[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) ps[i] = kv8_dot16(kk[i], qf);
    float s_mine = reduce_scatter_lanes<CH>(ps, c);   // full score of key_of_lane = c * KPI + lane / CH
    if (is_last) {
      // ---- the new token: key r_new of this tile, quantised first, scored from the bytes it stores ----
      uint32_t kr[8];
      head_chunk(qrow + k_col0 + head * HD, kr);
      u32x4 k8;
#pragma unroll
      for (int w = 0; w < 4; ++w)
        k8[w] = kv8_pack4(oplo_to_f32(kr[2 * w]), ophi_to_f32(kr[2 * w]), oplo_to_f32(kr[2 * w + 1]), ophi_to_f32(kr[2 * w + 1]));
      float part_s = allreduce_lanes<CH>(kv8_dot16(k8, qf));
      if (key_of_lane == r_new) s_mine = part_s;
      if (lane < CH) {   // lane < CH: c == lane
        *(u32x4*)(kt + r_new * HD + lane * 16) = k8;
        const bf16_t* vp = qrow + v_col0 + head * HD + lane * 16;   // operand from the projection -> the fp16 page value -> e4m3
        const u32x4 va = *(const u32x4*)vp, vb = *(const u32x4*)(vp + 8);
        u32x4 v8;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
          const uint32_t a0 = op2_to_f16x2(va[2 * w]), a1 = op2_to_f16x2(va[2 * w + 1]);
          const uint32_t b0 = op2_to_f16x2(vb[2 * w]), b1 = op2_to_f16x2(vb[2 * w + 1]);
          v8[w] = kv8_pack4(f16lo_to_f32(a0), f16hi_to_f32(a0), f16lo_to_f32(a1), f16hi_to_f32(a1));
          v8[2 + w] = kv8_pack4(f16lo_to_f32(b0), f16hi_to_f32(b0), f16lo_to_f32(b1), f16hi_to_f32(b1));
        }
        *(u32x4*)(&sm_v[lane * 16]) = v8;
      }
      __builtin_amdgcn_wave_barrier();
      if (!fresh) {
#pragma unroll
        for (int i = 0; i < HD / 64; ++i) vt[(lane + 64 * i) * 64 + r_new] = sm_v[lane + 64 * i];
      } else {
        const u32x4 z = {0u, 0u, 0u, 0u};
        for (int it = lane; it < 63 * CH; it += 64) *(u32x4*)(kt + HD + it * 16) = z;      // K rows 1..63
        for (int it = lane; it < HD * 4; it += 64) {                                        // V^T: (d, 16-key chunk)
          const int d = it >> 2, kc = it & 3;
          u32x4 w = z;
          if (kc == 0) w.x = sm_v[d];
          *(u32x4*)(vt + d * 64 + kc * 16) = w;
        }
      }
    }
    const int mykey = t * 64 + key_of_lane;
    const float s2 = (mykey < sq.kv_len) ? s_mine * scale_log2e : -INFINITY;
    const float m_new = fmaxf(m_run, wave_max(s2));
    const float alpha = fast_exp2(m_run - m_new);
    const float p = fast_exp2(s2 - m_new);
    l_run = l_run * alpha + wave_sum(p);
    m_run = m_new;
    sm_p[wave][key_of_lane] = p;
    __builtin_amdgcn_wave_barrier();
    float p_new = 0.f;
    if (is_last) {
      p_new = sm_p[wave][r_new];
      __builtin_amdgcn_wave_barrier();
      if (key_of_lane == r_new) sm_p[wave][r_new] = 0.f;
      __builtin_amdgcn_wave_barrier();
    }
    float pk[16];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const f32x4 pv = *(const f32x4*)(&sm_p[wave][vchk * 16 + 4 * w]);
#pragma unroll
      for (int j = 0; j < 4; ++j) pk[4 * w + j] = pv[j];
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = kv8_pv16(acc[i], alpha, vv[i], pk);
    if (is_last && vchk == 0) {   // column r_new of the loaded tile carries no weight (see above): add the new value here
#pragma unroll
      for (int i = 0; i < NACC; ++i) acc[i] = fmaf(kv8_byte_to_f32(sm_v[i * 16 + vrow]), p_new, acc[i]);
    }
    t += NW;
    if (t < ntiles) toff = issue(t);
  }
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    float a = acc[i];
    a += __shfl_xor(a, 1, 64);
    a += __shfl_xor(a, 2, 64);
    if (vchk == 0) sm_o[wave][i * 16 + vrow] = a;
  }
  if (lane == 0) {
    sm_m[wave] = m_run;
    sm_l[wave] = l_run;
  }
  __syncthreads();
  if (threadIdx.x < HD) {
    float m = sm_m[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) m = fmaxf(m, sm_m[w]);
    float l = 0.f, o = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float wt = (sm_m[w] == -INFINITY) ? 0.f : fast_exp2(sm_m[w] - m);
      l += sm_l[w] * wt;
      o += sm_o[w][threadIdx.x] * wt;
    }
    O[(size_t)sq.q_row0 * ldo + head * HD + threadIdx.x] = f32_to_op(l > 0.f ? o / l : 0.f);
  }
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
  const int ntiles = (max_kv_len + 63) / 64;
  int nsplit = (ntiles + 3) / 4;
  nsplit = nsplit < 1 ? 1 : (nsplit > 32 ? 32 : nsplit);
  const size_t need = vt_attn_decode_scratch_bytes(nseq, heads, HD, max_kv_len);
  if (scratch_bytes < need) {
    vt_set_error("vt_attn_decode_kv8: scratch too small (%zu < %zu)", scratch_bytes, need);
    return VT_ERR_WORKSPACE;
  }
  const float sl2 = scale * 1.4426950408889634f;
  VtProfScope prof(VT_PROF_ATTN_DECODE, 0.0, s);
  dim3 grid(heads, nseq, nsplit), block(256);
  if (HD == 64) {
    hipLaunchKernelGGL((attn_decode_kv8_kernel<64>), grid, block, 0, s, Q, ldq, K8, V8, tile_table, seqs, heads, sl2, scratch, nsplit);
    hipLaunchKernelGGL((attn_decode_kv8_combine_kernel<64>), dim3(heads, nseq), dim3(64), 0, s, scratch, seqs, O, ldo, heads, nsplit);
  } else {
    hipLaunchKernelGGL((attn_decode_kv8_kernel<128>), grid, block, 0, s, Q, ldq, K8, V8, tile_table, seqs, heads, sl2, scratch, nsplit);
    hipLaunchKernelGGL((attn_decode_kv8_combine_kernel<128>), dim3(heads, nseq), dim3(64), 0, s, scratch, seqs, O, ldo, heads, nsplit);
  }
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
