// vt_attn_decode.h -- single-query (decode) attention over the paged KV tiles, written ONCE for every page format (gfx950 / CDNA4).
//
// The __global__ kernels live beside their page format and are one-line calls of the two bodies below:
//   vt_attn.hip : attn_decode_kernel / attn_decode_fused_kernel on 16-bit pages (trait DecodePages16), and the format-free
//                 attn_decode_combine_kernel
//   vt_kv8.hip  : attn_decode_kv8_kernel / attn_decode_fused_kv8_kernel on e4m3 pages (trait DecodePagesE4M3)
//
// A page format is a trait F that supplies only what differs between formats:
//   F::elem_t                  one page element (K page [64 keys][HD], V^T page [HD][64 keys]); also the type of the new v column in LDS
//   F::EPC                     elements per 16-byte chunk -- every index below is derived from it
//   F::dot(chunk, qf)          fp32 score partial of one K chunk against this lane's EPC q values: one fmaf chain in element order
//   F::pv(acc, alpha, chunk, p) acc * alpha, then one fmaf chain over the chunk's EPC keys in order
//   F::pack_k(words)           EPC operand values (EPC / 2 packed pairs) -> the stored K chunk; the new token is scored through dot() on
//                              what pack_k returns, i.e. from the value every later step reads
//   F::pack_v(words)           EPC operand values -> fp16 page value -> the stored V^T elements
//   F::v_to_f32(elem)          one V^T element as a float
//
// Geometry (DecodeGeom): a K row is CH = HD / EPC chunks, so CH lanes cooperate on one key and one wave-instruction covers KPI = 64 / CH
// keys; a tile takes CH instructions. Lane (c = lane % CH, g = lane / CH) holds elements c * EPC .. of rows i * KPI + g; its CH partial
// sums are reduce-scattered over the CH lanes (CH - 1 DPP / swizzle exchanges per tile), after which the lane owns key c * KPI + g.
// A V^T row (64 keys) is LPV = 64 / EPC chunks, one wave-instruction covers RPI = 64 / LPV full rows, a tile takes NACC = HD / RPI
// instructions. Lane (vchk = lane % LPV, vrow = lane / LPV) holds keys vchk * EPC .. of rows i * RPI + vrow and keeps NACC partial
// accumulators (EPC + 1 roundings per tile each: the alpha product and EPC fmaf); the LPV lanes of a row meet ONCE after the last tile.
// The kernels are HBM-bound: the whole job is to stream K and V^T tiles once, 16 B per lane, fully coalesced, non-temporal, with a
// whole tile requested before anything of it is consumed.
#pragma once
#include "vt_kernels.h"

// lane ^ MASK exchange inside groups of 16 lanes without an LDS address: DPP quad_perm (1, 2), row_ror:8 (8), ds_swizzle (4)
template <int MASK>
__device__ __forceinline__ float lane_xor16(float v) {
  int x = __builtin_bit_cast(int, v);
  if constexpr (MASK == 1) x = __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true);
  else if constexpr (MASK == 2) x = __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true);
  else if constexpr (MASK == 8) x = __builtin_amdgcn_update_dpp(0, x, 0x128, 0xF, 0xF, true);
  else x = __builtin_amdgcn_ds_swizzle(x, (MASK << 10) | 0x1F);
  return __builtin_bit_cast(float, x);
}
// CH lanes (c = lane % CH) each hold CH partial sums part[i]; on return part[0] is the FULL sum of value i == c.
// Recursive halving: CH - 1 exchanges instead of CH * log2(CH) for one butterfly per value.
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
  VT_RS_STEP(8)
  VT_RS_STEP(4)
  VT_RS_STEP(2)
  VT_RS_STEP(1)
#undef VT_RS_STEP
  return part[0];
}
template <int CH>
__device__ __forceinline__ float allreduce_lanes(float v) {
  if constexpr (CH >= 16) v += lane_xor16<8>(v);
  if constexpr (CH >= 8) v += lane_xor16<4>(v);
  v += lane_xor16<2>(v);
  v += lane_xor16<1>(v);
  return v;
}

template <class F, int HD>
struct DecodeGeom {
  static constexpr int EPC = F::EPC;       // elements per 16-byte chunk
  static constexpr int CH = HD / EPC;      // chunks per K row; CH lanes cooperate on one key
  static constexpr int KPI = 64 / CH;      // keys per wave-instruction
  static constexpr int LPV = 64 / EPC;     // lanes (chunks) per V^T row
  static constexpr int RPI = 64 / LPV;     // V^T rows per wave-instruction
  static constexpr int NACC = HD / EPC;    // V^T rows handled per lane (one per PV instruction)
  static constexpr int NQ = EPC / 8;       // 16-byte loads of 16-bit operands behind one lane's EPC elements
  static_assert(sizeof(typename F::elem_t) * EPC == 16, "a chunk is 16 bytes");
  static_assert(CH * KPI == 64 && LPV * EPC == 64 && NACC * RPI == HD, "a wave-instruction covers whole rows");
  static_assert(HD % (2 * EPC) == 0, "the rotary halves of a head row split on a chunk boundary");
  static_assert(EPC % 8 == 0, "operands arrive as 16-byte loads of eight");
};

// ---- the per-tile step, shared by both bodies -----------------------------------------------------------------------------------
// request one whole tile: CH + NACC 16-byte non-temporal loads per lane
template <class F, int HD>
__device__ __forceinline__ void decode_request_tile(const typename F::elem_t* kt, const typename F::elem_t* vt, int lane,
                                                    u32x4 (&kk)[DecodeGeom<F, HD>::CH], u32x4 (&vv)[DecodeGeom<F, HD>::NACC]) {
  typedef DecodeGeom<F, HD> G;
  const int c = lane % G::CH, vrow = lane / G::LPV, vchk = lane % G::LPV;
#pragma unroll
  for (int i = 0; i < G::CH; ++i)
    kk[i] = __builtin_nontemporal_load((const u32x4*)(kt + (i * G::KPI + lane / G::CH) * HD + c * G::EPC));
#pragma unroll
  for (int i = 0; i < G::NACC; ++i)
    vv[i] = __builtin_nontemporal_load((const u32x4*)(vt + (i * G::RPI + vrow) * 64 + vchk * G::EPC));
}
// the tile's 64 scores: on return this lane owns the full score of key (lane % CH) * KPI + lane / CH
template <class F, int HD>
__device__ __forceinline__ float decode_scores(const u32x4 (&kk)[DecodeGeom<F, HD>::CH], const float (&qf)[F::EPC], int c) {
  constexpr int CH = DecodeGeom<F, HD>::CH;
  float part[CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) part[i] = F::dot(kk[i], qf);
  return reduce_scatter_lanes<CH>(part, c);
}
// one online-softmax step over the tile's 64 keys (one per lane); returns this lane's probability, alpha rescales what came before
__device__ __forceinline__ float decode_softmax_step(float s_mine, bool in_range, float scale_log2e, float& m_run, float& l_run,
                                                     float& alpha) {
  const float s2 = in_range ? s_mine * scale_log2e : -INFINITY;
  const float m_new = fmaxf(m_run, wave_max(s2));
  alpha = fast_exp2(m_run - m_new);
  const float p = fast_exp2(s2 - m_new);
  l_run = l_run * alpha + wave_sum(p);
  m_run = m_new;
  return p;
}
// the row of probabilities comes back from LDS in V^T order (this lane's EPC keys), then acc = acc * alpha + P.V per owned row.
// The caller has fenced its writes to sm_p with a wave_barrier: DS ops of one wave are in order, the barriers only stop the compiler.
template <class F, int HD>
__device__ __forceinline__ void decode_pv(const float (&sm_p)[64], int vchk, float alpha, const u32x4 (&vv)[DecodeGeom<F, HD>::NACC],
                                          float (&acc)[DecodeGeom<F, HD>::NACC]) {
  typedef DecodeGeom<F, HD> G;
  float pk[G::EPC];
#pragma unroll
  for (int w = 0; w < G::EPC / 4; ++w) {
    const f32x4 pv = *(const f32x4*)(&sm_p[vchk * G::EPC + 4 * w]);
#pragma unroll
    for (int j = 0; j < 4; ++j) pk[4 * w + j] = pv[j];
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < G::NACC; ++i) acc[i] = F::pv(acc[i], alpha, vv[i], pk);
}
// after the last tile: the sum over the LPV lanes that share a V^T row (every one of them gets it)
template <int LPV>
__device__ __forceinline__ float decode_row_sum(float a) {
#pragma unroll
  for (int m = 1; m < LPV; m <<= 1) a += __shfl_xor(a, m, 64);
  return a;
}

// ------------------------------------------------------------------------------------------------------------------
// attn_decode_split_body: single-query attention over an existing cache, flash-decoding style.
//   grid (head, sequence, split); 4 waves per block; wave w of split s owns tiles t = 4*s + w, 4*s + w + 4*nsplit, ...
//   each block writes an online-softmax partial (m, l, o[HD]) to scratch; attn_decode_combine_kernel merges the splits.
// ------------------------------------------------------------------------------------------------------------------
template <class F, int HD>
__device__ __forceinline__ void attn_decode_split_body(const bf16_t* __restrict__ Q, int ldq, const typename F::elem_t* __restrict__ Kt,
                                                       const typename F::elem_t* __restrict__ Vt, const int* __restrict__ tile_table,
                                                       const VtAttnSeq* __restrict__ seqs, int heads, float scale_log2e,
                                                       float* __restrict__ part, int nsplit) {
  typedef DecodeGeom<F, HD> G;
  constexpr int EPC = G::EPC, CH = G::CH, KPI = G::KPI, NACC = G::NACC, LPV = G::LPV, RPI = G::RPI;
  __shared__ float sm_m[4], sm_l[4];
  __shared__ float sm_o[4][HD];
  __shared__ __attribute__((aligned(16))) float sm_p[4][64];
  const VtAttnSeq sq = seqs[blockIdx.y];
  const int head = blockIdx.x, split = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ntiles = (sq.kv_len + 63) >> 6;
  const bf16_t* qp = Q + (size_t)sq.q_row0 * ldq + head * HD;
  const int c = lane % CH;
  float qf[EPC];
#pragma unroll
  for (int h = 0; h < G::NQ; ++h) {
    const u32x4 qv = *(const u32x4*)(qp + c * EPC + h * 8);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      qf[8 * h + 2 * w] = oplo_to_f32(qv[w]);
      qf[8 * h + 2 * w + 1] = ophi_to_f32(qv[w]);
    }
  }
  float m_run = -INFINITY, l_run = 0.f, acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.f;
  const int vrow = lane / LPV, vchk = lane % LPV;
  const int key_of_lane = c * KPI + lane / CH;   // the key (inside a tile) whose score this lane ends up owning

  for (int t = split * 4 + wave; t < ntiles; t += 4 * nsplit) {
    const size_t toff = ((size_t)tile_table[sq.table_off + t] * heads + head) * 64 * HD;
    u32x4 kk[CH], vv[NACC];
    decode_request_tile<F, HD>(Kt + toff, Vt + toff, lane, kk, vv);
    __builtin_amdgcn_sched_barrier(0);
    const float s_mine = decode_scores<F, HD>(kk, qf, c);
    float alpha;
    const float p = decode_softmax_step(s_mine, t * 64 + key_of_lane < sq.kv_len, scale_log2e, m_run, l_run, alpha);
    sm_p[wave][key_of_lane] = p;
    __builtin_amdgcn_wave_barrier();
    decode_pv<F, HD>(sm_p[wave], vchk, alpha, vv, acc);
  }
  // this wave's partial (m, l, o[HD]) goes to LDS, where the waves meet
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const float a = decode_row_sum<LPV>(acc[i]);
    if (vchk == 0) sm_o[wave][i * RPI + vrow] = a;
  }
  if (lane == 0) {
    sm_m[wave] = m_run;
    sm_l[wave] = l_run;
  }
  __syncthreads();
  if (wave == 0) {   // combine the 4 waves
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

// ------------------------------------------------------------------------------------------------------------------
// attn_decode_fused_body: the whole attention part of one decode step of one layer in ONE launch (q_len == 1):
//   rotary embedding of the new q and k rows (fp32 arithmetic, rounded once to the operand format, as kv_tiles_kernel), append of
//   the new k row / v column to the paged tiles, single-query attention over the cache, combine. Replaces kv_tiles + attn_decode +
//   attn_decode_combine (3 launches, 2 boundaries).
//   grid (head, sequence), 8 waves per block: wave w owns tiles w, w + 8, ... of its (sequence, head) and streams them with the
//   split body's per-tile step; the 8 online-softmax partials meet in LDS -- no scratch, no cross-block traffic. One head of one
//   sequence is <= 1 MiB of 16-bit K/V^T at 2048 tokens, which one CU streams in a few microseconds.
//   The wave that owns the LAST tile also owns the new token: it rotates k, packs it to the page format (F::pack_k), scores the
//   packed chunk from registers, stores the k row and the v column, and adds p_new * v_new to its accumulators -- so the step
//   computes what the split kernel computes on the cache the step leaves behind. A tile that STARTS with the new token is
//   zero-filled around it (same invariant as kv_tiles_kernel: padding rows/columns of a tile are zero, never garbage).
// ------------------------------------------------------------------------------------------------------------------
template <class F, int HD, bool ROPE>
__device__ __forceinline__ void attn_decode_fused_body(
    const bf16_t* __restrict__ qkv, int ldqkv, int q_col0, int k_col0, int v_col0, typename F::elem_t* __restrict__ Kt,
    typename F::elem_t* __restrict__ Vt, const int* __restrict__ tile_table, const VtAttnSeq* __restrict__ seqs, int heads,
    const float* __restrict__ rope_cos, const float* __restrict__ rope_sin, const int* __restrict__ positions, float scale_log2e,
    bf16_t* __restrict__ O, int ldo) {
  typedef DecodeGeom<F, HD> G;
  typedef typename F::elem_t elem_t;
  constexpr int NW = 8;
  constexpr int EPC = G::EPC, CH = G::CH, KPI = G::KPI, NACC = G::NACC, LPV = G::LPV, RPI = G::RPI, NQ = G::NQ;
  __shared__ float sm_m[NW], sm_l[NW];
  __shared__ float sm_o[NW][HD];
  __shared__ __attribute__((aligned(16))) float sm_p[NW][64];
  __shared__ __attribute__((aligned(16))) elem_t sm_v[HD];
  const VtAttnSeq sq = seqs[blockIdx.y];
  const int head = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int past = sq.kv_len - 1;
  const int t_last = past >> 6, r_new = past & 63, ntiles = t_last + 1;
  const bf16_t* qrow = qkv + (size_t)sq.q_row0 * ldqkv;
  const int c = lane % CH, ch = c % (CH / 2);
  const bool upper = c >= CH / 2;
  constexpr bool rope = ROPE;
  const int vrow = lane / LPV, vchk = lane % LPV;
  const int key_of_lane = c * KPI + lane / CH;   // the key (inside a tile) whose score this lane ends up owning
  float m_run = -INFINITY, l_run = 0.f, acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.f;

  // the whole tile is requested before anything is consumed; the first tile's requests go out before the rotary prologue so
  // that its three dependent look-ups (positions -> tables, q row) overlap the K/V latency
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
        kk[i] = __builtin_nontemporal_load((const u32x4*)(Kt + toff + (i * KPI + lane / CH) * HD + c * EPC));
#pragma unroll
      for (int i = 0; i < NACC; ++i)
        vv[i] = __builtin_nontemporal_load((const u32x4*)(Vt + toff + (i * RPI + vrow) * 64 + vchk * EPC));
    }
    return toff;
  };
  float cs[EPC], sn[EPC];
  if (rope) {
    const int rp = positions[sq.q_row0];
    const float* cp = rope_cos + (size_t)rp * (HD / 2) + ch * EPC;
    const float* sp = rope_sin + (size_t)rp * (HD / 2) + ch * EPC;
#pragma unroll
    for (int j = 0; j < EPC; ++j) {
      cs[j] = cp[j];
      sn[j] = sp[j];
    }
  }
  // this lane's EPC elements (d = c * EPC ..) of a head row as EPC / 2 packed operand pairs, rotated (half-split rotary, same
  // arithmetic and rounding to the operand format as kv_tiles_kernel)
  auto rotate = [&](const u32x4 (&lo)[NQ], const u32x4 (&hi)[NQ], uint32_t (&o)[EPC / 2]) {
#pragma unroll
    for (int w = 0; w < EPC / 2; ++w) {
      const uint32_t lw = lo[w >> 2][w & 3], hw = hi[w >> 2][w & 3];
      const float a0 = oplo_to_f32(lw), a1 = ophi_to_f32(lw);
      const float b0 = oplo_to_f32(hw), b1 = ophi_to_f32(hw);
      const float c0 = cs[2 * w], c1 = cs[2 * w + 1], s0 = sn[2 * w], s1 = sn[2 * w + 1];
      o[w] = upper ? pack_op2(rope_hi(a0, b0, c0, s0), rope_hi(a1, b1, c1, s1)) : pack_op2(rope_lo(a0, b0, c0, s0), rope_lo(a1, b1, c1, s1));
    }
  };
  // this lane's EPC operand values at base + off, unrotated
  auto load_words = [&](const bf16_t* base, int off, u32x4 (&o)[NQ]) {
#pragma unroll
    for (int h = 0; h < NQ; ++h) o[h] = *(const u32x4*)(base + off + h * 8);
  };
  auto unpack_words = [&](const u32x4 (&v)[NQ], uint32_t (&o)[EPC / 2]) {
#pragma unroll
    for (int w = 0; w < EPC / 2; ++w) o[w] = v[w >> 2][w & 3];
  };
  auto head_chunk = [&](const bf16_t* base, uint32_t (&o)[EPC / 2]) {
    u32x4 lo[NQ], hi[NQ];
    if (!rope) {
      load_words(base, c * EPC, lo);
      unpack_words(lo, o);
    } else {
      load_words(base, ch * EPC, lo);
      load_words(base, HD / 2 + ch * EPC, hi);
      rotate(lo, hi, o);
    }
  };
  // raw q chunks first, then the first tile's requests, then the rotary arithmetic: loads complete in issue order, so the
  // prologue only ever waits for its own small look-ups while the tile is in flight
  const bf16_t* qbase = qrow + q_col0 + head * HD;
  u32x4 q_lo[NQ], q_hi[NQ];
  load_words(qbase, (rope ? ch : c) * EPC, q_lo);
  load_words(qbase, rope ? HD / 2 + ch * EPC : c * EPC, q_hi);
  __builtin_amdgcn_sched_barrier(0);
  int t = wave;
  size_t toff = 0;
  if (t < ntiles) toff = issue(t);
  __builtin_amdgcn_sched_barrier(0);
  uint32_t qv[EPC / 2];
  if (rope) rotate(q_lo, q_hi, qv);
  else unpack_words(q_lo, qv);
  float qf[EPC];
#pragma unroll
  for (int w = 0; w < EPC / 2; ++w) {
    qf[2 * w] = oplo_to_f32(qv[w]);
    qf[2 * w + 1] = ophi_to_f32(qv[w]);
  }
  __builtin_amdgcn_sched_barrier(0);

  while (t < ntiles) {
    const bool is_last = t == t_last;
    const bool fresh = is_last && r_new == 0;
    elem_t* kt = Kt + toff;
    elem_t* vt = Vt + toff;
    float s_mine = decode_scores<F, HD>(kk, qf, c);
    if (is_last) {
      // ---- the new token: key r_new of this tile, packed first, scored from the chunk it stores ----
      uint32_t kr[EPC / 2];
      head_chunk(qrow + k_col0 + head * HD, kr);
      const u32x4 kc = F::pack_k(kr);
      const float part_s = allreduce_lanes<CH>(F::dot(kc, qf));
      if (key_of_lane == r_new) s_mine = part_s;
      if (lane < CH) {   // lane < CH: c == lane
        *(u32x4*)(kt + r_new * HD + lane * EPC) = kc;
        u32x4 vn[NQ];   // operand from the projection -> the fp16 page value -> the page element
        load_words(qrow + v_col0 + head * HD, lane * EPC, vn);
        uint32_t vw[EPC / 2];
        unpack_words(vn, vw);
        *(u32x4*)(&sm_v[lane * EPC]) = F::pack_v(vw);
      }
      __builtin_amdgcn_wave_barrier();
      if (!fresh) {
#pragma unroll
        for (int i = 0; i < HD / 64; ++i) vt[(lane + 64 * i) * 64 + r_new] = sm_v[lane + 64 * i];
      } else {
        const u32x4 z = {0u, 0u, 0u, 0u};
        for (int it = lane; it < 63 * CH; it += 64) *(u32x4*)(kt + HD + it * EPC) = z;      // K rows 1..63
        for (int it = lane; it < HD * LPV; it += 64) {                                       // V^T: (d, EPC-key chunk)
          const int d = it / LPV, kc0 = it % LPV;
          u32x4 w = z;
          if (kc0 == 0) w.x = sm_v[d];
          *(u32x4*)(vt + d * 64 + kc0 * EPC) = w;
        }
      }
    }
    float alpha;
    const float p = decode_softmax_step(s_mine, t * 64 + key_of_lane < sq.kv_len, scale_log2e, m_run, l_run, alpha);
    sm_p[wave][key_of_lane] = p;
    __builtin_amdgcn_wave_barrier();
    float p_new = 0.f;
    if (is_last) {
      // the new token's value comes from sm_v below, never from the loaded tile: its weight is taken out of the tile's row of
      // probabilities, so a column r_new that already holds a value (a step that was rolled back and is run again) is not
      // counted twice and the kernel is idempotent
      p_new = sm_p[wave][r_new];
      __builtin_amdgcn_wave_barrier();
      if (key_of_lane == r_new) sm_p[wave][r_new] = 0.f;
      __builtin_amdgcn_wave_barrier();
    }
    decode_pv<F, HD>(sm_p[wave], vchk, alpha, vv, acc);
    if (is_last && vchk == 0) {   // column r_new of the loaded tile carries no weight (see above): add the new value here
#pragma unroll
      for (int i = 0; i < NACC; ++i) acc[i] = fmaf(F::v_to_f32(sm_v[i * RPI + vrow]), p_new, acc[i]);
    }
    t += NW;
    if (t < ntiles) toff = issue(t);
  }
  // this wave's partial (m, l, o[HD]) goes to LDS, where the waves meet
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const float a = decode_row_sum<LPV>(acc[i]);
    if (vchk == 0) sm_o[wave][i * RPI + vrow] = a;
  }
  if (lane == 0) {
    sm_m[wave] = m_run;
    sm_l[wave] = l_run;
  }
  __syncthreads();
  if (threadIdx.x < HD) {   // combine the waves
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
