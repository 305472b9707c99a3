// vt_rows.h -- the block primitives of the row kernels: kernels that run ONE 1024-thread block (16 waves) per fp32
// logit row -- vt_argmax and the cross entropy (vt_llama.hip), the samplers (vt_sample.hip), vt_beam_step's stage 1, vt_logprob_rows, vt_cfg_rows,
// vt_dola_rows.
// Device only. These kernels' outputs are pinned bit for bit and several contracts are stated in terms of one another ("the lse is
// vt_logprob_rows' expression", "the mask follows vt_cfg_rows' layout"): this header is the one statement they all share, so the order
// of every reduction below is part of the contract. A new row kernel starts from here.
//   lse = m + logf(sum_i expf(x_i - m)), m = max x; fmaxf skips a NaN, the sum does not.
#pragma once
#include "vt_common.h"

constexpr int kRowThreads = 1024;
constexpr int kRowNone = 0x7fffffff;      // "no index": behind every real index in the (value, index) order

// ---- block reductions over N values at once ----------------------------------------------------------------------------------------
// 6 shuffle levels, then the 16 wave totals serially from LDS, slots 0..15 in that order. The N values share one pair of barriers;
// the first barrier lets the scratch of the previous call be reused. Every thread gets the result. sh: N x 16 slots of LDS.
template <int N>
__device__ __forceinline__ void row_block_max(float (&v)[N], float (*sh)[16]) {
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = wave_max(v[n]);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int n = 0; n < N; ++n) sh[n][threadIdx.x >> 6] = v[n];
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = sh[n][0];
  for (int i = 1; i < 16; ++i) {
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = fmaxf(v[n], sh[n][i]);
  }
}
template <int N, class T>       // T: float, or int for a count
__device__ __forceinline__ void row_block_sum(T (&v)[N], T (*sh)[16]) {
#pragma unroll
  for (int n = 0; n < N; ++n) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[n] += __shfl_xor(v[n], o, 64);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int n = 0; n < N; ++n) sh[n][threadIdx.x >> 6] = v[n];
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = 0;
  for (int i = 0; i < 16; ++i) {
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] += sh[n][i];
  }
}
// N = 1 by value
__device__ __forceinline__ float row_block_max(float v, float* sh) {
  float a[1] = {v};
  row_block_max(a, (float (*)[16])sh);
  return a[0];
}
__device__ __forceinline__ float row_block_sum(float v, float* sh) {
  float a[1] = {v};
  row_block_sum(a, (float (*)[16])sh);
  return a[0];
}
__device__ __forceinline__ int row_block_count(int c, int* sh) {
  int a[1] = {c};
  row_block_sum(a, (int (*)[16])sh);
  return a[0];
}

// ---- the (value, index) order: larger value first, exact ties by the lower index ---------------------------------------------------
// Every comparison with a NaN is false: a NaN is never taken. Two spellings of the take step that mean the same; which one a kernel
// uses is a matter of its registers alone (each was checked against the other with -Rpass-analysis=kernel-resource-usage):
//   RowTake, the select form: & and | on bools, the update as selects -- straight-line code (one v_cndmask per update), no branch per
//     candidate; `ok` gates the candidate. vt_logprob_rows.
//   RowTakeIf, the branch form. vt_beam_step (with selects the compiler keeps a scan's 32 unrolled candidates live at once:
//     beam_rows_kernel<true> 80 -> 102 VGPRs, 6 -> 4 waves per SIMD), vt_argmax (13 -> 23 VGPRs) and the samplers' greedy rows
//     (the register form of vt_sample_rows_adj: 16 -> 20 bytes of scratch).
struct RowTake {
  __device__ __forceinline__ void operator()(float& best, int& bi, float v, int i, bool ok = true) const {
    const bool t = ok & ((v > best) | ((v == best) & (i < bi)));
    best = t ? v : best;
    bi = t ? i : bi;
  }
};
struct RowTakeIf {
  __device__ __forceinline__ void operator()(float& best, int& bi, float v, int i) const {
    if (v > best || (v == best && i < bi)) {
      best = v;
      bi = i;
    }
  }
};
// is (v, i) strictly after (ls, li) in that order? (& and | for RowTake's `ok`; the branch form's callers write && and ||)
__device__ __forceinline__ bool row_after(float v, int i, float ls, int li) { return (v < ls) | ((v == ls) & (i > li)); }
template <class Take>
__device__ __forceinline__ void row_wave_argmax(float& best, int& bi, Take take) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    take(best, bi, ov, oi);
  }
}
// block-wide, result in THREAD 0 only, which goes on from its own wave's pair (vt_argmax, the greedy rows of the samplers). sv / si:
// 16 LDS slots each. ONE barrier, after the stores: the caller keeps the previous use of sv / si behind a barrier of its own.
// (The selection passes of vt_beam_step and vt_logprob_rows, which need the result in every thread pass after pass, alternate two
// pairs of buffers and keep that loop with their kernels.)
template <class Take>
__device__ __forceinline__ void row_block_argmax(float& best, int& bi, float* sv, int* si, Take take) {
  row_wave_argmax(best, bi, take);
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = best;
    si[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < 16; ++w) take(best, bi, sv[w], si[w]);
}

// ---- register form: a row of V <= 32 * 1024 floats, 16-byte aligned, in 32 registers per thread -------------------------------------
// Thread t owns the floats 4 (t + 1024 j) + k in slot 4 j + k; slots past V hold -inf (expf gives 0, and -inf never wins a maximum).
__device__ __forceinline__ int row_slot_index(int tid, int s) { return 4 * (tid + 1024 * (s >> 2)) + (s & 3); }
// N rows side by side: one test of the tail per j for all of them
template <int N>
__device__ __forceinline__ void row_load32(const float* const (&row)[N], int V, int tid, float (&x)[N][32]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i0 = 4 * (tid + 1024 * j);
    if (i0 + 3 < V) {
#pragma unroll
      for (int n = 0; n < N; ++n) {
        const f32x4 v = *(const f32x4*)(row[n] + i0);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[n][4 * j + k] = v[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int n = 0; n < N; ++n) x[n][4 * j + k] = i0 + k < V ? row[n][i0 + k] : -INFINITY;
      }
    }
  }
}
__device__ __forceinline__ void row_load32(const float* row, int V, int tid, float (&x)[32]) {      // N = 1
  const float* const r[1] = {row};
  row_load32(r, V, tid, reinterpret_cast<float (&)[1][32]>(x));
}
__device__ __forceinline__ float row_max32(const float (&x)[32]) {
  float m = -INFINITY;
#pragma unroll
  for (int s = 0; s < 32; ++s) m = fmaxf(m, x[s]);
  return m;
}
__device__ __forceinline__ float row_sumexp32(const float (&x)[32], float m) {
  float z = 0.f;
#pragma unroll
  for (int s = 0; s < 32; ++s) z += expf(x[s] - m);
  return z;
}
// lse of N rows at once (N pairs of barriers saved for N - 1); mx: the rows' maxima
template <int N>
__device__ __forceinline__ void row_lse32(const float (&x)[N][32], float (*sh)[16], float (&mx)[N], float (&lse)[N]) {
#pragma unroll
  for (int n = 0; n < N; ++n) mx[n] = row_max32(x[n]);
  row_block_max(mx, sh);
  float z[N];
#pragma unroll
  for (int n = 0; n < N; ++n) z[n] = row_sumexp32(x[n], mx[n]);
  row_block_sum(z, sh);
#pragma unroll
  for (int n = 0; n < N; ++n) lse[n] = mx[n] + logf(z[n]);
}
__device__ __forceinline__ float row_lse32(const float (&x)[32], float* sh, float& mx) {      // N = 1 by value
  mx = row_block_max(row_max32(x), sh);
  return mx + logf(row_block_sum(row_sumexp32(x, mx), sh));
}
// out[i] = value(slot of i) for every i < V: 16-byte stores, a scalar tail
template <class F>
__device__ __forceinline__ void row_store32(float* out, int V, int tid, F value) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i0 = 4 * (tid + 1024 * j);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = value(4 * j + k);
    if (i0 + 3 < V) {
      *(f32x4*)(out + i0) = o;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (i0 + k < V) out[i0 + k] = o[k];
    }
  }
}

// ---- streamed form: any V, the row read again for every pass -----------------------------------------------------------------------
// TWO element orders, and they must stay two: a thread's partial sum of expf(x - m) runs over different elements in each, so the last
// bits of lse differ, and every caller's outputs are pinned to its own.
//   vec order (vt_logprob_rows, vt_beam_step): f32x4 at 4 i for i = tid, tid + 1024, .. < V4, then the scalars 4 V4 + tid, + 1024, ..
//     V4 = V / 4 where base and stride allow 16-byte loads, else 0 (which leaves the scalar order).
//   scalar order (vt_cfg_rows, vt_dola_rows, the samplers' logprob, the cross entropy): the scalars tid + 1024 j. Their rows carry
//     their own pointers and alignments, and N rows advance together.
template <class F>       // f(value, index) over this thread's elements in the vec order
__device__ __forceinline__ void row_for_each_vec(const float* row, int V, int V4, int tid, F f) {
  for (int i = tid; i < V4; i += 1024) {
    const f32x4 v = *(const f32x4*)(row + 4 * i);
#pragma unroll
    for (int k = 0; k < 4; ++k) f(v[k], 4 * i + k);
  }
  for (int i = 4 * V4 + tid; i < V; i += 1024) f(row[i], i);
}
__device__ __forceinline__ float row_stream_max_vec(const float* row, int V, int V4, int tid) {
  float m = -INFINITY;
  for (int i = tid; i < V4; i += 1024) {
    const f32x4 v = *(const f32x4*)(row + 4 * i);
    m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
  }
  for (int i = 4 * V4 + tid; i < V; i += 1024) m = fmaxf(m, row[i]);
  return m;
}
template <class F>       // each(value, index): what else the caller takes from the same pass
__device__ __forceinline__ float row_stream_sumexp_vec(const float* row, int V, int V4, int tid, float m, F each) {
  float z = 0.f;
  row_for_each_vec(row, V, V4, tid, [&](float v, int i) {
    z += expf(v - m);
    each(v, i);
  });
  return z;
}
__device__ __forceinline__ float row_stream_sumexp_vec(const float* row, int V, int V4, int tid, float m) {
  return row_stream_sumexp_vec(row, V, V4, tid, m, [](float, int) {});
}
// scalar order, N rows side by side
template <int N>
__device__ __forceinline__ void row_lse_stream(const float* const (&row)[N], int V, int tid, float (*sh)[16], float (&mx)[N],
                                               float (&lse)[N]) {
#pragma unroll
  for (int n = 0; n < N; ++n) mx[n] = -INFINITY;
  for (int i = tid; i < V; i += 1024) {
#pragma unroll
    for (int n = 0; n < N; ++n) mx[n] = fmaxf(mx[n], row[n][i]);
  }
  row_block_max(mx, sh);
  float z[N];
#pragma unroll
  for (int n = 0; n < N; ++n) z[n] = 0.f;
  for (int i = tid; i < V; i += 1024) {
#pragma unroll
    for (int n = 0; n < N; ++n) z[n] += expf(row[n][i] - mx[n]);
  }
  row_block_sum(z, sh);
#pragma unroll
  for (int n = 0; n < N; ++n) lse[n] = mx[n] + logf(z[n]);
}
__device__ __forceinline__ float row_lse_stream(const float* row, int V, int tid, float* sh, float& mx) {      // N = 1 by value
  const float* const r[1] = {row};
  float m[1], lse[1];
  row_lse_stream(r, V, tid, (float (*)[16])sh, m, lse);
  mx = m[0];
  return lse[0];
}

// ---- allow masks: V bits in W = ceil(V / 32) words, bit i & 31 of word i >> 5 ------------------------------------------------------
// word w of the starting mask: base's word as it is, or (base NULL) the bits [0, V) -- vt_ban_rows' convention. An output word is
// keep AND base, so the bits >= V of the last word follow base's, and are clear without one.
__device__ __forceinline__ uint32_t row_base_word(const uint32_t* base, int w, int W, int V) {
  if (base != nullptr) return base[w];
  return (w == W - 1 && (V & 31)) ? (1u << (V & 31)) - 1u : 0xffffffffu;
}
// register form: keep(s) for slot s; a word is 8 neighbouring lanes' nibbles, gathered with three shuffles. Every lane of the block
// takes part, so the call is block-uniform.
template <class F>
__device__ __forceinline__ void row_mask32(uint32_t* mask_out, const uint32_t* base, int V, int tid, F keep) {
  const int W = (V + 31) >> 5;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i0 = 4 * (tid + 1024 * j);
    uint32_t nib = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) nib |= ((i0 + k >= V) | keep(4 * j + k)) ? (1u << k) : 0u;
    uint32_t word = nib << (4 * (tid & 7));
    word |= __shfl_xor(word, 1, 64);
    word |= __shfl_xor(word, 2, 64);
    word |= __shfl_xor(word, 4, 64);
    const int w = (tid >> 3) + 128 * j;
    if ((tid & 7) == 0 && w < W) mask_out[w] = word & row_base_word(base, w, W, V);
  }
}
// streamed form: the block's elements b0 + tid, a wave's 64 are two words: one ballot, lanes 0 and 32 store. `keep` is this lane's
// bit (true for an element past V); every lane of the block reaches the call.
__device__ __forceinline__ void row_mask_ballot(uint32_t* mask_out, const uint32_t* base, int V, int b0, int tid, bool keep) {
  const int W = (V + 31) >> 5;
  const int lane = tid & 63, wave = tid >> 6;
  const unsigned long long bal = __ballot(keep);
  const int w = ((b0 + 64 * wave) >> 5) + (lane >> 5);
  if ((lane & 31) == 0 && w < W) mask_out[w] = (uint32_t)(bal >> (lane & 32)) & row_base_word(base, w, W, V);
}
