// vt_beam.hip -- the two device pieces of beam search: vt_beam_step turns the logit rows of a beam group into the
// group's best continuations without a read-back of the rows, vt_kv_copy_pages copies KV pages so that a beam that continues another
// beam's hypothesis gets that beam's generated tail.
//
// vt_beam_step, two launches:
//   stage 1 (one 1024-thread block per row): the row's log-sum-exp -- vt_rows.h's expression and reductions, the streamed form in its
//     vec order: m = max, z = sum expf(x - m), lse = m + logf(z) -- then the candidate score s = (x - lse) + beam_score of every token
//     and the row's own n_out best by repeated block arg-max. No candidate outside a row's own n_out best can be among the group's
//     n_out best, so this loses nothing.
//   stage 2 (one wave per group): merges the beams_in * n_out survivors.
// Order everywhere: larger score first, exact ties by the lower flat index b * V + t. A pass never marks what it took: pass p takes
// the best candidate strictly AFTER pass p - 1's pick in that order, so the selection needs no mask and the logits are only read.
// A NaN score is never taken; a row needs a finite maximum.
#include "vt_common.h"
#include "vt_kernels.h"
#include "vt_rows.h"

namespace {

// vt_rows.h's (value, index) order in its branch form (see there why), and the after test spelled to match (with row_after's & and |
// beam_merge_kernel allocates 32 VGPRs instead of 33)
constexpr RowTakeIf beam_take{};
__device__ __forceinline__ bool beam_after(float v, int i, float ls, int li) { return v < ls || (v == ls && i > li); }

// Stage 1. kReg (V <= 32 * 1024): the row is read ONCE, 32 values per thread, and the n_out arg-max passes run over registers;
// otherwise a thread streams its part of the row again (L2) whenever it looks for its next candidate. vec: 16-byte loads (row
// stride a multiple of 4 floats, base 16-byte aligned); thread t then owns the floats 4 (t + 1024 j) + k, else t + 1024 (4 j + k)
// -- both cover [0, 32768) once.
template <bool kReg>
__global__ __launch_bounds__(1024) void beam_rows_kernel(const float* __restrict__ logits, int ldl, int V,
                                                         const float* __restrict__ beam_scores, int n_out,
                                                         float* __restrict__ cand_s, int* __restrict__ cand_t) {
  __shared__ float sh[16];
  __shared__ float sv[2][16];
  __shared__ int si[2][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.x;
  const float* row = logits + (size_t)r * ldl;
  const bool vec = (ldl % 4) == 0 && ((uintptr_t)logits % 16) == 0;
  const int V4 = vec ? (V >> 2) : 0;
  const float bs = beam_scores[r];
  float x[kReg ? 32 : 1];
  auto slot_index = [&](int j, int k) { return vec ? 4 * (tid + 1024 * j) + k : tid + 1024 * (4 * j + k); };
  float mx, z;
  if constexpr (kReg) {
    // vt_rows.h's row_load32 with beam's second slot layout, for rows that 16-byte loads cannot reach, folded into its tail branch
    // (two loaders behind one test of `vec` are 24 more loads and 25 more branches in the kernel, and 0.04 us at 4 rows)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (vec && 4 * (tid + 1024 * j) + 3 < V) {
        const f32x4 v = *(const f32x4*)(row + 4 * (tid + 1024 * j));
#pragma unroll
        for (int k = 0; k < 4; ++k) x[4 * j + k] = v[k];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int i = slot_index(j, k);
          x[4 * j + k] = i < V ? row[i] : -INFINITY;
        }
      }
    }
    mx = row_block_max(row_max32(x), sh);
    z = row_sumexp32(x, mx);
  } else {
    mx = row_block_max(row_stream_max_vec(row, V, V4, tid), sh);
    z = row_stream_sumexp_vec(row, V, V4, tid, mx);
  }
  z = row_block_sum(z, sh);
  const float lse = mx + logf(z);
  if constexpr (kReg) {
#pragma unroll
    for (int s = 0; s < 32; ++s) x[s] = (x[s] - lse) + bs;
  }
  // the best of this thread's own candidates strictly after (ls, li)
  auto scan = [&](float ls, int li, float& best, int& bi) {
    best = -INFINITY;
    bi = kRowNone;
    if constexpr (kReg) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int i = slot_index(j, k);
          const float s = x[4 * j + k];
          if (i < V && beam_after(s, i, ls, li)) beam_take(best, bi, s, i);
        }
    } else {
      row_for_each_vec(row, V, V4, tid, [&](float v, int i) {
        const float s = (v - lse) + bs;
        if (beam_after(s, i, ls, li)) beam_take(best, bi, s, i);
      });
    }
  };
  // Every thread keeps the best of its own candidates that no pass has taken (mb, mi). A pass is a block arg-max over those; only the
  // thread whose candidate was taken looks for its next one -- everybody else's still lies after the pick in the order.
  float mb;
  int mi;
  scan(INFINITY, -1, mb, mi);       // everything finite (and -inf) is after (+inf, -1)
  for (int p = 0; p < n_out; ++p) {
    float best = mb;
    int bi = mi;
    row_wave_argmax(best, bi, beam_take);
    // two LDS buffers in turn: a wave that writes pass p + 2's has passed pass p + 1's barrier, behind which nobody reads pass p's
    if (lane == 0) {
      sv[p & 1][wave] = best;
      si[p & 1][wave] = bi;
    }
    __syncthreads();
    best = sv[p & 1][0];
    bi = si[p & 1][0];
    for (int w = 1; w < 16; ++w) beam_take(best, bi, sv[p & 1][w], si[p & 1][w]);
    if (tid == 0) {
      cand_s[(size_t)r * n_out + p] = best;
      cand_t[(size_t)r * n_out + p] = bi == kRowNone ? -1 : bi;
    }
    if (bi == mi && bi != kRowNone) scan(best, bi, mb, mi);     // (kRowNone: nothing is left, the remaining passes write (-inf, -1))
  }
}

// Stage 2: one wave per group over its beams_in * n_out <= 512 survivors, lane l holds the candidates l + 64 j.
__global__ __launch_bounds__(64) void beam_merge_kernel(const float* __restrict__ cand_s, const int* __restrict__ cand_t, int V,
                                                        int beams_in, int n_out, float* __restrict__ out_scores,
                                                        int* __restrict__ out_tokens, int* __restrict__ out_beams) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const int C = beams_in * n_out;
  float s[8];
  int f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = lane + 64 * j;
    s[j] = -INFINITY;
    f[j] = kRowNone;
    if (c < C) {
      const int t = cand_t[(size_t)g * C + c];
      if (t >= 0) {
        s[j] = cand_s[(size_t)g * C + c];
        f[j] = (c / n_out) * V + t;
      }
    }
  }
  float ls = INFINITY;
  int li = -1;
  for (int p = 0; p < n_out; ++p) {
    float best = -INFINITY;
    int bi = kRowNone;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (f[j] != kRowNone && beam_after(s[j], f[j], ls, li)) beam_take(best, bi, s[j], f[j]);
    row_wave_argmax(best, bi, beam_take);
    if (lane == 0) {
      out_scores[(size_t)g * n_out + p] = best;
      out_tokens[(size_t)g * n_out + p] = bi == kRowNone ? -1 : bi % V;
      out_beams[(size_t)g * n_out + p] = bi == kRowNone ? -1 : bi / V;
    }
    ls = best;
    li = bi;
  }
}

// grid (pair, layer, K | V^T): page src_pages[i] onto page dst_pages[i] of that layer and pool, 16 bytes per thread and trip.
// A pair with an id outside [0, num_pages) is skipped (block-uniform).
__global__ __launch_bounds__(256) void kv_copy_pages_kernel(uint8_t* __restrict__ k, uint8_t* __restrict__ vt, int num_pages,
                                                            size_t page_bytes, const int* __restrict__ src_pages,
                                                            const int* __restrict__ dst_pages) {
  const int src = src_pages[blockIdx.x], dst = dst_pages[blockIdx.x];
  if ((unsigned)src >= (unsigned)num_pages || (unsigned)dst >= (unsigned)num_pages || src == dst) return;
  uint8_t* pool = blockIdx.z ? vt : k;
  const size_t layer0 = (size_t)blockIdx.y * num_pages;
  const u32x4* s = (const u32x4*)(pool + (layer0 + src) * page_bytes);
  u32x4* d = (u32x4*)(pool + (layer0 + dst) * page_bytes);
  const size_t chunks = page_bytes >> 4;
  for (size_t c = threadIdx.x; c < chunks; c += 256) d[c] = s[c];
}

}  // namespace

size_t vt_beam_step_scratch_bytes_impl(int groups, int beams_in, int n_out) {
  if (groups <= 0 || beams_in <= 0 || n_out <= 0) return 0;
  return (size_t)groups * beams_in * n_out * (sizeof(float) + sizeof(int));
}

int vt_beam_step_launch(const float* logits, int ldl, int V, int groups, int beams_in, const float* beam_scores, int n_out,
                        float* out_scores, int* out_tokens, int* out_beams, void* scratch, size_t scratch_bytes, hipStream_t s) {
  VT_REQUIRE(logits && beam_scores && out_scores && out_tokens && out_beams && scratch, "vt_beam_step: null pointer");
  VT_REQUIRE(groups > 0 && V > 0 && ldl >= V, "vt_beam_step: groups=%d V=%d ldl=%d (groups, V > 0 and ldl >= V)", groups, V, ldl);
  VT_REQUIRE(beams_in >= 1 && beams_in <= 16, "vt_beam_step: beams_in=%d (1 <= beams_in <= 16)", beams_in);
  VT_REQUIRE(n_out >= 1 && n_out <= 32, "vt_beam_step: n_out=%d (1 <= n_out <= 32)", n_out);
  VT_REQUIRE(n_out <= V, "vt_beam_step: n_out=%d exceeds V=%d", n_out, V);
  VT_REQUIRE(V <= VT_SAMPLE_ROWS_MAX_V, "vt_beam_step: V=%d (V <= %d)", V, VT_SAMPLE_ROWS_MAX_V);
  VT_REQUIRE(((uintptr_t)scratch % 4) == 0, "vt_beam_step: scratch must be 4-byte aligned");
  const size_t need = vt_beam_step_scratch_bytes_impl(groups, beams_in, n_out);
  if (scratch_bytes < need) {
    vt_set_error("vt_beam_step: scratch of %zu bytes, %zu needed", scratch_bytes, need);
    return VT_ERR_WORKSPACE;
  }
  const int rows = groups * beams_in;
  float* cand_s = (float*)scratch;
  int* cand_t = (int*)(cand_s + (size_t)rows * n_out);
  if (V <= 32 * 1024)
    hipLaunchKernelGGL(beam_rows_kernel<true>, dim3(rows), dim3(1024), 0, s, logits, ldl, V, beam_scores, n_out, cand_s, cand_t);
  else
    hipLaunchKernelGGL(beam_rows_kernel<false>, dim3(rows), dim3(1024), 0, s, logits, ldl, V, beam_scores, n_out, cand_s, cand_t);
  VT_LAUNCH_CHECK();
  hipLaunchKernelGGL(beam_merge_kernel, dim3(groups), dim3(64), 0, s, cand_s, cand_t, V, beams_in, n_out, out_scores, out_tokens,
                     out_beams);
  VT_LAUNCH_CHECK();
  return VT_OK;
}

int vt_kv_copy_pages_launch(void* k, void* vt, int num_layers, int num_pages, size_t page_bytes, const int* src_pages,
                            const int* dst_pages, int n, hipStream_t s) {
  VT_REQUIRE(n >= 0, "vt_kv_copy_pages: n=%d", n);
  if (n == 0) return VT_OK;
  VT_REQUIRE(k && vt && src_pages && dst_pages, "vt_kv_copy_pages: null pointer");
  VT_REQUIRE(num_layers > 0 && num_layers <= 65535 && num_pages > 0, "vt_kv_copy_pages: num_layers=%d num_pages=%d", num_layers,
             num_pages);
  VT_REQUIRE(page_bytes > 0 && page_bytes % 16 == 0, "vt_kv_copy_pages: page_bytes=%zu must be a positive multiple of 16", page_bytes);
  VT_REQUIRE(((uintptr_t)k % 16) == 0 && ((uintptr_t)vt % 16) == 0, "vt_kv_copy_pages: the pools must be 16-byte aligned");
  hipLaunchKernelGGL(kv_copy_pages_kernel, dim3(n, num_layers, 2), dim3(256), 0, s, (uint8_t*)k, (uint8_t*)vt, num_pages, page_bytes,
                     src_pages, dst_pages);
  VT_LAUNCH_CHECK();
  return VT_OK;
}
