// vt_logprob.hip -- vt_logprob_rows: what a caller can learn about the distribution behind a logit row without reading
// the row back -- its log-sum-exp, the log-probability and the rank of a given token, and the n_top most likely tokens with their
// log-probabilities. One launch, one 1024-thread block per row, over the RAW fp32 row (no penalty, temperature or mask); the logits are
// only read.
//   lse = m + logf(sum_i expf(x_i - m)), m = max x -- the sampler's logprob expression (vt_llama.hip) and vt_beam_step's, restated here
//     with its small block reductions so that those files keep their code.
//   Order: larger RAW logit first, exact ties by the lower index. Selection compares x, never x - lse, so it is exact. The n_top passes
//     are vt_beam.hip's: pass p takes the best candidate strictly AFTER pass p - 1's pick, so nothing is marked and nothing is written
//     to the row. The rank is a count of the tokens strictly ahead of the target in that order: integer arithmetic.
//   NaN: every comparison with a NaN is false, so a NaN is never taken and never counted as ahead; it reaches the sum, so lse and with
//     it every log-probability of the row is NaN. -inf is an ordinary value.
// No input value is used as an index unchecked: target[r] is compared with [0, V) before row[target[r]] is read.
#include "vt_common.h"
#include "vt_kernels.h"

namespace {

constexpr int kNone = 0x7fffffff;

// The comparisons are written with & and | on bools and the updates as selects: the selection passes are straight-line code (one
// v_cndmask per update) instead of a branch per slot.
// (value, index) pairs ordered by larger value, then lower index; `ok` gates the candidate
__device__ __forceinline__ void lp_take(float& best, int& bi, float v, int i, bool ok = true) {
  const bool t = ok & ((v > best) | ((v == best) & (i < bi)));
  best = t ? v : best;
  bi = t ? i : bi;
}
// is (v, i) strictly after (ls, li) in that order?
__device__ __forceinline__ bool lp_after(float v, int i, float ls, int li) { return (v < ls) | ((v == ls) & (i > li)); }
// is (v, i) strictly ahead of the target (xt, t)? A NaN target stands behind every value that is not a NaN.
__device__ __forceinline__ bool lp_ahead(float v, int i, float xt, int t, bool t_nan) {
  return t_nan ? v == v : ((v > xt) | ((v == xt) & (i < t)));
}

__device__ __forceinline__ void lp_wave_argmax(float& best, int& bi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    lp_take(best, bi, ov, oi);
  }
}
__device__ __forceinline__ float lp_block_sum(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < 16; ++i) t += sh[i];
  return t;
}
__device__ __forceinline__ float lp_block_max(float v, float* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = sh[0];
  for (int i = 1; i < 16; ++i) t = fmaxf(t, sh[i]);
  return t;
}
__device__ __forceinline__ int lp_block_count(int c, int* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  int t = 0;
  for (int i = 0; i < 16; ++i) t += sh[i];
  return t;
}

// kReg (V <= 32 * 1024, base 16-byte aligned, ldl % 4 == 0): the row is read ONCE, 32 values per thread -- thread t owns the floats
// 4 (t + 1024 j) + k -- and the sum, the count and the n_top passes run over registers. Otherwise a thread streams its part of the row
// again (L2) for the sum, the count and whenever it looks for its next candidate; 16-byte loads where stride and base allow them.
template <bool kReg>
__global__ __launch_bounds__(1024) void logprob_rows_kernel(const float* __restrict__ logits, int ldl, int V, const int* __restrict__ target,
                                                            int n_top, float* __restrict__ lse_out, float* __restrict__ target_lp,
                                                            int* __restrict__ target_rank, int* __restrict__ top_ids,
                                                            float* __restrict__ top_lp) {
  __shared__ float sh[16];
  __shared__ int shc[16];
  __shared__ float sv[2][16];
  __shared__ int si[2][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.x;
  const float* row = logits + (size_t)r * ldl;
  const int t = target ? target[r] : -1;
  const bool has_t = (unsigned)t < (unsigned)V;
  if (!has_t && n_top == 0 && !lse_out) {      // (block-uniform) a row that asks for nothing: the row is not read
    if (tid == 0) {
      if (target_lp) target_lp[r] = NAN;
      if (target_rank) target_rank[r] = 0;
    }
    return;
  }
  const bool vec = kReg || ((ldl % 4) == 0 && ((uintptr_t)logits % 16) == 0);
  const int V4 = vec ? (V >> 2) : 0;
  const float xt = has_t ? row[t] : NAN;
  const bool t_nan = xt != xt;
  float x[kReg ? 32 : 1];
  float mx = -INFINITY;
  if constexpr (kReg) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i0 = 4 * (tid + 1024 * j);
      if (i0 + 3 < V) {
        const f32x4 v = *(const f32x4*)(row + i0);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[4 * j + k] = v[k];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[4 * j + k] = i0 + k < V ? row[i0 + k] : -INFINITY;
      }
    }
#pragma unroll
    for (int s = 0; s < 32; ++s) mx = fmaxf(mx, x[s]);
  } else {
    for (int i = tid; i < V4; i += 1024) {
      const f32x4 v = *(const f32x4*)(row + 4 * i);
      mx = fmaxf(fmaxf(mx, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
    }
    for (int i = 4 * V4 + tid; i < V; i += 1024) mx = fmaxf(mx, row[i]);
  }
  mx = lp_block_max(mx, sh);
  float z = 0.f;
  int ahead = 0;
  if constexpr (kReg) {
#pragma unroll
    for (int s = 0; s < 32; ++s) z += expf(x[s] - mx);       // (a slot past V holds -inf: expf gives 0)
    if (has_t) {
#pragma unroll
      for (int s = 0; s < 32; ++s) {
        const int i = 4 * (tid + 1024 * (s >> 2)) + (s & 3);
        ahead += ((i < V) & lp_ahead(x[s], i, xt, t, t_nan)) ? 1 : 0;
      }
    }
  } else {
    for (int i = tid; i < V4; i += 1024) {
      const f32x4 v = *(const f32x4*)(row + 4 * i);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        z += expf(v[k] - mx);
        ahead += (has_t && lp_ahead(v[k], 4 * i + k, xt, t, t_nan)) ? 1 : 0;
      }
    }
    for (int i = 4 * V4 + tid; i < V; i += 1024) {
      const float v = row[i];
      z += expf(v - mx);
      ahead += (has_t && lp_ahead(v, i, xt, t, t_nan)) ? 1 : 0;
    }
  }
  z = lp_block_sum(z, sh);
  const float lse = mx + logf(z);
  if (has_t) ahead = lp_block_count(ahead, shc);       // (block-uniform)
  if (tid == 0) {
    if (lse_out) lse_out[r] = lse;
    if (target_lp) target_lp[r] = has_t ? xt - lse : NAN;
    if (target_rank) target_rank[r] = has_t ? 1 + ahead : 0;
  }
  if (n_top <= 0) return;
  // the best of this thread's own values strictly after (ls, li)
  auto scan = [&](float ls, int li, float& best, int& bi) {
    best = -INFINITY;
    bi = kNone;
    if constexpr (kReg) {
#pragma unroll
      for (int s = 0; s < 32; ++s) {
        const int i = 4 * (tid + 1024 * (s >> 2)) + (s & 3);
        lp_take(best, bi, x[s], i, (i < V) & lp_after(x[s], i, ls, li));
      }
    } else {
      for (int i4 = tid; i4 < V4; i4 += 1024) {
        const f32x4 v = *(const f32x4*)(row + 4 * i4);
#pragma unroll
        for (int k = 0; k < 4; ++k) lp_take(best, bi, v[k], 4 * i4 + k, lp_after(v[k], 4 * i4 + k, ls, li));
      }
      for (int i = 4 * V4 + tid; i < V; i += 1024) {
        const float v = row[i];
        lp_take(best, bi, v, i, lp_after(v, i, ls, li));
      }
    }
  };
  // Every thread keeps the best of its own values that no pass has taken (mb, mi). A pass is a block arg-max over those; only the
  // thread whose value was taken looks for its next one -- everybody else's still lies after the pick in the order.
  float mb;
  int mi;
  scan(INFINITY, -1, mb, mi);       // every value that is not a NaN (+inf and -inf included) is after (+inf, -1)
  for (int p = 0; p < n_top; ++p) {
    float best = mb;
    int bi = mi;
    lp_wave_argmax(best, bi);
    // two LDS buffers in turn: a wave that writes pass p + 2's has passed pass p + 1's barrier, behind which nobody reads pass p's
    if (lane == 0) {
      sv[p & 1][wave] = best;
      si[p & 1][wave] = bi;
    }
    __syncthreads();
    best = sv[p & 1][0];
    bi = si[p & 1][0];
    for (int w = 1; w < 16; ++w) lp_take(best, bi, sv[p & 1][w], si[p & 1][w]);
    if (tid == 0) {
      top_ids[(size_t)r * n_top + p] = bi == kNone ? -1 : bi;
      top_lp[(size_t)r * n_top + p] = bi == kNone ? NAN : best - lse;
    }
    if (bi == mi && bi != kNone) scan(best, bi, mb, mi);     // (kNone: nothing is left, the remaining slots hold (-1, NaN))
  }
}

}  // namespace

int vt_logprob_rows_launch(const float* logits, int rows, int V, int ldl, const int* target, int n_top, float* lse, float* target_lp,
                           int* target_rank, int* top_ids, float* top_lp, hipStream_t s) {
  VT_REQUIRE(logits, "vt_logprob_rows: null pointer (logits is required)");
  VT_REQUIRE(rows > 0 && V > 0 && ldl >= V, "vt_logprob_rows: rows=%d V=%d ldl=%d (rows, V > 0 and ldl >= V)", rows, V, ldl);
  VT_REQUIRE(V <= VT_LOGPROB_MAX_V, "vt_logprob_rows: V=%d (V <= %d)", V, VT_LOGPROB_MAX_V);
  VT_REQUIRE(n_top >= 0 && n_top <= VT_LOGPROB_MAX_TOP, "vt_logprob_rows: n_top=%d (0 <= n_top <= %d)", n_top, VT_LOGPROB_MAX_TOP);
  VT_REQUIRE(n_top == 0 || (top_ids && top_lp), "vt_logprob_rows: null pointer (n_top=%d needs top_ids and top_lp)", n_top);
  VT_REQUIRE(n_top > 0 || lse || target_lp || target_rank, "vt_logprob_rows: null pointer (n_top=0 and no output to write)");
  VT_REQUIRE(((uintptr_t)logits % 4) == 0 && ((uintptr_t)target % 4) == 0 && ((uintptr_t)lse % 4) == 0 && ((uintptr_t)target_lp % 4) == 0 &&
                 ((uintptr_t)target_rank % 4) == 0 && ((uintptr_t)top_ids % 4) == 0 && ((uintptr_t)top_lp % 4) == 0,
             "vt_logprob_rows: every pointer must be 4-byte aligned");
  if (V <= 32 * 1024 && (ldl % 4) == 0 && ((uintptr_t)logits % 16) == 0)
    hipLaunchKernelGGL(logprob_rows_kernel<true>, dim3(rows), dim3(1024), 0, s, logits, ldl, V, target, n_top, lse, target_lp, target_rank,
                       top_ids, top_lp);
  else
    hipLaunchKernelGGL(logprob_rows_kernel<false>, dim3(rows), dim3(1024), 0, s, logits, ldl, V, target, n_top, lse, target_lp,
                       target_rank, top_ids, top_lp);
  VT_LAUNCH_CHECK();
  return VT_OK;
}
