// vt_logprob.hip -- vt_logprob_rows: what a caller can learn about the distribution behind a logit row without reading
// the row back -- its log-sum-exp, the log-probability and the rank of a given token, and the n_top most likely tokens with their
// log-probabilities. One launch, one 1024-thread block per row, over the RAW fp32 row (no penalty, temperature or mask); the logits are
// only read.
//   lse = m + logf(sum_i expf(x_i - m)), m = max x -- vt_rows.h's expression and block reductions, which the sampler's logprob and
//     vt_beam_step share; the streamed form reads in that header's vec order.
//   Order: vt_rows.h's -- larger RAW logit first, exact ties by the lower index. Selection compares x, never x - lse, so it is exact.
//     The n_top passes are built like vt_beam.hip's: pass p takes the best candidate strictly AFTER pass p - 1's pick, so nothing is
//     marked and nothing is written to the row. The rank is a count of the tokens strictly ahead of the target in that order: integer
//     arithmetic.
//   NaN: every comparison with a NaN is false, so a NaN is never taken and never counted as ahead; it reaches the sum, so lse and with
//     it every log-probability of the row is NaN. -inf is an ordinary value.
// No input value is used as an index unchecked: target[r] is compared with [0, V) before row[target[r]] is read.
#include "vt_common.h"
#include "vt_kernels.h"
#include "vt_rows.h"

namespace {

constexpr RowTake row_take{};       // vt_rows.h's (value, index) order in its select form: the selection passes are straight-line code

// is (v, i) strictly ahead of the target (xt, t)? A NaN target stands behind every value that is not a NaN.
__device__ __forceinline__ bool lp_ahead(float v, int i, float xt, int t, bool t_nan) {
  return t_nan ? v == v : ((v > xt) | ((v == xt) & (i < t)));
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
  float mx, z;
  int ahead = 0;
  if constexpr (kReg) {
    row_load32(row, V, tid, x);
    mx = row_block_max(row_max32(x), sh);
    z = row_sumexp32(x, mx);
    if (has_t) {
#pragma unroll
      for (int s = 0; s < 32; ++s) {
        const int i = row_slot_index(tid, s);
        ahead += ((i < V) & lp_ahead(x[s], i, xt, t, t_nan)) ? 1 : 0;
      }
    }
  } else {
    mx = row_block_max(row_stream_max_vec(row, V, V4, tid), sh);
    z = row_stream_sumexp_vec(row, V, V4, tid, mx, [&](float v, int i) { ahead += (has_t && lp_ahead(v, i, xt, t, t_nan)) ? 1 : 0; });
  }
  z = row_block_sum(z, sh);
  const float lse = mx + logf(z);
  if (has_t) ahead = row_block_count(ahead, shc);      // (block-uniform)
  if (tid == 0) {
    if (lse_out) lse_out[r] = lse;
    if (target_lp) target_lp[r] = has_t ? xt - lse : NAN;
    if (target_rank) target_rank[r] = has_t ? 1 + ahead : 0;
  }
  if (n_top <= 0) return;
  // the best of this thread's own values strictly after (ls, li)
  auto scan = [&](float ls, int li, float& best, int& bi) {
    best = -INFINITY;
    bi = kRowNone;
    if constexpr (kReg) {
#pragma unroll
      for (int s = 0; s < 32; ++s) {
        const int i = row_slot_index(tid, s);
        row_take(best, bi, x[s], i, (i < V) & row_after(x[s], i, ls, li));
      }
    } else {
      row_for_each_vec(row, V, V4, tid, [&](float v, int i) { row_take(best, bi, v, i, row_after(v, i, ls, li)); });
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
    row_wave_argmax(best, bi, row_take);
    // two LDS buffers in turn: a wave that writes pass p + 2's has passed pass p + 1's barrier, behind which nobody reads pass p's
    if (lane == 0) {
      sv[p & 1][wave] = best;
      si[p & 1][wave] = bi;
    }
    __syncthreads();
    best = sv[p & 1][0];
    bi = si[p & 1][0];
    for (int w = 1; w < 16; ++w) row_take(best, bi, sv[p & 1][w], si[p & 1][w]);
    if (tid == 0) {
      top_ids[(size_t)r * n_top + p] = bi == kRowNone ? -1 : bi;
      top_lp[(size_t)r * n_top + p] = bi == kRowNone ? NAN : best - lse;
    }
    if (bi == mi && bi != kRowNone) scan(best, bi, mb, mi);     // (kRowNone: nothing is left, the remaining slots hold (-1, NaN))
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
