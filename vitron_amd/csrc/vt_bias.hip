// vt_bias.hip -- vt_bias_rows: the additive adjustment of a row's COMING pick, built on the device from (the ids the row
// has GENERATED so far, its logit bias, its presence / frequency penalties), in front of vt_sample_rows_adj. out is fp32 [V][2]:
// out[2t] = pre[t] (added before the repetition penalty), out[2t + 1] = post[t] (added after it).
//
// One 1024-thread block per row. Dynamic LDS: ceil(V / 2) words of 16-bit counters packed two per word (128 KiB at VT_BIAS_ROWS_MAX_V),
// then ceil(V / 32) words of "this id carries a bias" bits (8 KiB there):
//   1. clear both                                                                                                          -- barrier
//   2. threads stride over the history (its last 65535 ids: a counter cannot carry into its neighbour) and add 1 to the id's counter
//      with an LDS atomicAdd; threads stride over the bias ids, set the id's bit with an LDS atomicOr and store the value to out[2 id].
//      Counts are integers and bits are only ever set, so neither depends on the order of the atomics.                     -- barrier
//   3. every t of [0, V): post[t] from its count; a t whose bit is clear gets (0, post) in one 8-byte store, a t whose bit is set gets
//      post alone -- its pre was stored in step 2. No address is written twice (but for a duplicate bias id, where one value lands),
//      and nothing the block wrote to global memory is read back.
// Every index is checked against the length it indexes: the kernel is total over the fields of vt_bias_row.
#include "vt_common.h"
#include "vt_kernels.h"

static_assert(sizeof(vt_bias_row) == 48 && alignof(vt_bias_row) == 8, "vt_bias_row is 48 bytes, 8-byte aligned (ABI)");
static_assert(offsetof(vt_bias_row, history) == 0 && offsetof(vt_bias_row, bias_ids) == 8 && offsetof(vt_bias_row, bias_vals) == 16 &&
                  offsetof(vt_bias_row, out) == 24 && offsetof(vt_bias_row, history_len) == 32 && offsetof(vt_bias_row, n_bias) == 36 &&
                  offsetof(vt_bias_row, presence) == 40 && offsetof(vt_bias_row, frequency) == 44,
              "vt_bias_row offsets are part of the ABI");

namespace {

constexpr int kBiasThreads = 1024;
constexpr int kBiasMaxCount = 65535;                                                           // what a 16-bit counter holds
constexpr int kBiasMaxLds = (VT_BIAS_ROWS_MAX_V / 2 + VT_BIAS_ROWS_MAX_V / 32) * 4;            // 136 KiB of the CU's 160

// -(frequency * c + presence), the product and the sum rounded separately (hipcc would contract them into one fma otherwise)
__device__ __forceinline__ float count_penalty(float frequency, float c, float presence) {
#pragma clang fp contract(off)
  const float prod = frequency * c;
  return -(prod + presence);
}

__global__ __launch_bounds__(kBiasThreads) void bias_rows_kernel(const vt_bias_row* __restrict__ rows, int V) {
  extern __shared__ __attribute__((aligned(16))) uint32_t bias_lds[];
  const vt_bias_row row = rows[blockIdx.x];
  if (row.out == nullptr) return;        // block-uniform, before any barrier: the row is skipped entirely
  const int tid = threadIdx.x;
  const int CW = (V + 1) >> 1, BW = (V + 31) >> 5;
  uint32_t* __restrict__ cnt = bias_lds;             // counter of id t: bits [16 (t & 1), 16 (t & 1) + 16) of word t >> 1
  uint32_t* __restrict__ has = bias_lds + CW;        // bit (t & 31) of word t >> 5: t carries a bias
  float* __restrict__ out = row.out;

  // 1.
  for (int w = tid; w < CW + BW; w += kBiasThreads) bias_lds[w] = 0u;
  __syncthreads();

  // 2.
  const int* __restrict__ h = row.history;
  int n = (h != nullptr && row.history_len > 0) ? row.history_len : 0;
  if (n > kBiasMaxCount) {
    h += n - kBiasMaxCount;
    n = kBiasMaxCount;
  }
  for (int i = tid; i < n; i += kBiasThreads) {
    const int id = h[i];
    if ((unsigned)id < (unsigned)V) atomicAdd(&cnt[id >> 1], 1u << (16 * (id & 1)));
  }
  const int nb = (row.bias_ids != nullptr && row.bias_vals != nullptr && row.n_bias > 0) ? row.n_bias : 0;
  for (int j = tid; j < nb; j += kBiasThreads) {
    const int id = row.bias_ids[j];
    if ((unsigned)id < (unsigned)V) {
      atomicOr(&has[id >> 5], 1u << (id & 31));
      out[2 * (size_t)id] = row.bias_vals[j];
    }
  }
  __syncthreads();

  // 3. the 2 V floats of out, nothing behind them
  const bool wide = ((uintptr_t)out % 8) == 0;     // block-uniform
  for (int t = tid; t < V; t += kBiasThreads) {
    const uint32_t c = (cnt[t >> 1] >> (16 * (t & 1))) & 0xffffu;
    const float post = c == 0u ? 0.0f : count_penalty(row.frequency, (float)c, row.presence);
    const bool biased = (has[t >> 5] >> (t & 31)) & 1u;
    if (biased) {
      out[2 * (size_t)t + 1] = post;
    } else if (wide) {
      *(float2*)(out + 2 * (size_t)t) = make_float2(0.0f, post);
    } else {
      out[2 * (size_t)t] = 0.0f;
      out[2 * (size_t)t + 1] = post;
    }
  }
}

}  // namespace

int vt_bias_rows_launch(const vt_bias_row* rows, int n_rows, int V, hipStream_t s) {
  VT_REQUIRE(V > 0 && V <= VT_BIAS_ROWS_MAX_V, "vt_bias_rows: V=%d (0 < V <= %d)", V, VT_BIAS_ROWS_MAX_V);
  VT_REQUIRE(n_rows >= 0, "vt_bias_rows: n_rows=%d", n_rows);
  if (n_rows == 0) return VT_OK;
  VT_REQUIRE(rows != nullptr, "vt_bias_rows: rows is NULL with n_rows=%d", n_rows);
  VT_REQUIRE(((uintptr_t)rows % 8) == 0, "vt_bias_rows: rows must be 8-byte aligned");
  const int smem = (((V + 1) >> 1) + ((V + 31) >> 5)) * 4;
  VT_LDS_ATTR_ONCE(bias_rows_kernel, kBiasMaxLds);
  hipLaunchKernelGGL(bias_rows_kernel, dim3(n_rows), dim3(kBiasThreads), smem, s, rows, V);
  VT_LAUNCH_CHECK();
  return VT_OK;
}
