// vt_ban.hip -- vt_ban_rows: the allow mask of a row's COMING pick, built on the device from (a base mask, the ids the
// row has seen so far, its rules), in front of the unchanged vt_sample_rows_allow. The two rules are the history-dependent ones of
// transformers: NoRepeatNGramLogitsProcessor (no_repeat_ngram_size) and NoBadWordsLogitsProcessor with multi-token entries.
//
// One 1024-thread block per row. The mask lives in LDS (ceil(V / 32) words, 32 KiB at VT_SAMPLE_ROWS_MAX_V):
//   1. copy `base` into it (or set the bits [0, V))                                         -- barrier
//   2. threads stride over the window positions of the n-gram rule and over the sequences; every hit clears one bit with an LDS
//      atomicAnd. Bits are only ever cleared, so the result does not depend on the order: the mask is deterministic.       -- barrier
//   3. write the words to `out`, 16 bytes per thread where `out` is 16-byte aligned.
// Every index is checked against the length it indexes: the kernel is total over the fields of vt_ban_row.
#include "vt_common.h"
#include "vt_kernels.h"

static_assert(sizeof(vt_ban_row) == 48 && alignof(vt_ban_row) == 8, "vt_ban_row is 48 bytes, 8-byte aligned (ABI)");
static_assert(offsetof(vt_ban_row, history) == 0 && offsetof(vt_ban_row, base) == 8 && offsetof(vt_ban_row, out) == 16 &&
                  offsetof(vt_ban_row, seqs) == 24 && offsetof(vt_ban_row, history_len) == 32 && offsetof(vt_ban_row, ngram) == 36 &&
                  offsetof(vt_ban_row, n_seqs) == 40 && offsetof(vt_ban_row, seqs_len) == 44,
              "vt_ban_row offsets are part of the ABI");

namespace {

constexpr int kBanThreads = 1024;
constexpr int kBanMaxWords = VT_SAMPLE_ROWS_MAX_V / 32;

__device__ __forceinline__ void ban_clear(uint32_t* mask, int id, int V) {
  if ((unsigned)id < (unsigned)V) atomicAnd(&mask[id >> 5], ~(1u << (id & 31)));
}

__global__ __launch_bounds__(kBanThreads) void ban_rows_kernel(const vt_ban_row* __restrict__ rows, int V) {
  __shared__ __attribute__((aligned(16))) uint32_t mask[kBanMaxWords];
  const vt_ban_row row = rows[blockIdx.x];
  if (row.out == nullptr) return;        // block-uniform, before any barrier: the row is skipped entirely
  const int tid = threadIdx.x;
  const int W = (V + 31) >> 5;

  // 1. the starting mask
  if (row.base != nullptr) {
    const uint32_t* __restrict__ base = row.base;
    const int W4 = ((uintptr_t)base % 16) == 0 ? (W >> 2) : 0;
    for (int c = tid; c < W4; c += kBanThreads) *(u32x4*)(mask + 4 * c) = *(const u32x4*)(base + 4 * c);
    for (int w = 4 * W4 + tid; w < W; w += kBanThreads) mask[w] = base[w];
  } else {
    const uint32_t last = (V & 31) ? (1u << (V & 31)) - 1u : 0xffffffffu;     // the bits >= V of the last word stay clear
    for (int w = tid; w < W; w += kBanThreads) mask[w] = w == W - 1 ? last : 0xffffffffu;
  }
  __syncthreads();

  const int* __restrict__ h = row.history;
  const int n = (h != nullptr && row.history_len > 0) ? row.history_len : 0;

  // 2a. the n-gram rule: window i = h[i .. i + g - 2] against the last g - 1 ids; a match bans the id that followed the window
  const int g = row.ngram;
  if (g >= 1 && n >= g - 1) {
    const int tail = n - g + 1;          // start of the last g - 1 ids; also the number of windows that have a follower
    for (int i = tid; i < tail; i += kBanThreads) {
      bool same = true;
      for (int k = 0; k < g - 1 && same; ++k) same = h[i + k] == h[tail + k];
      if (same) ban_clear(mask, h[i + g - 1], V);
    }
  }

  // 2b. the sequences {L, id_0 .. id_{L-1}}: every thread walks the headers (the same addresses in every lane) and handles the
  // sequences j == tid (mod 1024). A header that is <= 0 or runs past seqs_len ends the walk.
  const int* __restrict__ sq = row.seqs;
  if (sq != nullptr && row.n_seqs > 0 && row.seqs_len > 0) {
    const int end = row.seqs_len;
    int pos = 0;
    for (int j = 0; j < row.n_seqs && pos < end; ++j) {
      const int L = sq[pos];
      if (L <= 0 || L > end - pos - 1) break;
      if ((j & (kBanThreads - 1)) == tid) {
        const int* s = sq + pos + 1;
        bool hit = n >= L - 1;
        for (int k = 0; k < L - 1 && hit; ++k) hit = h[n - (L - 1) + k] == s[k];
        if (hit) ban_clear(mask, s[L - 1], V);
      }
      pos += 1 + L;
    }
  }
  __syncthreads();

  // 3. the words [0, W) of out, nothing behind them
  uint32_t* __restrict__ out = row.out;
  const int W4 = ((uintptr_t)out % 16) == 0 ? (W >> 2) : 0;
  for (int c = tid; c < W4; c += kBanThreads) *(u32x4*)(out + 4 * c) = *(const u32x4*)(mask + 4 * c);
  for (int w = 4 * W4 + tid; w < W; w += kBanThreads) out[w] = mask[w];
}

}  // namespace

int vt_ban_rows_launch(const vt_ban_row* rows, int n_rows, int V, hipStream_t s) {
  VT_REQUIRE(V > 0 && V <= VT_SAMPLE_ROWS_MAX_V, "vt_ban_rows: V=%d (0 < V <= %d)", V, VT_SAMPLE_ROWS_MAX_V);
  VT_REQUIRE(n_rows >= 0, "vt_ban_rows: n_rows=%d", n_rows);
  if (n_rows == 0) return VT_OK;
  VT_REQUIRE(rows != nullptr, "vt_ban_rows: rows is NULL with n_rows=%d", n_rows);
  VT_REQUIRE(((uintptr_t)rows % 8) == 0, "vt_ban_rows: rows must be 8-byte aligned");
  hipLaunchKernelGGL(ban_rows_kernel, dim3(n_rows), dim3(kBanThreads), 0, s, rows, V);
  VT_LAUNCH_CHECK();
  return VT_OK;
}
