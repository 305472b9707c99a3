// vt_fsm.hip -- vt_fsm_rows: guided decoding by a finite automaton over token ids. A row carries {state, consumed} in a
// two-int cell; the ids it has generated since `consumed` move the state, the state decides the allow mask of the row's COMING pick,
// built in front of the unchanged vt_sample_rows_allow (and, when an n-gram ban is on too, in front of vt_ban_rows as its base).
//
// One 1024-thread block per row. The mask lives in LDS (ceil(V / 32) words, 32 KiB at VT_SAMPLE_ROWS_MAX_V):
//   0. thread 0 advances the state over gen[consumed .. gen_len) -- one binary search per id, normally one id -- and writes the cell back
//                                                                                                                        -- barrier
//   1. a dead state: zeros. Else, under a default edge, ones over [0, V); without one, zeros                          -- barrier
//   2. the EOS ids (never covered by the default edge): set when the state accepts, cleared when it does not           -- barrier
//   3. threads stride over the state's listed edges: next inside [0, n_states) sets the bit, anything else clears it (a listed edge
//      overrides what 1 and 2 left for its id). The ids of a state are unique, so every bit is touched by one atomic per phase: the
//      result does not depend on their order.                                                                          -- barrier
//   4. out = mask AND base, 16 bytes per thread where out (and base) are 16-byte aligned.
// Every index is checked against the length it indexes: the kernel is total over the fields of vt_fsm_row.
#include "vt_common.h"
#include "vt_kernels.h"

static_assert(sizeof(vt_fsm_row) == 96 && alignof(vt_fsm_row) == 8, "vt_fsm_row is 96 bytes, 8-byte aligned (ABI)");
static_assert(offsetof(vt_fsm_row, gen) == 0 && offsetof(vt_fsm_row, cell) == 8 && offsetof(vt_fsm_row, base) == 16 &&
                  offsetof(vt_fsm_row, out) == 24 && offsetof(vt_fsm_row, offsets) == 32 && offsetof(vt_fsm_row, edge_tok) == 40 &&
                  offsetof(vt_fsm_row, edge_next) == 48 && offsetof(vt_fsm_row, state_info) == 56 && offsetof(vt_fsm_row, gen_len) == 64 &&
                  offsetof(vt_fsm_row, n_states) == 68 && offsetof(vt_fsm_row, n_edges) == 72 && offsetof(vt_fsm_row, n_eos) == 76 &&
                  offsetof(vt_fsm_row, eos) == 80,
              "vt_fsm_row offsets are part of the ABI");

namespace {

constexpr int kFsmThreads = 1024;
constexpr int kFsmMaxWords = VT_SAMPLE_ROWS_MAX_V / 32;

// the automaton of one row with its lengths made safe: n_states / n_edges are 0 where a table is missing
struct FsmTables {
  const int* __restrict__ offsets;
  const int* __restrict__ edge_tok;
  const int* __restrict__ edge_next;
  const int* __restrict__ info;
  int n_states, n_edges, n_eos;
  int e0, e1, e2, e3;
};

__device__ __forceinline__ FsmTables fsm_tables(const vt_fsm_row& row) {
  FsmTables a;
  a.offsets = row.offsets;
  a.edge_tok = row.edge_tok;
  a.edge_next = row.edge_next;
  a.info = row.state_info;
  a.n_states = (row.offsets != nullptr && row.state_info != nullptr && row.n_states > 0) ? row.n_states : 0;
  a.n_edges = (row.edge_tok != nullptr && row.edge_next != nullptr && row.n_edges > 0) ? row.n_edges : 0;
  a.n_eos = row.n_eos < 0 ? 0 : (row.n_eos > 4 ? 4 : row.n_eos);
  a.e0 = row.eos[0];
  a.e1 = row.eos[1];
  a.e2 = row.eos[2];
  a.e3 = row.eos[3];
  return a;
}

__device__ __forceinline__ int fsm_clamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

__device__ __forceinline__ bool fsm_is_eos(const FsmTables& a, int t) {
  return (a.n_eos > 0 && t == a.e0) || (a.n_eos > 1 && t == a.e1) || (a.n_eos > 2 && t == a.e2) || (a.n_eos > 3 && t == a.e3);
}

// the edge range of a state inside [0, n_states), clamped into [0, n_edges]
__device__ __forceinline__ void fsm_range(const FsmTables& a, int s, int& lo, int& hi) {
  lo = fsm_clamp(a.offsets[s], 0, a.n_edges);
  hi = fsm_clamp(a.offsets[s + 1], lo, a.n_edges);
}

__device__ __forceinline__ int fsm_step(const FsmTables& a, int s, int t) {
  if ((unsigned)s >= (unsigned)a.n_states) return -1;
  int lo, hi;
  fsm_range(a, s, lo, hi);
  int l = lo, r = hi;                    // the first edge whose id is >= t
  while (l < r) {
    const int m = l + ((r - l) >> 1);
    if (a.edge_tok[m] < t) l = m + 1; else r = m;
  }
  int nx;
  if (l < hi && a.edge_tok[l] == t) nx = a.edge_next[l];
  else if (fsm_is_eos(a, t)) nx = a.info[2 * s + 1] != 0 ? s : -1;
  else nx = a.info[2 * s];
  return (unsigned)nx < (unsigned)a.n_states ? nx : -1;
}

__global__ __launch_bounds__(kFsmThreads) void fsm_rows_kernel(const vt_fsm_row* __restrict__ rows, int V) {
  __shared__ __attribute__((aligned(16))) uint32_t mask[kFsmMaxWords];
  __shared__ int s_state;
  const vt_fsm_row row = rows[blockIdx.x];
  if (row.out == nullptr || row.cell == nullptr) return;      // block-uniform, before any barrier: the row is skipped entirely
  const int tid = threadIdx.x;
  const int W = (V + 31) >> 5;
  const FsmTables a = fsm_tables(row);

  // 0. the advance: one thread
  if (tid == 0) {
    int state = row.cell[0];
    const int consumed = row.cell[1] > 0 ? row.cell[1] : 0;
    const int n = row.gen != nullptr ? row.gen_len : 0;
    for (int i = consumed; i < n; ++i) state = fsm_step(a, state, row.gen[i]);
    row.cell[0] = state;
    row.cell[1] = consumed > n ? consumed : n;
    s_state = state;
  }
  __syncthreads();
  const int s = s_state;
  const bool live = (unsigned)s < (unsigned)a.n_states;
  int lo = 0, hi = 0, dflt = -1, accept = 0;
  if (live) {
    fsm_range(a, s, lo, hi);
    dflt = a.info[2 * s];
    accept = a.info[2 * s + 1];
  }
  const bool ones = live && (unsigned)dflt < (unsigned)a.n_states;

  // 1. the starting mask
  {
    const uint32_t full = ones ? 0xffffffffu : 0u;
    const uint32_t last = (V & 31) ? (full & ((1u << (V & 31)) - 1u)) : full;       // the bits >= V of the last word stay clear
    for (int w = tid; w < W; w += kFsmThreads) mask[w] = w == W - 1 ? last : full;
  }
  __syncthreads();

  // 2. the EOS ids
  if (live && tid < a.n_eos) {
    const int e = tid == 0 ? a.e0 : (tid == 1 ? a.e1 : (tid == 2 ? a.e2 : a.e3));
    if ((unsigned)e < (unsigned)V) {
      if (accept != 0) atomicOr(&mask[e >> 5], 1u << (e & 31));
      else atomicAnd(&mask[e >> 5], ~(1u << (e & 31)));
    }
  }
  __syncthreads();

  // 3. the listed edges
  for (int j = lo + tid; j < hi; j += kFsmThreads) {
    const int t = a.edge_tok[j];
    if ((unsigned)t < (unsigned)V) {
      if ((unsigned)a.edge_next[j] < (unsigned)a.n_states) atomicOr(&mask[t >> 5], 1u << (t & 31));
      else atomicAnd(&mask[t >> 5], ~(1u << (t & 31)));
    }
  }
  __syncthreads();

  // 4. the words [0, W) of out, nothing behind them
  uint32_t* __restrict__ out = row.out;
  const uint32_t* __restrict__ base = row.base;
  const bool vec = ((uintptr_t)out % 16) == 0 && ((uintptr_t)base % 16) == 0;        // (a NULL base is aligned)
  const int W4 = vec ? (W >> 2) : 0;
  if (base != nullptr) {
    for (int c = tid; c < W4; c += kFsmThreads) *(u32x4*)(out + 4 * c) = *(const u32x4*)(mask + 4 * c) & *(const u32x4*)(base + 4 * c);
    for (int w = 4 * W4 + tid; w < W; w += kFsmThreads) out[w] = mask[w] & base[w];
  } else {
    for (int c = tid; c < W4; c += kFsmThreads) *(u32x4*)(out + 4 * c) = *(const u32x4*)(mask + 4 * c);
    for (int w = 4 * W4 + tid; w < W; w += kFsmThreads) out[w] = mask[w];
  }
}

}  // namespace

int vt_fsm_rows_launch(const vt_fsm_row* rows, int n_rows, int V, hipStream_t s) {
  VT_REQUIRE(V > 0 && V <= VT_SAMPLE_ROWS_MAX_V, "vt_fsm_rows: V=%d (0 < V <= %d)", V, VT_SAMPLE_ROWS_MAX_V);
  VT_REQUIRE(n_rows >= 0, "vt_fsm_rows: n_rows=%d", n_rows);
  if (n_rows == 0) return VT_OK;
  VT_REQUIRE(rows != nullptr, "vt_fsm_rows: rows is NULL with n_rows=%d", n_rows);
  VT_REQUIRE(((uintptr_t)rows % 8) == 0, "vt_fsm_rows: rows must be 8-byte aligned");
  hipLaunchKernelGGL(fsm_rows_kernel, dim3(n_rows), dim3(kFsmThreads), 0, s, rows, V);
  VT_LAUNCH_CHECK();
  return VT_OK;
}
