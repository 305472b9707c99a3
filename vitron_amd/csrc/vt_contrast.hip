// vt_contrast.hip -- vt_unit_rows and vt_contrast_rows: the degeneration penalty of contrastive search (Su et al. 2022,
// transformers' penalty_alpha / top_k). Every candidate token's final hidden state is compared, by cosine similarity, with the final
// hidden state of EVERY earlier position; the candidate with the best (1 - alpha) p - alpha max_j cos wins.
//
// vt_unit_rows: out[r] = op16(y / |y|), y_i = w_i x[r][i], one 256-thread block per row, everything in fp32. With w = final_norm this is
//   the direction of the final-normed state (RMSNorm's scalar cancels in a cosine). H <= 4096 with 16-byte aligned rows keeps the row
//   in registers (one read, 37 VGPRs); any other row is read twice (11 VGPRs). No scratch, 16 bytes of LDS, 8 waves per SIMD.
//
// vt_contrast_rows, two stages, no atomics, plain vector stores only:
//   stage 1, contrast_dots_kernel: grid (chunks of 16 bank rows, groups), 512 threads = 8 waves. The 16 bank rows of a chunk are the
//     16-row A operand of v_mfma_f32_16x16x32, the group's k <= 16 candidates the 16 columns of B (columns >= k are zero registers and
//     load nothing). Both operands go from global memory straight into the MFMA fragments with 16-byte loads -- lane l holds
//     row (l & 15), k = 8 (l >> 4) + j -- so there is no LDS staging and no banking question: the candidates (k x H x 2 bytes, 32 KiB at
//     k = 4, H = 4096) are re-read from L2 by every block, the bank is streamed exactly once. The K dimension is sliced over the
//     8 waves (wave w takes the 32-wide steps w, w + 8, ...), 8 steps per wave in flight at once (two rounds at H = 4096); the 8 partial
//     16 x 16 tiles meet in 8 KiB of LDS and are summed in wave order, the rows >= T are masked to -inf and the chunk's per-candidate
//     maximum goes to the workspace. Bank rows >= T are never read (their lanes load nothing).
//     80 VGPRs, no scratch, 9 KiB of LDS: 6 waves per SIMD = 3 blocks per CU by registers (16 steps in flight were 144 VGPRs and one
//     block per CU: the 336 blocks of T = 5376 then ran in two rounds).
//   stage 2, contrast_pick_kernel: one 512-thread block per group: thread t folds the chunk maxima (t >> 4) + 32 i of candidate t & 15
//     (a wave reads 64 consecutive floats per load), the 32 partial maxima per candidate meet in LDS, then the scores, the arg-max
//     (serial over k <= 16 in thread 0: `sel` starts at 0 and moves only on a strictly greater score, so it lies in [0, k) whatever the
//     inputs), and bank[T] = cand[first + sel] with 16-byte copies of the very bits that were compared. 36 VGPRs, no scratch, 2.1 KiB
//     of LDS. (A first form walked the chunks serially in k threads: 336 dependent L2 round trips, 48 us at T = 5376.)
// The row array is a HOST array: the launcher checks every field before anything runs and hands the rows to the kernels by value, 32
// groups per launch pair.
#include "vt_common.h"
#include "vt_kernels.h"

static_assert(sizeof(vt_contrast_row) == 64 && alignof(vt_contrast_row) == 8, "vt_contrast_row is 64 bytes, 8-byte aligned (ABI)");
static_assert(offsetof(vt_contrast_row, bank) == 0 && offsetof(vt_contrast_row, cand_lp) == 8 && offsetof(vt_contrast_row, d_out) == 16 &&
                  offsetof(vt_contrast_row, score_out) == 24 && offsetof(vt_contrast_row, sel_out) == 32 &&
                  offsetof(vt_contrast_row, bank_len) == 40 && offsetof(vt_contrast_row, bank_cap) == 44 && offsetof(vt_contrast_row, k) == 48 &&
                  offsetof(vt_contrast_row, first) == 52 && offsetof(vt_contrast_row, alpha) == 56,
              "vt_contrast_row offsets are part of the ABI");

namespace {

constexpr int kUnitThreads = 256;
constexpr int kUnitRegs = 4;                      // 16-byte pieces of x per thread in the register form
constexpr int kChunk = VT_CONTRAST_CHUNK;         // bank rows per block: the MFMA's 16-row operand
constexpr int kDotWaves = 8;
constexpr int kDotUnroll = 8;                     // K steps of 32 a wave holds in flight
constexpr int kPickThreads = 512;
constexpr int kGroupsPerLaunch = 32;

struct ContrastRows {
  vt_contrast_row r[kGroupsPerLaunch];
};

__device__ __forceinline__ float unit_block_sum(float v, float* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < kUnitThreads / 64; ++i) t += sh[i];
  return t;
}

// kReg: H <= kUnitThreads * kUnitRegs * 4, x rows 16-byte aligned, H % 4 == 0: thread t owns the floats 4 (t + 256 j) + e
template <bool kReg>
__global__ __launch_bounds__(kUnitThreads) void unit_rows_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                                                 op16_t* __restrict__ out, int ldo, int H) {
  __shared__ float sh[kUnitThreads / 64];
  const int tid = threadIdx.x;
  const float* xr = x + (size_t)blockIdx.x * ldx;
  op16_t* orow = out + (size_t)blockIdx.x * ldo;
  if (kReg) {
    float y[kUnitRegs][4];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < kUnitRegs; ++j) {
      const int i0 = 4 * (tid + kUnitThreads * j);
      f32x4 v = {0.f, 0.f, 0.f, 0.f}, ww = {1.f, 1.f, 1.f, 1.f};
      if (i0 < H) {
        v = *(const f32x4*)(xr + i0);
        if (w != nullptr) ww = *(const f32x4*)(w + i0);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        y[j][e] = ww[e] * v[e];
        ss = __builtin_fmaf(y[j][e], y[j][e], ss);
      }
    }
    ss = unit_block_sum(ss, sh);
    const float rn = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
#pragma unroll
    for (int j = 0; j < kUnitRegs; ++j) {
      const int i0 = 4 * (tid + kUnitThreads * j);
      if (i0 < H) {
        u32x2 o;
        o[0] = pack_op2(y[j][0] * rn, y[j][1] * rn);
        o[1] = pack_op2(y[j][2] * rn, y[j][3] * rn);
        *(u32x2*)(orow + i0) = o;
      }
    }
    return;
  }
  float ss = 0.f;
  for (int i = tid; i < H; i += kUnitThreads) {
    const float yi = (w != nullptr ? w[i] : 1.f) * xr[i];
    ss = __builtin_fmaf(yi, yi, ss);
  }
  ss = unit_block_sum(ss, sh);
  const float rn = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
  for (int i = tid; i < H; i += kUnitThreads) {
    const float yi = (w != nullptr ? w[i] : 1.f) * xr[i];
    orow[i] = f32_to_op(yi * rn);
  }
}

// stage 1: the chunk's 16 bank rows x the group's candidates, K sliced over the waves; ws[(group * ws_chunks + chunk) * 16 + c]
__global__ __launch_bounds__(kDotWaves * 64) void contrast_dots_kernel(const ContrastRows rows, const op16_t* __restrict__ cand, int ld, int H,
                                                                        float* __restrict__ ws, int ws_chunks, int g0) {
  __shared__ float part[kDotWaves][kChunk][16];
  __shared__ float tile[kChunk][16];
  const vt_contrast_row row = rows.r[blockIdx.y];
  const int T = row.bank_len;
  const int j0 = blockIdx.x * kChunk;
  if (j0 >= T) return;                                       // block-uniform, before any barrier
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const bool a_ok = j0 + r < T;                              // a bank row at or beyond T is never read
  const bool b_ok = r < row.k;                               // an unused operand column is zero registers
  const op16_t* ap = (const op16_t*)row.bank + (size_t)(j0 + (a_ok ? r : 0)) * H + q * 8;
  const op16_t* bp = cand + (size_t)(row.first + (b_ok ? r : 0)) * ld + q * 8;
  const int n_steps = H >> 5;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s0 = wave; s0 < n_steps; s0 += kDotWaves * kDotUnroll) {
    u32x4 A[kDotUnroll], B[kDotUnroll];
#pragma unroll
    for (int u = 0; u < kDotUnroll; ++u) {
      const int s = s0 + kDotWaves * u;
      const bool ok = s < n_steps;
      A[u] = (ok && a_ok) ? *(const u32x4*)(ap + (size_t)s * 32) : (u32x4){0u, 0u, 0u, 0u};
      B[u] = (ok && b_ok) ? *(const u32x4*)(bp + (size_t)s * 32) : (u32x4){0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int u = 0; u < kDotUnroll; ++u) acc = VT_MFMA_16x16x32(__builtin_bit_cast(bf16x8, A[u]), __builtin_bit_cast(bf16x8, B[u]), acc);
  }
  // acc[e] = D[bank row 4 q + e][candidate r]  (4-way bank conflicts on these 4 stores per lane, once per block)
#pragma unroll
  for (int e = 0; e < 4; ++e) part[wave][4 * q + e][r] = acc[e];
  __syncthreads();
  if (tid < kChunk * 16) {
    const int br = tid >> 4, c = tid & 15;
    float v = part[0][br][c];
#pragma unroll
    for (int wv = 1; wv < kDotWaves; ++wv) v += part[wv][br][c];
    tile[br][c] = j0 + br < T ? v : -INFINITY;
  }
  __syncthreads();
  if (tid < 16) {
    float m = tile[0][tid];
#pragma unroll
    for (int br = 1; br < kChunk; ++br) m = fmaxf(m, tile[br][tid]);
    ws[((size_t)(g0 + blockIdx.y) * ws_chunks + blockIdx.x) * 16 + tid] = m;
  }
}

// stage 2: d, score, sel of one group, and the append. Thread t folds the chunks (t >> 4), (t >> 4) + 32, ... of candidate t & 15 --
// a wave reads 64 consecutive floats of the workspace per load -- then the 32 partial maxima per candidate meet in LDS.
__global__ __launch_bounds__(kPickThreads) void contrast_pick_kernel(const ContrastRows rows, const op16_t* __restrict__ cand, int ld, int H,
                                                                      const float* __restrict__ ws, int ws_chunks, int g0) {
  __shared__ float part[kPickThreads / 16][16];
  __shared__ float sc[16];
  __shared__ int sel_sh;
  const vt_contrast_row row = rows.r[blockIdx.x];
  const int tid = threadIdx.x;
  const int T = row.bank_len, k = row.k;
  const int nch = (T + kChunk - 1) / kChunk;
  const float* p = ws + (size_t)(g0 + blockIdx.x) * ws_chunks * 16 + (tid & 15);
  float m = -INFINITY;
#pragma unroll 4
  for (int ch = tid >> 4; ch < nch; ch += kPickThreads / 16) m = fmaxf(m, p[(size_t)ch * 16]);
  part[tid >> 4][tid & 15] = m;
  __syncthreads();
  if (tid < k) {
    float d = part[0][tid];
#pragma unroll
    for (int i = 1; i < kPickThreads / 16; ++i) d = fmaxf(d, part[i][tid]);
    const float t = (1.0f - row.alpha) * __expf(row.cand_lp[tid]);     // rounded on its own; the fma below rounds once more
    const float s = __builtin_fmaf(-row.alpha, d, t);
    row.d_out[tid] = d;
    row.score_out[tid] = s;
    sc[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    int sel = 0;
    float best = sc[0];
    for (int c = 1; c < k; ++c)
      if (sc[c] > best) {          // strictly greater: an exact tie stays with the lower c, a NaN never wins
        best = sc[c];
        sel = c;
      }
    row.sel_out[0] = sel;
    sel_sh = sel;
  }
  __syncthreads();
  const u32x4* src = (const u32x4*)(cand + (size_t)(row.first + sel_sh) * ld);
  u32x4* dst = (u32x4*)((op16_t*)row.bank + (size_t)T * H);
  for (int i = tid; i < (H >> 3); i += kPickThreads) dst[i] = src[i];
}

}  // namespace

int vt_unit_rows_launch(const float* x, int ldx, const float* w, op16_t* out, int ldo, int rows, int H, hipStream_t s) {
  VT_REQUIRE(x != nullptr && out != nullptr, "vt_unit_rows: x or out is NULL");
  VT_REQUIRE(rows > 0 && H > 0, "vt_unit_rows: rows=%d H=%d (both > 0)", rows, H);
  VT_REQUIRE(ldx >= H && ldo >= H, "vt_unit_rows: ldx=%d ldo=%d must be >= H=%d", ldx, ldo, H);
  const bool reg = H <= kUnitThreads * kUnitRegs * 4 && (H % 4) == 0 && (ldx % 4) == 0 && (ldo % 4) == 0 && ((uintptr_t)x % 16) == 0 &&
                   ((uintptr_t)out % 8) == 0 && (w == nullptr || ((uintptr_t)w % 16) == 0);
  if (reg)
    hipLaunchKernelGGL(unit_rows_kernel<true>, dim3(rows), dim3(kUnitThreads), 0, s, x, ldx, w, out, ldo, H);
  else
    hipLaunchKernelGGL(unit_rows_kernel<false>, dim3(rows), dim3(kUnitThreads), 0, s, x, ldx, w, out, ldo, H);
  VT_LAUNCH_CHECK();
  return VT_OK;
}

static size_t contrast_workspace_bytes(int n_groups, int max_bank_len) { return VT_CONTRAST_WORKSPACE_BYTES(n_groups, max_bank_len); }

int vt_contrast_rows_launch(const vt_contrast_row* rows, int n_groups, const op16_t* cand, int n_cand, int ld, int H, void* workspace,
                            size_t workspace_bytes, hipStream_t s) {
  VT_REQUIRE(rows != nullptr && cand != nullptr, "vt_contrast_rows: rows or cand is NULL");
  VT_REQUIRE(n_groups > 0, "vt_contrast_rows: n_groups=%d (n_groups > 0)", n_groups);
  VT_REQUIRE(H > 0 && (H % 32) == 0, "vt_contrast_rows: H=%d must be a positive multiple of 32", H);
  VT_REQUIRE(ld >= H && (ld % 8) == 0, "vt_contrast_rows: ld=%d must be >= H=%d and a multiple of 8", ld, H);
  VT_REQUIRE(n_cand > 0, "vt_contrast_rows: n_cand=%d (n_cand > 0)", n_cand);
  VT_REQUIRE(((uintptr_t)cand % 16) == 0, "vt_contrast_rows: cand must be 16-byte aligned");
  int max_T = 0;
  for (int g = 0; g < n_groups; ++g) {
    const vt_contrast_row& r = rows[g];
    VT_REQUIRE(r.bank != nullptr && ((uintptr_t)r.bank % 16) == 0, "vt_contrast_rows: group %d: bank is NULL or not 16-byte aligned", g);
    VT_REQUIRE(r.cand_lp != nullptr && r.d_out != nullptr && r.score_out != nullptr && r.sel_out != nullptr,
               "vt_contrast_rows: group %d: cand_lp, d_out, score_out and sel_out must not be NULL", g);
    VT_REQUIRE(r.k >= 1 && r.k <= VT_CONTRAST_MAX_K, "vt_contrast_rows: group %d: k=%d (1 <= k <= %d)", g, r.k, VT_CONTRAST_MAX_K);
    VT_REQUIRE(r.bank_len >= 1, "vt_contrast_rows: group %d: bank_len=%d (bank_len >= 1)", g, r.bank_len);
    VT_REQUIRE(r.bank_len < r.bank_cap, "vt_contrast_rows: group %d: bank_len=%d leaves no row to append in a bank of %d", g, r.bank_len,
               r.bank_cap);
    VT_REQUIRE(r.first >= 0 && r.first <= n_cand - r.k, "vt_contrast_rows: group %d: candidates [%d, %d) outside cand's %d rows", g, r.first,
               r.first + r.k, n_cand);
    VT_REQUIRE(r.alpha >= 0.f && r.alpha <= 1.f, "vt_contrast_rows: group %d: alpha=%g outside [0, 1]", g, (double)r.alpha);
    max_T = r.bank_len > max_T ? r.bank_len : max_T;
  }
  const int ws_chunks = (max_T + kChunk - 1) / kChunk;
  VT_REQUIRE(workspace != nullptr && ((uintptr_t)workspace % 4) == 0, "vt_contrast_rows: workspace is NULL or misaligned");
  VT_REQUIRE(workspace_bytes >= contrast_workspace_bytes(n_groups, max_T),
             "vt_contrast_rows: workspace of %zu bytes, %zu needed (n_groups * ceil(max bank_len / %d) * 64)", workspace_bytes,
             contrast_workspace_bytes(n_groups, max_T), kChunk);
  for (int g0 = 0; g0 < n_groups; g0 += kGroupsPerLaunch) {
    const int n = n_groups - g0 < kGroupsPerLaunch ? n_groups - g0 : kGroupsPerLaunch;
    ContrastRows a;
    int chunks = 0;
    for (int g = 0; g < n; ++g) {
      a.r[g] = rows[g0 + g];
      const int c = (a.r[g].bank_len + kChunk - 1) / kChunk;
      chunks = c > chunks ? c : chunks;
    }
    for (int g = n; g < kGroupsPerLaunch; ++g) a.r[g] = a.r[0];
    hipLaunchKernelGGL(contrast_dots_kernel, dim3(chunks, n), dim3(kDotWaves * 64), 0, s, a, cand, ld, H, (float*)workspace, ws_chunks, g0);
    VT_LAUNCH_CHECK();
    hipLaunchKernelGGL(contrast_pick_kernel, dim3(n), dim3(kPickThreads), 0, s, a, cand, ld, H, (const float*)workspace, ws_chunks, g0);
    VT_LAUNCH_CHECK();
  }
  return VT_OK;
}
