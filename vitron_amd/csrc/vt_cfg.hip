// vt_cfg.hip -- vt_cfg_rows: classifier-free guidance over logit rows, the arithmetic of transformers'
// UnbatchedClassifierFreeGuidanceLogitsProcessor (guidance_scale / negative_prompt_ids) and of contrastive decoding. A row names a
// conditional and an unconditional logit row; the guided row is
//     out_i = ul_i + scale * (cl_i - ul_i),   cl = c - lse_c,   ul = u - lse_u,   lse = m + logf(sum_i expf(x_i - m)),  m = max x
// with every one of the three blend steps and the two subtractions rounded to fp32 on its own (no fused multiply-add: cfg_blend
// switches hipcc's contraction off), so that `out` follows bit for bit from the kernel's own lse values. Optionally the adaptive plausibility
// mask of contrastive decoding: bit i = base bit i AND c_i >= m_c + log_beta.
// One launch, one 1024-thread block per row; no workspace, no atomics, plain vector stores only.
//   register form (V <= 32 * 1024 and cond, uncond, out 16-byte aligned): both rows are read ONCE, 2 x 32 values per thread -- thread t
//     owns the floats 4 (t + 1024 j) + k -- and the reductions and the write run over registers. A mask word is 8 neighbouring lanes'
//     nibbles, gathered with three shuffles.
//   re-read form (anything else; chosen per ROW, since rows carry their own pointers): a thread streams the elements t + 1024 j three
//     times (maximum, sum, write); the second and third reads come from L2. A wave's 64 elements are two mask words: one ballot.
// `out` may alias `cond`: in the register form every read precedes the block reductions and every write follows them; in the re-read
// form a thread writes only the element it has just read, after the reductions. NaN and +-inf propagate by IEEE rules (fmaxf skips a
// NaN, the sum does not: a row that holds one has lse = NaN); nothing is special-cased.
#include "vt_common.h"
#include "vt_kernels.h"
#include "vt_rows.h"

static_assert(sizeof(vt_cfg_row) == 56 && alignof(vt_cfg_row) == 8, "vt_cfg_row is 56 bytes, 8-byte aligned (ABI)");
static_assert(offsetof(vt_cfg_row, cond) == 0 && offsetof(vt_cfg_row, uncond) == 8 && offsetof(vt_cfg_row, out) == 16 &&
                  offsetof(vt_cfg_row, base) == 24 && offsetof(vt_cfg_row, mask_out) == 32 && offsetof(vt_cfg_row, lse_out) == 40 &&
                  offsetof(vt_cfg_row, scale) == 48 && offsetof(vt_cfg_row, log_beta) == 52,
              "vt_cfg_row offsets are part of the ABI");

namespace {

// The blend, every step rounded to nearest on its own: __fsub_rn / __fmul_rn / __fadd_rn in the header's statement of the contract.
// hipcc compiles those intrinsics as plain operators that carry its default contraction flag, so after inlining it fuses
// ul + s * d into an fma all the same (seen in the assembly: v_fmac_f32); the operators are therefore written out under
// fp contract(off), as vt_sample.hip's add_rounded is, which is what keeps the product and the sum apart.
__device__ __forceinline__ float cfg_blend(float c, float u, float lse_c, float lse_u, float scale) {
#pragma clang fp contract(off)
  const float cl = c - lse_c;
  const float ul = u - lse_u;
  const float d = cl - ul;
  const float p = scale * d;
  return ul + p;
}
// word w of the starting mask (base's word as it is, or the bits [0, V)) and the two mask builders are vt_rows.h's, as are the
// reductions: the two rows' share their barriers (N = 2).
template <bool kReg>
__global__ __launch_bounds__(kRowThreads) void cfg_rows_kernel(const vt_cfg_row* __restrict__ rows, int V) {
  __shared__ float sh[2][16];
  const vt_cfg_row row = rows[blockIdx.x];
  if (row.cond == nullptr) return;       // block-uniform, before any barrier: the row is skipped entirely
  const int tid = threadIdx.x;
  const float* cond = row.cond;          // (no __restrict__: out may alias cond)
  const float* unc = row.uncond;
  float* out = row.out;
  const float scale = row.scale;
  const bool aligned = (((uintptr_t)cond | (uintptr_t)unc | (uintptr_t)out) % 16) == 0;     // block-uniform
  const float* const both[2] = {cond, unc};
  float mx[2], lse[2];                   // [0]: cond, [1]: uncond

  if (kReg && aligned) {
    float x[2][32];
    row_load32(both, V, tid, x);
    row_lse32(x, sh, mx, lse);
    if (tid == 0 && row.lse_out != nullptr) {
      row.lse_out[0] = lse[0];
      row.lse_out[1] = lse[1];
    }
    if (row.mask_out != nullptr) {       // block-uniform: every lane takes part in the shuffles
      const float thr = mx[0] + row.log_beta;
      row_mask32(row.mask_out, row.base, V, tid, [&](int s) { return x[0][s] >= thr; });
    }
    row_store32(out, V, tid, [&](int s) { return cfg_blend(x[0][s], x[1][s], lse[0], lse[1], scale); });
    return;
  }

  row_lse_stream(both, V, tid, sh, mx, lse);
  if (tid == 0 && row.lse_out != nullptr) {
    row.lse_out[0] = lse[0];
    row.lse_out[1] = lse[1];
  }
  const float thr = mx[0] + row.log_beta;
  const bool want_mask = row.mask_out != nullptr;
  for (int b0 = 0; b0 < V; b0 += kRowThreads) {     // a block-uniform trip count: every lane reaches the ballot
    const int i = b0 + tid;
    const bool in = i < V;
    const float ci = in ? cond[i] : 0.f;
    const float ui = in ? unc[i] : 0.f;
    if (want_mask) row_mask_ballot(row.mask_out, row.base, V, b0, tid, (!in) | (ci >= thr));
    if (in) out[i] = cfg_blend(ci, ui, lse[0], lse[1], scale);
  }
}

}  // namespace

int vt_cfg_rows_launch(const vt_cfg_row* rows, int n_rows, int V, hipStream_t s) {
  VT_REQUIRE(rows != nullptr, "vt_cfg_rows: rows is NULL");
  VT_REQUIRE(n_rows > 0, "vt_cfg_rows: n_rows=%d (n_rows > 0)", n_rows);
  VT_REQUIRE(V > 0 && V <= VT_LOGPROB_MAX_V, "vt_cfg_rows: V=%d (0 < V <= %d)", V, VT_LOGPROB_MAX_V);
  VT_REQUIRE(((uintptr_t)rows % 8) == 0, "vt_cfg_rows: rows must be 8-byte aligned");
  if (V <= 32 * 1024)
    hipLaunchKernelGGL(cfg_rows_kernel<true>, dim3(n_rows), dim3(kRowThreads), 0, s, rows, V);
  else
    hipLaunchKernelGGL(cfg_rows_kernel<false>, dim3(n_rows), dim3(kRowThreads), 0, s, rows, V);
  VT_LAUNCH_CHECK();
  return VT_OK;
}
