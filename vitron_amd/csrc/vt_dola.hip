// vt_dola.hip -- vt_dola_rows: DoLa, "Decoding by Contrasting Layers" (Chuang et al. 2023), over logit rows -- the
// arithmetic of transformers 4.4x' _dola_decoding / _dola_select_contrast / _relative_top_filter. A row names the final layer's logit row
// and n_cand rows of early ("premature") layers' streams put through the lm_head. Per row, everything in fp32:
//     lse_x  = m + logf(sum_i expf(x_i - m)),  m = max x                                  (vt_rows.h; vt_logprob_rows' too)
//     div_j  = 0.5 * sum_i [ M (log M - lpf) + M (log M - lpj) ],  lpf = f_i - lse_f,  lpj = x_i - lse_j,  M = 0.5 (expf(lpf) + expf(lpj)),
//              a term with M == 0 counting 0                                              (F.kl_div(log_softmax, average): KL(M || p))
//     j*     = 0;  for j = 1 .. n_cand - 1:  if div_j > div_j*:  j* = j                    (the largest, ties and NaNs to the lower j)
//     out_i  = f_i >= m_f + log_relative_top  ?  (f_i - lse_f) - (x_i - lse_j*)  :  -inf   (x = candidate j*)
// with each of the three subtractions of out rounded on its own, so that `out` follows bit for bit from the inputs, two lse values and
// j*. mask_out bit i = base bit i AND (f_i >= m_f + log_relative_top), vt_rows.h's layout and tail-bit rule, as vt_cfg_rows'. One
// candidate: j* = 0 and no divergence is computed (div_out[0] = 0).
// One launch, one 1024-thread block per row; no workspace, no atomics, plain vector stores only. Two forms, chosen per ROW:
//   register form (V <= 32 * 1024; final, prem and out 16-byte aligned, prem_stride % 4 == 0): the final row is read ONCE and stays in
//     registers (thread t owns the floats 4 (t + 1024 j) + k); every candidate is read once into a second set of 32 registers, where its
//     maximum, its sum and its divergence are taken; the chosen candidate is read again (L2) for the write unless it was the last one.
//   re-read form (anything else): a thread streams the elements t + 1024 j: the final row twice for its lse, each candidate three times
//     (maximum, sum, divergence; the final row beside it the third time), and both rows once more for the write.
// Every candidate of a row runs the same form and the same reduction order, so two bitwise equal candidate rows have bitwise equal
// lse and div. `out` may alias `final`: a thread writes only elements it alone reads, after the last block reduction.
// NaN and +-inf propagate by IEEE rules (fmaxf skips a NaN, the sums do not); a NaN div is never chosen over an earlier candidate.
#include "vt_common.h"
#include "vt_kernels.h"
#include "vt_rows.h"

static_assert(sizeof(vt_dola_row) == 80 && alignof(vt_dola_row) == 8, "vt_dola_row is 80 bytes, 8-byte aligned (ABI)");
static_assert(offsetof(vt_dola_row, final) == 0 && offsetof(vt_dola_row, prem) == 8 && offsetof(vt_dola_row, out) == 16 &&
                  offsetof(vt_dola_row, base) == 24 && offsetof(vt_dola_row, mask_out) == 32 && offsetof(vt_dola_row, layer_out) == 40 &&
                  offsetof(vt_dola_row, div_out) == 48 && offsetof(vt_dola_row, lse_out) == 56 && offsetof(vt_dola_row, prem_stride) == 64 &&
                  offsetof(vt_dola_row, n_cand) == 72 && offsetof(vt_dola_row, log_relative_top) == 76,
              "vt_dola_row offsets are part of the ABI");

namespace {

// one term of the divergence; every operation rounded on its own (tests/dola_ref.py restates it in numpy float32)
__device__ __forceinline__ float dola_term(float f, float x, float lse_f, float lse_j) {
#pragma clang fp contract(off)
  const float lpf = f - lse_f;
  const float lpj = x - lse_j;
  const float m = 0.5f * (expf(lpf) + expf(lpj));
  const float lm = logf(m);
  const float t = m * (lm - lpf) + m * (lm - lpj);
  return m == 0.f ? 0.f : t;
}
// the contrast, three subtractions each rounded on its own (see cfg_blend in vt_cfg.hip on why the operators are written out)
__device__ __forceinline__ float dola_out(float f, float x, float lse_f, float lse_j, float thr) {
#pragma clang fp contract(off)
  const float a = f - lse_f;
  const float b = x - lse_j;
  const float r = a - b;
  return f >= thr ? r : -INFINITY;
}
// The lse, the mask's starting word and the two mask builders are vt_rows.h's. (tests/test_dola_ref_host.py reads dola_out's body as
// the text up to "__device__ __forceinline__ uint32_t dola_base_word", the function that stood here: it is row_base_word now.)
template <bool kReg>
__global__ __launch_bounds__(kRowThreads) void dola_rows_kernel(const vt_dola_row* __restrict__ rows, int V) {
  __shared__ float sh[16];
  const vt_dola_row row = rows[blockIdx.x];
  if (row.final == nullptr) return;      // block-uniform, before any barrier: the row is skipped entirely
  const int tid = threadIdx.x;
  const int n_cand = row.n_cand;
  if (n_cand < 1 || n_cand > VT_DOLA_MAX_LAYERS) {     // bad row content: nothing is read or written but layer_out = -1
    if (tid == 0 && row.layer_out != nullptr) *row.layer_out = -1;
    return;
  }
  const float* fin = row.final;          // (no __restrict__: out may alias final)
  const float* prem = row.prem;
  const long long stride = row.prem_stride;
  float* out = row.out;
  const bool aligned = (((uintptr_t)fin | (uintptr_t)prem | (uintptr_t)out) % 16) == 0 && (stride % 4) == 0;     // block-uniform

  if (kReg && aligned) {
    float f[32], x[32];
    row_load32(fin, V, tid, f);
    float mf;
    const float lse_f = row_lse32(f, sh, mf);
    if (tid == 0 && row.lse_out != nullptr) row.lse_out[0] = lse_f;
    int jb = 0;
    float db = 0.f, lse_b = 0.f;
    for (int j = 0; j < n_cand; ++j) {
      row_load32(prem + j * stride, V, tid, x);
      float mj;
      const float lse_j = row_lse32(x, sh, mj);
      float d = 0.f;
      if (n_cand > 1) {                  // block-uniform
        // lse_f through an empty asm: otherwise the compiler hoists the 32 f_i - lse_f and their expf out of the candidate loop, 64
        // more live registers next to f[] and x[] under the 128 of a 1024-thread block (324 bytes of scratch per lane; 48 with this,
        // none of them touched inside this loop)
        float lf = lse_f;
        asm volatile("" : "+v"(lf));
#pragma unroll
        for (int s = 0; s < 32; ++s) d += dola_term(f[s], x[s], lf, lse_j);
        d = 0.5f * row_block_sum(d, sh);
      }
      if (tid == 0) {
        if (row.lse_out != nullptr) row.lse_out[1 + j] = lse_j;
        if (row.div_out != nullptr) row.div_out[j] = d;
      }
      if (j == 0 || d > db) {            // block-uniform: every thread holds the same totals
        jb = j;
        db = d;
        lse_b = lse_j;
      }
    }
    if (tid == 0 && row.layer_out != nullptr) *row.layer_out = jb;
    if (jb != n_cand - 1) row_load32(prem + jb * stride, V, tid, x);
    const float thr = mf + row.log_relative_top;
    if (row.mask_out != nullptr)         // block-uniform: every lane takes part in the shuffles
      row_mask32(row.mask_out, row.base, V, tid, [&](int s) { return f[s] >= thr; });
    row_store32(out, V, tid, [&](int s) { return dola_out(f[s], x[s], lse_f, lse_b, thr); });
    return;
  }

  float mf;
  const float lse_f = row_lse_stream(fin, V, tid, sh, mf);
  if (tid == 0 && row.lse_out != nullptr) row.lse_out[0] = lse_f;
  int jb = 0;
  float db = 0.f, lse_b = 0.f;
  for (int j = 0; j < n_cand; ++j) {
    const float* xr = prem + j * stride;
    float mj;
    const float lse_j = row_lse_stream(xr, V, tid, sh, mj);
    float d = 0.f;
    if (n_cand > 1) {
      for (int i = tid; i < V; i += kRowThreads) d += dola_term(fin[i], xr[i], lse_f, lse_j);
      d = 0.5f * row_block_sum(d, sh);
    }
    if (tid == 0) {
      if (row.lse_out != nullptr) row.lse_out[1 + j] = lse_j;
      if (row.div_out != nullptr) row.div_out[j] = d;
    }
    if (j == 0 || d > db) {
      jb = j;
      db = d;
      lse_b = lse_j;
    }
  }
  if (tid == 0 && row.layer_out != nullptr) *row.layer_out = jb;
  const float* xb = prem + jb * stride;
  const float thr = mf + row.log_relative_top;
  const bool want_mask = row.mask_out != nullptr;
  for (int b0 = 0; b0 < V; b0 += kRowThreads) {     // a block-uniform trip count: every lane reaches the ballot
    const int i = b0 + tid;
    const bool in = i < V;
    const float fi = in ? fin[i] : 0.f;
    const float xi = in ? xb[i] : 0.f;
    if (want_mask) row_mask_ballot(row.mask_out, row.base, V, b0, tid, (!in) | (fi >= thr));
    if (in) out[i] = dola_out(fi, xi, lse_f, lse_b, thr);
  }
}

}  // namespace

int vt_dola_rows_launch(const vt_dola_row* rows, int n_rows, int V, hipStream_t s) {
  VT_REQUIRE(rows != nullptr, "vt_dola_rows: rows is NULL");
  VT_REQUIRE(n_rows > 0, "vt_dola_rows: n_rows=%d (n_rows > 0)", n_rows);
  VT_REQUIRE(V > 0 && V <= VT_LOGPROB_MAX_V, "vt_dola_rows: V=%d (0 < V <= %d)", V, VT_LOGPROB_MAX_V);
  VT_REQUIRE(((uintptr_t)rows % 8) == 0, "vt_dola_rows: rows must be 8-byte aligned");
  if (V <= 32 * 1024)
    hipLaunchKernelGGL(dola_rows_kernel<true>, dim3(n_rows), dim3(kRowThreads), 0, s, rows, V);
  else
    hipLaunchKernelGGL(dola_rows_kernel<false>, dim3(n_rows), dim3(kRowThreads), 0, s, rows, V);
  VT_LAUNCH_CHECK();
  return VT_OK;
}
