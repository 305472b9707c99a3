// vt_api.hip -- the extern "C" surface of libvitron_hip.so (include/vitron_hip.h) and the host-side
// orchestration of the composite operators (ViT tower, projector, region extractor, LLaMA decoder).
// The orchestration is plain stream-ordered kernel launches: no allocation, no synchronisation, no
// hidden state -- so a whole tower / decoder pass is ONE ctypes call from Python.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "vt_common.h"
#include "vt_kernels.h"

// ---- error plumbing --------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void vt_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---- profiling ---------------------------------------------------------------------------------------------------
#include <mutex>
#include <vector>
namespace {
struct ProfRec {
  hipEvent_t a, b;
  int cls;
  double work;
};
std::mutex g_prof_mu;
bool g_prof_on = false;
std::vector<ProfRec> g_prof_recs;
std::vector<hipEvent_t> g_prof_pool;
hipEvent_t prof_event() {
  if (!g_prof_pool.empty()) {
    hipEvent_t e = g_prof_pool.back();
    g_prof_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}
}  // namespace
bool vt_prof_enabled() { return g_prof_on; }
void vt_prof_start(int cls, double work, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  ProfRec r{prof_event(), prof_event(), cls, work};
  if (!r.a || !r.b) return;
  if (hipEventRecord(r.a, s) != hipSuccess) return;   // profiling is best effort: an unrecorded pair is simply not counted
  g_prof_recs.push_back(r);
}
void vt_prof_stop(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (!g_prof_recs.empty() && hipEventRecord(g_prof_recs.back().b, s) != hipSuccess) g_prof_recs.pop_back();
}

namespace {
struct Carver {  // bump allocator over the caller's workspace
  char* base;
  size_t cap, off;
  Carver(void* p, size_t n) : base((char*)p), cap(n), off(0) {}
  void* take(size_t bytes) {
    off = align_up(off, 256);
    void* r = base ? base + off : nullptr;
    off += bytes;
    return r;
  }
  bool ok() const { return off <= cap; }
};
inline hipStream_t S(void* s) { return (hipStream_t)s; }
inline hipStream_t S_(void* s) { return (hipStream_t)s; }
}  // namespace

namespace {
// vt_probe_mfma: the matrix pipe alone (include/vitron_hip.h). 8 x 8 accumulator quads = the 128 x 128 wave tile of gemm_w4_kernel,
// two k-halves of fragments held in registers, 128 MFMAs per iteration and nothing else.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void probe_mfma_kernel(const bf16x8* __restrict__ a,
                                                                                                    const bf16x8* __restrict__ b,
                                                                                                    float* __restrict__ out, int iters) {
  const int t = threadIdx.x + blockIdx.x * 256;
  bf16x8 fa[2][8], fb[2][8];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      fa[h][i] = a[(t * 16 + h * 8 + i) & 0xffff];
      fb[h][i] = b[(t * 16 + h * 8 + i) & 0xffff];
    }
  f32x4 acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = VT_MFMA_16x16x32(fa[h][i], fb[h][j], acc[i][j]);
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) s += acc[i][j][0] + acc[i][j][3];
  out[t] = s;
}
}  // namespace

// vt_probe_read: what a kernel that does NOTHING BUT read sustains from HBM on this device (include/vitron_hip.h): 16 bytes per lane and load,
// eight loads in flight per lane, sixteen workgroups per CU walking the buffer with a grid stride; the values are folded into one word per lane and
// one conditional store keeps the loads alive. nt = 1: the read-once cache policy of the weight-streaming GEMM.
namespace {
template <bool NT, int U>
__global__ __launch_bounds__(256) void probe_read_kernel(const u32x4* __restrict__ p, size_t n16, unsigned* __restrict__ out) {
  const size_t stride = (size_t)gridDim.x * 256;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  u32x4 acc = {0u, 0u, 0u, 0u};
  for (; i + (U - 1) * stride < n16; i += U * stride) {
    u32x4 v[U];
#pragma unroll
    for (int k = 0; k < U; ++k) v[k] = NT ? __builtin_nontemporal_load(p + i + k * stride) : p[i + k * stride];
#pragma unroll
    for (int k = 0; k < U; ++k) acc ^= v[k];
  }
  for (; i < n16; i += stride) acc ^= NT ? __builtin_nontemporal_load(p + i) : p[i];
  if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x9e3779b9u) *out = 1u;
}
}  // namespace


extern "C" {

int vt_version(void) { return VT_ABI_VERSION; }

int vt_operand_format(void) { return VT_OPERAND_F16 ? VT_OPERAND_FP16 : VT_OPERAND_BF16; }

int vt_last_error(char* buf, size_t buf_len) {
  const size_t n = strlen(g_err);
  if (buf && buf_len) {
    const size_t c = n < buf_len - 1 ? n : buf_len - 1;
    memcpy(buf, g_err, c);
    buf[c] = 0;
  }
  return (int)n;
}

int vt_profile_begin(void) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (auto& r : g_prof_recs) {
    g_prof_pool.push_back(r.a);
    g_prof_pool.push_back(r.b);
  }
  g_prof_recs.clear();
  g_prof_on = true;
  return VT_OK;
}

int vt_probe_read(const void* p, size_t bytes, int nt, unsigned* out, void* stream) {
  VT_REQUIRE(p && out && bytes >= 16 && (((size_t)p) & 15) == 0, "vt_probe_read: null / misaligned pointer or fewer than 16 bytes");
  int dev = 0, ncu = 0;
  VT_HIP(hipGetDevice(&dev));
  VT_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  const size_t n16 = bytes / 16;
  // 8 loads in flight per lane x 16 workgroups per CU: the fastest of the shapes tried (round 6, GB/s with the read-once policy: 8 x 8 5481,
  // 16 x 8 5140, 8 x 16 5679, 16 x 4 5002; plain loads 5008 / 4769 / 5069 / 4742)
  if (nt) hipLaunchKernelGGL((probe_read_kernel<true, 8>), dim3(ncu * 16), dim3(256), 0, S(stream), (const u32x4*)p, n16, out);
  else hipLaunchKernelGGL((probe_read_kernel<false, 8>), dim3(ncu * 16), dim3(256), 0, S(stream), (const u32x4*)p, n16, out);
  VT_LAUNCH_CHECK();
  return VT_OK;
}

int vt_probe_mfma(const uint16_t* a, const uint16_t* b, float* out, int iters, void* stream) {
  VT_REQUIRE(a && b && out && iters > 0, "vt_probe_mfma: null pointer or iters <= 0");
  int dev = 0, ncu = 0;
  VT_HIP(hipGetDevice(&dev));
  VT_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  hipLaunchKernelGGL(probe_mfma_kernel, dim3(ncu), dim3(256), 0, S(stream), (const bf16x8*)a, (const bf16x8*)b, out, iters);
  VT_LAUNCH_CHECK();
  return VT_OK;
}

int vt_profile_end(int* launches, double* total_ms, double* total_work) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = false;
  for (int c = 0; c < VT_PROF_CLASSES; ++c) {
    if (launches) launches[c] = 0;
    if (total_ms) total_ms[c] = 0.0;
    if (total_work) total_work[c] = 0.0;
  }
  for (auto& r : g_prof_recs) {
    float ms = 0.f;
    // a record whose stop event was never recorded (a launch that bailed out early) is dropped, not an error
    const bool ok = hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    if (ok && r.cls >= 0 && r.cls < VT_PROF_CLASSES) {
      if (launches) launches[r.cls] += 1;
      if (total_ms) total_ms[r.cls] += ms;
      if (total_work) total_work[r.cls] += r.work;
    }
    g_prof_pool.push_back(r.a);
    g_prof_pool.push_back(r.b);
  }
  g_prof_recs.clear();
  return VT_OK;
}

// ---- primitives -----------------------------------------------------------------------------------------------------
int vt_gemm_bf16(const uint16_t* A, int lda, const uint16_t* W, int ldw, void* C, int ldc, const float* bias, int M,
                 int N, int K, int epi, int cfg, const float* row_scale, void* stream) {
  if (!row_scale) return vt_gemm_launch(A, lda, W, ldw, C, ldc, bias, M, N, K, epi, cfg, S(stream));
  VtGemmNormFuse nf;
  nf.row_scale = row_scale;
  return vt_gemm_launch(A, lda, W, ldw, C, ldc, bias, M, N, K, epi, cfg, S(stream), &nf);
}

int vt_gemm_plan_query(int M, int N, int K, int epi, int* cfg, int* rows_first) { return vt_gemm_plan_describe(M, N, K, epi, cfg, rows_first); }
int vt_gemm_plan_query2(int M, int N, int K, int epi, int* cfg, int* rows_first, int* cols_first) {
  return vt_gemm_plan_describe(M, N, K, epi, cfg, rows_first, cols_first);
}
int vt_gemm_plan_query3(int M, int N, int K, int epi, int* cfg, int* rows_first, int* cols_first, int* cfg_rest) {
  VT_REQUIRE(cols_first && cfg_rest, "vt_gemm_plan_query3: bad arguments");
  return vt_gemm_plan_describe(M, N, K, epi, cfg, rows_first, cols_first, cfg_rest);
}

int vt_gemm_bf16_colsplit(const uint16_t* A, int lda, const uint16_t* W, int ldw, void* C, int ldc, const float* bias, int M, int N, int K,
                          int epi, int cfg_first, int cols_first, int cfg_rest, void* stream) {
  return vt_gemm_colsplit_launch(A, lda, W, ldw, C, ldc, bias, M, N, K, epi, cfg_first, cols_first, cfg_rest, S(stream));
}

int vt_layernorm(float* x, const float* temb, int T, int tokens_per_frame, const float* gamma, const float* beta,
                 uint16_t* y, int rows, int D, float eps, void* stream) {
  return vt_layernorm_launch(x, temb, T, tokens_per_frame, gamma, beta, y, rows, D, eps, S(stream));
}

int vt_rmsnorm(const float* x, const int* idx, const float* w, uint16_t* y, int rows, int D, float eps, void* stream) {
  return vt_rmsnorm_launch(x, idx, w, y, rows, D, eps, S(stream));
}

int vt_flash_attn(const uint16_t* Q, int ldq, const uint16_t* k_tiles, const uint16_t* vt_tiles, const int* tile_table,
                  const int* seq_desc, int nseq, int max_q_len, uint16_t* O, int ldo, int heads, int head_dim,
                  int causal, float scale, void* stream) {
  return vt_flash_attn_launch(Q, ldq, k_tiles, vt_tiles, tile_table, (const VtAttnSeq*)seq_desc, nseq, max_q_len, O,
                              ldo, heads, head_dim, causal, scale, S(stream));
}

int vt_flash_attn_select(int kernel) {
  const int k = kernel & 0xff, wgs = kernel >> 8;
  VT_REQUIRE(kernel >= 0 && k <= 5 && (wgs == 0 || k == 4),
             "vt_flash_attn_select: kernel %d (0 auto, 1 two-waves-per-SIMD, 2 one-wave-per-SIMD placed, 3 unplaced, 4 placed + persistent, "
             "5 placed in the grid's natural block order; bits 8.. = workgroup cap of 4)", kernel);
  g_vt_flash_attn_kernel = k == 5 ? 2 : k;
  g_vt_flash_attn_order = k == 5 ? 0 : 1;
  g_vt_flash_attn_wgs = wgs;
  return VT_OK;
}

int vt_flash_attn_block_order(int heads, int q_blocks, int nseq, int multiprocessors, int* order, int capacity) {
  VT_REQUIRE(heads > 0 && q_blocks > 0 && nseq > 0 && multiprocessors > 0, "vt_flash_attn_block_order: empty problem");
  const std::vector<int> o = vt_flash_attn_w4_block_order(heads, q_blocks, nseq, multiprocessors);
  VT_REQUIRE(o.empty() || (order && capacity >= (int)o.size()), "vt_flash_attn_block_order: order[] holds %d entries, need %d", capacity, (int)o.size());
  for (size_t i = 0; i < o.size(); ++i) order[i] = o[i];
  return (int)o.size();
}

int vt_attn_decode(const uint16_t* Q, int ldq, const uint16_t* k_tiles, const uint16_t* vt_tiles, const int* tile_table,
                   const int* seq_desc, int nseq, uint16_t* O, int ldo, int heads, int head_dim, float scale,
                   int max_kv_len, void* scratch, size_t scratch_bytes, void* stream) {
  return vt_attn_decode_launch(Q, ldq, k_tiles, vt_tiles, tile_table, (const VtAttnSeq*)seq_desc, nseq, O, ldo, heads,
                               head_dim, scale, max_kv_len, (float*)scratch, scratch_bytes, S(stream));
}

int vt_nf4_quant(const void* W, int src_dtype, int ldw, int N, int K, uint8_t* codes, float* absmax, void* stream) {
  return vt_nf4_quant_launch(W, src_dtype, ldw, N, K, codes, absmax, S(stream));
}
int vt_nf4_dequant(const uint8_t* codes, const float* absmax, int N, int K, uint16_t* W, int ldw, void* stream) {
  return vt_nf4_dequant_launch(codes, absmax, N, K, W, ldw, S(stream));
}
int vt_gemm_nf4(const uint16_t* A, int lda, const uint8_t* codes, const float* absmax, void* C, int ldc, int M, int N, int K, int epi,
                const float* in_partials, int in_n, float inv_dim, float eps, const float* out_w, uint16_t* out_xw, int ld_xw,
                float* out_partials, void* stream) {
  VtGemmNormFuse nf;
  nf.in_partials = in_partials;
  nf.in_n = in_n;
  nf.inv_dim = inv_dim;
  nf.eps = eps;
  nf.out_w = out_w;
  nf.out_xw = out_xw;
  nf.ld_xw = ld_xw;
  nf.out_partials = out_partials;
  return vt_gemm_nf4_launch(A, lda, codes, absmax, C, ldc, M, N, K, epi, nf, S(stream));
}
int vt_mx4_quant_weights(const uint16_t* W, int ldw, int N, int K, uint8_t* W4, uint8_t* wexp, void* stream) {
  return vt_mx4_quant_weights_launch(W, ldw, N, K, W4, wexp, S(stream));
}
int vt_mx4_quant_lo(const uint16_t* lo, int ld, int M, int K, uint8_t* A4, uint8_t* aexp, void* stream) {
  return vt_mx4_quant_lo_launch(lo, ld, M, K, A4, aexp, S(stream));
}
int vt_rmsnorm_mx(const float* x, const int* idx, const float* w, uint16_t* y, uint8_t* A4, uint8_t* aexp, int rows, int D, float eps,
                  void* stream) {
  return vt_rmsnorm_mx_launch(x, idx, w, y, A4, aexp, rows, D, eps, S(stream));
}
int vt_gemm_mx(const uint16_t* A, int lda, const uint8_t* A4, const uint8_t* aexp, const uint16_t* W, int ldw, const uint8_t* W4,
               const uint8_t* wexp, void* C, int ldc, const float* bias, int M, int N, int K, int epi, void* stream) {
  return vt_gemm_mx_launch(A, lda, A4, aexp, W, ldw, W4, wexp, C, ldc, bias, M, N, K, epi, 1, 0, nullptr, nullptr, S(stream));
}

int vt_gemm_mx_swiglu(const uint16_t* A, int lda, const uint8_t* A4, const uint8_t* aexp, const uint16_t* W, int ldw, const uint8_t* W4,
                      const uint8_t* wexp, uint16_t* C, int ldc, uint8_t* out4, uint8_t* oexp, int M, int N, int K, void* stream) {
  return vt_gemm_mx_launch(A, lda, A4, aexp, W, ldw, W4, wexp, C, ldc, nullptr, M, N, K, VT_EPI_SWIGLU_MX, 1, 0, out4, oexp, S(stream));
}
int vt_gemm_mx_gelu(const uint16_t* A, int lda, const uint8_t* A4, const uint8_t* aexp, const uint16_t* W, int ldw, const uint8_t* W4,
                    const uint8_t* wexp, const float* bias, uint16_t* C, int ldc, uint8_t* out4, uint8_t* oexp, int M, int N, int K, int quick,
                    void* stream) {
  return vt_gemm_mx_launch(A, lda, A4, aexp, W, ldw, W4, wexp, C, ldc, bias, M, N, K, quick ? VT_EPI_QGELU_MX : VT_EPI_GELU_MX, 1, 0, out4, oexp,
                           S(stream));
}
int vt_layernorm_mx(const float* x, const float* gamma, const float* beta, uint16_t* y, uint8_t* A4, uint8_t* aexp, int rows, int D, float eps,
                    void* stream) {
  return vt_layernorm_mx_launch(x, gamma, beta, y, A4, aexp, rows, D, eps, S(stream));
}
int vt_gemm_mx_resid(const uint16_t* A, int lda, const uint8_t* A4, const uint8_t* aexp, const uint16_t* W, int ldw, const uint8_t* W4,
                     const uint8_t* wexp, float* C, int ldc, int M, int N, int K, float* partials, size_t partial_bytes, void* stream) {
  return vt_gemm_mx_resid_launch(A, lda, A4, aexp, W, ldw, W4, wexp, C, ldc, nullptr, M, N, K, partials, partial_bytes, S(stream));
}
int vt_flash_attn_mx(const uint16_t* Q, int ldq, const uint16_t* k_tiles, const uint16_t* vt_tiles, const int* tile_table,
                     const int* seq_desc, int nseq, int max_q_len, uint16_t* O, int ldo, uint8_t* O4, uint8_t* oexp, int heads, float scale,
                     void* stream) {
  VT_REQUIRE(O4 && oexp, "vt_flash_attn_mx: null pointer");
  return vt_flash_attn_launch(Q, ldq, k_tiles, vt_tiles, tile_table, (const VtAttnSeq*)seq_desc, nseq, max_q_len, O, ldo, heads, 128, 1, scale,
                              S(stream), O4, oexp);
}

int vt_gemm_bf16_resid_splitk(const uint16_t* A, int lda, const uint16_t* W, int ldw, float* C, int ldc, const float* bias,
                              int M, int N, int K, int ksplit, float* partials, size_t partial_bytes, void* stream) {
  return vt_gemm_resid_launch(A, lda, W, ldw, C, ldc, bias, M, N, K, ksplit, partials, partial_bytes, S(stream));
}

// ---- the folded RMSNorm of the 16-bit GEMMs, one launch at a time (unit parity tests) ----
int vt_gemm_bf16_norm(const uint16_t* A, int lda, const uint16_t* W, int ldw, void* C, int ldc, int M, int N, int K, int epi,
                      const float* in_partials, int in_n, float inv_dim, float eps, const float* out_w, uint16_t* out_xw, int ld_xw,
                      float* out_partials, void* stream) {
  VtGemmNormFuse nf;
  nf.in_partials = in_partials;
  nf.in_n = in_n;
  nf.inv_dim = inv_dim;
  nf.eps = eps;
  nf.out_w = out_w;
  nf.out_xw = out_xw;
  nf.ld_xw = ld_xw;
  nf.out_partials = out_partials;
  return vt_gemm_skinny_norm_launch(A, lda, W, ldw, C, ldc, M, N, K, epi, nf, S(stream));
}

int vt_gemm_bf16_resid_norm(const uint16_t* A, int lda, const uint16_t* W, int ldw, float* C, int ldc, const float* bias, int M, int N, int K,
                            int cfg, int ksplit, float* workspace, size_t workspace_bytes, const float* out_w, uint16_t* out_xw, int ld_xw,
                            float* out_partials, int out_np, int out_ldp, void* stream) {
  VT_REQUIRE(out_w && out_xw && out_partials, "vt_gemm_bf16_resid_norm: the producer needs out_w, out_xw and out_partials");
  VtGemmNormFuse nf;
  nf.out_w = out_w;
  nf.out_xw = out_xw;
  nf.ld_xw = ld_xw;
  nf.out_partials = out_partials;
  nf.out_np = out_np;
  nf.out_ldp = out_ldp;
  if (ksplit < 0) return vt_gemm_launch(A, lda, W, ldw, C, ldc, bias, M, N, K, VT_EPI_F32_RESID, cfg, S(stream), &nf);
  return vt_gemm_resid_launch(A, lda, W, ldw, C, ldc, bias, M, N, K, ksplit, workspace, workspace_bytes, S(stream), &nf);
}

int vt_rowscale_finalize(const float* partials, int np, int ldp, int rows, float inv_dim, float eps, float* out, void* stream) {
  return vt_rowscale_finalize_launch(partials, np, ldp, rows, inv_dim, eps, out, S(stream));
}

int vt_attn_decode_fused(const uint16_t* qkv, int ldqkv, int q_col0, int k_col0, int v_col0, uint16_t* k_tiles,
                         uint16_t* vt_tiles, const int* tile_table, const int* seq_desc, int nseq, uint16_t* O, int ldo,
                         int heads, int head_dim, float scale, const float* rope_cos, const float* rope_sin,
                         const int* positions, void* stream) {
  return vt_attn_decode_fused_launch(qkv, ldqkv, q_col0, k_col0, v_col0, k_tiles, vt_tiles, tile_table,
                                     (const VtAttnSeq*)seq_desc, nseq, O, ldo, heads, head_dim, scale, rope_cos, rope_sin,
                                     positions, S(stream));
}

// ---- FP8 KV cache (vt_kv8.hip) ----
int vt_kv8_quant(const uint16_t* k_tiles, const uint16_t* vt_tiles, const int* src_table, uint8_t* k8, uint8_t* vt8,
                 const int* dst_table, int ntiles, int heads, int head_dim, void* stream) {
  return vt_kv8_quant_launch(k_tiles, vt_tiles, src_table, k8, vt8, dst_table, ntiles, heads, head_dim, S(stream));
}
int vt_kv8_dequant(const uint8_t* k8, const uint8_t* vt8, const int* src_table, uint16_t* k_tiles, uint16_t* vt_tiles,
                   const int* dst_table, int ntiles, int heads, int head_dim, void* stream) {
  return vt_kv8_dequant_launch(k8, vt8, src_table, k_tiles, vt_tiles, dst_table, ntiles, heads, head_dim, S(stream));
}
int vt_attn_decode_kv8(const uint16_t* Q, int ldq, const uint8_t* k8, const uint8_t* vt8, const int* tile_table,
                       const int* seq_desc, int nseq, uint16_t* O, int ldo, int heads, int head_dim, float scale,
                       int max_kv_len, void* scratch, size_t scratch_bytes, void* stream) {
  return vt_attn_decode_kv8_launch(Q, ldq, k8, vt8, tile_table, (const VtAttnSeq*)seq_desc, nseq, O, ldo, heads, head_dim, scale,
                                   max_kv_len, (float*)scratch, scratch_bytes, S(stream));
}
int vt_attn_decode_fused_kv8(const uint16_t* qkv, int ldqkv, int q_col0, int k_col0, int v_col0, uint8_t* k8, uint8_t* vt8,
                             const int* tile_table, const int* seq_desc, int nseq, uint16_t* O, int ldo, int heads, int head_dim,
                             float scale, const float* rope_cos, const float* rope_sin, const int* positions, void* stream) {
  return vt_attn_decode_fused_kv8_launch(qkv, ldqkv, q_col0, k_col0, v_col0, k8, vt8, tile_table, (const VtAttnSeq*)seq_desc, nseq, O,
                                         ldo, heads, head_dim, scale, rope_cos, rope_sin, positions, S(stream));
}

int vt_kv_tiles(uint16_t* qkv, int ldqkv, int q_col0, int k_col0, int v_col0, uint16_t* k_tiles, uint16_t* vt_tiles,
                const int* tile_table, const int* seq_desc, int nseq, int max_new_tiles, int heads, int head_dim,
                const float* rope_cos, const float* rope_sin, const int* positions, void* stream) {
  return vt_kv_tiles_launch(qkv, ldqkv, q_col0, k_col0, v_col0, k_tiles, vt_tiles, tile_table,
                            (const VtAttnSeq*)seq_desc, nseq, max_new_tiles, heads, head_dim, rope_cos, rope_sin,
                            positions, S(stream));
}

int vt_attn_tail_desc(const int* seq_desc, int nseq, const int* logit_rows, int n, int* out, void* stream) {
  return vt_attn_tail_desc_launch((const VtAttnSeq*)seq_desc, nseq, logit_rows, n, (VtAttnSeq*)out, S(stream));
}

int vt_attn_temporal(const uint16_t* qkv, uint16_t* out, int B, int T, int N, int heads, void* stream) {
  return vt_attn_temporal_launch(qkv, out, B, T, N, heads, S(stream));
}

int vt_attn_temporal_f32(const float* qkv, int ld, uint16_t* out, uint16_t* out_lo, int B, int T, int N, int heads, void* stream) {
  return vt_attn_temporal_f32_launch(qkv, ld, out, out_lo, B, T, N, heads, S(stream));
}

int vt_vit_embed(const float* patch_out, const float* cls, const float* pos, const float* g, const float* b, float* x, int F, int G2,
                 int D, float eps, void* stream) {
  return vt_vit_embed_launch(patch_out, cls, pos, g, b, x, F, G2, D, eps, S(stream));
}

int vt_region_pool(const uint16_t* feats, const int* slices, int B, int G, int image_size, int D, uint16_t* pooled, int* cell_mask,
                   int* cell_count, const float* coords, const uint16_t* loc_w0, const float* loc_b0, int loc_n, uint16_t* loc_out,
                   int ld_loc, void* stream) {
  return vt_region_pool_launch(feats, slices, B, G, image_size, D, pooled, cell_mask, cell_count, coords, loc_w0, loc_b0, loc_n, loc_out,
                               ld_loc, S(stream));
}

int vt_im2col(const void* pixels, int pix_dtype, uint16_t* patches, int B, int T, int H, int W, int P, int k_pad,
              int video_layout, void* stream) {
  return vt_im2col_launch(pixels, pix_dtype, patches, B, T, H, W, P, k_pad, video_layout, S(stream));
}

int vt_embed_splice(const uint16_t* tok_table, int vocab, const uint16_t* vis, int vis_rows, const uint16_t* reg, int reg_rows,
                    const int* plan, int rows, int H, uint16_t* out, void* stream) {
  return vt_embed_splice_launch(tok_table, vocab, vis, vis_rows, reg, reg_rows, plan, rows, H, out, S(stream));
}

int vt_argmax(const float* logits, int rows, int V, int ldl, int* out_ids, void* stream) {
  return vt_argmax_launch(logits, rows, V, ldl, out_ids, S(stream));
}

int vt_decode_feed(const uint16_t* tok_table, int H, int vocab, const int* next_ids, int* finished, const int* eos_ids, int n_eos,
                   int pad_id, int* tokens_out, uint16_t* x, int* seq_desc, int* positions, int nseq, void* stream) {
  return vt_decode_feed_launch(tok_table, H, vocab, next_ids, finished, eos_ids, n_eos, pad_id, tokens_out, x, seq_desc, positions,
                               nseq, S(stream));
}

int vt_preprocess(const void* src, int src_u8, int hwc, int F, int H, int W, int bicubic, int S, const float* mean,
                  const float* std, int flip, void* dst, int dst_dtype, long dst_stride_c, long dst_stride_f, void* stream) {
  return vt_preprocess_launch(src, src_u8, hwc, F, H, W, bicubic, S, mean, std, flip, dst, dst_dtype, dst_stride_c, dst_stride_f,
                              S_(stream));
}

int vt_cross_entropy(const float* logits, int rows, int V, int ldl, const int* labels, int ignore_index, float* row_nll,
                     float* loss, void* stream) {
  return vt_cross_entropy_launch(logits, rows, V, ldl, labels, ignore_index, row_nll, loss, S(stream));
}

int vt_sample_top_p(const float* logits, int rows, int V, int ldl, float temperature, int top_k, float top_p, uint64_t seed,
                    uint64_t step, int* out_ids, int* kept_count, void* stream) {
  return vt_sample_top_p_launch(logits, rows, V, ldl, temperature, top_k, top_p, seed, step, out_ids, kept_count, S(stream));
}

int vt_sample_rows(const float* logits, int rows, int V, int ldl, const vt_sample_row* params, int* out_ids, int* kept_count,
                   float* logprob, void* stream) {
  return vt_sample_rows_launch(logits, rows, V, ldl, params, nullptr, out_ids, kept_count, logprob, S(stream));
}

int vt_sample_rows_allow(const float* logits, int rows, int V, int ldl, const vt_sample_row* params, const uint32_t* const* allow,
                         int* out_ids, int* kept_count, float* logprob, void* stream) {
  return vt_sample_rows_launch(logits, rows, V, ldl, params, allow, out_ids, kept_count, logprob, S(stream));
}

int vt_sample_rows_adj(const float* logits, int rows, int V, int ldl, const vt_sample_row* params, const uint32_t* const* allow,
                       const float* const* adjust, int* out_ids, int* kept_count, float* logprob, void* stream) {
  return vt_sample_rows_launch(logits, rows, V, ldl, params, allow, out_ids, kept_count, logprob, S(stream), adjust);
}

int vt_sample_rows_trunc(const float* logits, int rows, int V, int ldl, const vt_sample_row* params, const uint32_t* const* allow,
                         const float* const* adjust, const vt_trunc_row* trunc, int* out_ids, int* kept_count, float* logprob,
                         void* stream) {
  return vt_sample_rows_launch(logits, rows, V, ldl, params, allow, out_ids, kept_count, logprob, S(stream), adjust, trunc);
}

int vt_sample_rows_wm(const float* logits, int rows, int V, int ldl, const vt_sample_row* params, const uint32_t* const* allow,
                      const float* const* adjust, const vt_trunc_row* trunc, const vt_wm_row* wm, int* out_ids, int* kept_count,
                      float* logprob, void* stream) {
  return vt_sample_rows_launch(logits, rows, V, ldl, params, allow, out_ids, kept_count, logprob, S(stream), adjust, trunc, wm);
}

size_t vt_wm_cell_words(int history_size) { return 12 + (size_t)(history_size > 0 ? history_size : 0); }

int vt_sample_rows_miro(const float* logits, int rows, int V, int ldl, const vt_sample_row* params, const uint32_t* const* allow,
                        const float* const* adjust, const vt_trunc_row* trunc, const vt_miro_row* miro, int* out_ids, int* kept_count,
                        float* logprob, void* stream) {
  return vt_sample_rows_launch(logits, rows, V, ldl, params, allow, out_ids, kept_count, logprob, S(stream), adjust, trunc, nullptr, miro);
}

// ---- beam search (vt_beam.hip) ----------------------------------------------------------------------------------------
size_t vt_beam_step_scratch_bytes(int groups, int beams_in, int n_out) { return vt_beam_step_scratch_bytes_impl(groups, beams_in, n_out); }

int vt_beam_step(const float* logits, int ldl, int V, int groups, int beams_in, const float* beam_scores, int n_out, float* out_scores,
                 int* out_tokens, int* out_beams, void* scratch, size_t scratch_bytes, void* stream) {
  return vt_beam_step_launch(logits, ldl, V, groups, beams_in, beam_scores, n_out, out_scores, out_tokens, out_beams, scratch,
                             scratch_bytes, S(stream));
}

// ---- log-probabilities of logit rows (vt_logprob.hip) -----------------------------------------------------------------
int vt_logprob_rows(const float* logits, int rows, int V, int ldl, const int* target, int n_top, float* lse, float* target_lp,
                    int* target_rank, int* top_ids, float* top_lp, void* stream) {
  return vt_logprob_rows_launch(logits, rows, V, ldl, target, n_top, lse, target_lp, target_rank, top_ids, top_lp, S(stream));
}

int vt_kv_copy_pages(void* k, void* vt, int num_layers, int num_pages, size_t page_bytes, const int* src_pages, const int* dst_pages,
                     int n, void* stream) {
  return vt_kv_copy_pages_launch(k, vt, num_layers, num_pages, page_bytes, src_pages, dst_pages, n, S(stream));
}

// ---- history-dependent bans (vt_ban.hip) ------------------------------------------------------------------------------
int vt_ban_rows(const vt_ban_row* rows, int n_rows, int V, void* stream) { return vt_ban_rows_launch(rows, n_rows, V, S(stream)); }
int vt_bias_rows(const vt_bias_row* rows, int n_rows, int V, void* stream) { return vt_bias_rows_launch(rows, n_rows, V, S(stream)); }
// ---- token automata (vt_fsm.hip) -----------------------------------------------------------------------------------------
int vt_fsm_rows(const vt_fsm_row* rows, int n_rows, int V, void* stream) { return vt_fsm_rows_launch(rows, n_rows, V, S(stream)); }
int vt_cfg_rows(const vt_cfg_row* rows, int n_rows, int V, void* stream) { return vt_cfg_rows_launch(rows, n_rows, V, S(stream)); }
// ---- DoLa (vt_dola.hip) --------------------------------------------------------------------------------------------------
int vt_dola_rows(const vt_dola_row* rows, int n_rows, int V, void* stream) { return vt_dola_rows_launch(rows, n_rows, V, S(stream)); }
// ---- contrastive search (vt_contrast.hip) ------------------------------------------------------------------------------------
int vt_unit_rows(const float* x, int ldx, const float* w, uint16_t* out, int ldo, int rows, int H, void* stream) {
  return vt_unit_rows_launch(x, ldx, w, out, ldo, rows, H, S(stream));
}
int vt_contrast_rows(const vt_contrast_row* rows, int n_groups, const uint16_t* cand, int n_cand, int ld, int H, void* workspace,
                     size_t workspace_bytes, void* stream) {
  return vt_contrast_rows_launch(rows, n_groups, cand, n_cand, ld, H, workspace, workspace_bytes, S(stream));
}

// ---- mm_projector ---------------------------------------------------------------------------------------------------
size_t vt_projector_workspace_bytes(int M, int Dh) { return align_up((size_t)M * Dh * 2, 256) + 256; }

int vt_projector_forward(const uint16_t* x, int M, int Din, const uint16_t* w1, const float* b1, int Dh,
                         const uint16_t* w2, const float* b2, int Dout, uint16_t* out, void* workspace,
                         size_t workspace_bytes, void* stream) {
  VT_REQUIRE(x && w1 && out && M > 0, "vt_projector_forward: null pointer / empty input");
  hipStream_t s = S(stream);
  if (!w2) {  // 'linear' projector
    return vt_gemm_launch(x, Din, w1, Din, out, Dh, b1, M, Dh, Din, VT_EPI_BF16, VT_GEMM_CFG_AUTO, s);
  }
  Carver ws(workspace, workspace_bytes);
  bf16_t* h = (bf16_t*)ws.take((size_t)M * Dh * 2);
  if (!workspace || !ws.ok()) {
    vt_set_error("vt_projector_forward: workspace too small (%zu < %zu)", workspace_bytes, ws.off);
    return VT_ERR_WORKSPACE;
  }
  VT_TRY(vt_gemm_launch(x, Din, w1, Din, h, Dh, b1, M, Dh, Din, VT_EPI_BF16_GELU, VT_GEMM_CFG_AUTO, s));
  VT_TRY(vt_gemm_launch(h, Dh, w2, Dh, out, Dout, b2, M, Dout, Dh, VT_EPI_BF16, VT_GEMM_CFG_AUTO, s));
  return VT_OK;
}

// precise level 2: the mlp2x_gelu projector on operand pairs -- x (+ x_lo) in, out (+ out_lo) out; both Linear layers as two launches
// accumulating in fp32, the GELU as an fp32 -> pair pass; the output leaves as a pair so that the decoder's residual stream starts from the
// fp32 value (vt_llama_model.embeds_lo)
size_t vt_projector_precise_workspace_bytes(int M, int Dh, int Dout) {
  return align_up((size_t)M * Dh * 4, 256) + 2 * align_up((size_t)M * Dh * 2, 256) + align_up((size_t)M * Dout * 4, 256) + 256;
}

int vt_projector_forward_precise(const uint16_t* x, const uint16_t* x_lo, int M, int Din, const uint16_t* w1, const float* b1, int Dh,
                                 const uint16_t* w2, const float* b2, int Dout, uint16_t* out, uint16_t* out_lo, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  VT_REQUIRE(x && x_lo && w1 && w2 && out && out_lo && M > 0, "vt_projector_forward_precise: null pointer / empty input (mlp2x_gelu only)");
  hipStream_t s = S(stream);
  Carver ws(workspace, workspace_bytes);
  float* h32 = (float*)ws.take((size_t)M * Dh * 4);
  bf16_t* h = (bf16_t*)ws.take((size_t)M * Dh * 2);
  bf16_t* hlo = (bf16_t*)ws.take((size_t)M * Dh * 2);
  float* o32 = (float*)ws.take((size_t)M * Dout * 4);
  if (!workspace || !ws.ok()) {
    vt_set_error("vt_projector_forward_precise: workspace too small (%zu < %zu)", workspace_bytes, ws.off);
    return VT_ERR_WORKSPACE;
  }
  const int AUTO = VT_GEMM_CFG_AUTO;
  VT_TRY(vt_gemm_launch(x, Din, w1, Din, h32, Dh, b1, M, Dh, Din, VT_EPI_F32, AUTO, s));
  VT_TRY(vt_gemm_resid_launch(x_lo, Din, w1, Din, h32, Dh, nullptr, M, Dh, Din, 0, nullptr, 0, s));
  VT_TRY(vt_act_pair_launch(h32, Dh, h, hlo, M, Dh, 0, s));
  VT_TRY(vt_gemm_launch(h, Dh, w2, Dh, o32, Dout, b2, M, Dout, Dh, VT_EPI_F32, AUTO, s));
  VT_TRY(vt_gemm_resid_launch(hlo, Dh, w2, Dh, o32, Dout, nullptr, M, Dout, Dh, 0, nullptr, 0, s));
  VT_TRY(vt_f32_to_pair_launch(o32, out, out_lo, (size_t)M, 0, Dout, s));
  return VT_OK;
}

// ---- region_extractor ------------------------------------------------------------------------------------------------
size_t vt_region_workspace_bytes(int B, int in_dim, int out_dim) {
  size_t n = 0;
  n += align_up((size_t)B * in_dim * 2, 256);                       // pooled
  n += align_up((size_t)B * out_dim * 2, 256);                      // h1
  n += align_up((size_t)B * (out_dim + out_dim / 2) * 2, 256);      // [ h2 | location hidden ]
  return n + 1024;
}

int vt_region_forward(const vt_region_weights* w, const uint16_t* feats, const int* slices, const float* coords,
                      int B, int G, int image_size, uint16_t* out, int* cell_mask, int* cell_count, void* workspace,
                      size_t workspace_bytes, void* stream) {
  VT_REQUIRE(w && feats && slices && coords && out, "vt_region_forward: null pointer");
  VT_REQUIRE(B > 0 && B <= 16, "vt_region_forward: B=%d (1..16 boxes per call)", B);
  hipStream_t s = S(stream);
  const int D = w->in_dim, H = w->out_dim;
  VT_REQUIRE(D % 64 == 0 && H % 128 == 0, "vt_region_forward: in_dim %% 64 and out_dim %% 128 must be 0 (in=%d out=%d)", D, H);
  VT_REQUIRE(w->mlp_w[0] && w->mlp_w[1] && w->loc_w0 && w->loc_b0 && w->final_w, "vt_region_forward: weight pointer missing");
  const int KC = H + H / 2;
  Carver ws(workspace, workspace_bytes);
  bf16_t* pooled = (bf16_t*)ws.take((size_t)B * D * 2);
  bf16_t* h1 = (bf16_t*)ws.take((size_t)B * H * 2);
  bf16_t* cat = (bf16_t*)ws.take((size_t)B * KC * 2);
  if (!workspace || !ws.ok()) {
    vt_set_error("vt_region_forward: workspace too small (%zu < %zu)", workspace_bytes, ws.off);
    return VT_ERR_WORKSPACE;
  }
  // 1: cell mask + count + masked mean + LocationEncoder layer 0 (into the right part of `cat`)
  VT_TRY(vt_region_pool_launch(feats, slices, B, G, image_size, D, pooled, cell_mask, cell_count, coords, w->loc_w0, w->loc_b0,
                               H / 2, cat + H, KC, s));
  // 2-4: weight-streaming GEMMs; the last contracts [h2 | loc hidden] with [W2 | Wloc1]: MLP output + location embedding
  const int SK = VT_GEMM_CFG_SKINNY;
  VT_TRY(vt_gemm_launch(pooled, D, w->mlp_w[0], D, h1, H, w->mlp_b[0], B, H, D, VT_EPI_BF16_RELU, SK, s));
  VT_TRY(vt_gemm_launch(h1, H, w->mlp_w[1], H, cat, KC, w->mlp_b[1], B, H, H, VT_EPI_BF16_RELU, SK, s));
  VT_TRY(vt_gemm_launch(cat, KC, w->final_w, KC, out, H, w->final_b, B, H, KC, VT_EPI_BF16, SK, s));
  return VT_OK;
}

// ---- ViT tower ---------------------------------------------------------------------------------------------------------
namespace {
struct VitWs {
  float* x;
  float* patch_out;
  bf16_t *y, *qkv, *att, *h, *patches, *kt, *vt;
  int *seq_desc, *tile_table;
  float* splitk;   // split-K partial products (single images: the N = 1024 projections cover a fraction of the chip)
  size_t splitk_bytes;
  // precise level 2: the MLP's two operands as pairs (low halves) and fc1's fp32 output; the attention paths' fp32 q | k | v, the low
  // halves of q, of the keys (one workspace tile per page) and of the attention output
  bf16_t *ylo, *hlo, *qlo, *klo, *attlo;
  float *h32, *qkv32;
  // precise level 1 with the layers' MX-FP4 weight images: the MLP's two A operands as 16-bit value + 4-bit image of the remainder
  uint8_t *y4, *yexp, *h4, *hexp;
  size_t total;
};
VitWs vit_carve(const vt_vit_model* m, int B, int T, void* p, size_t n) {
  const int G = m->image_size / m->patch, G2 = G * G, N = G2 + 1, F = B * T, R = F * N;
  const int D = m->hidden, I = m->intermediate;
  const int ntiles = cdiv(N, 64);
  Carver ws(p, n);
  VitWs w;
  w.x = (float*)ws.take((size_t)R * D * 4);
  w.patch_out = (float*)ws.take((size_t)F * G2 * D * 4);
  w.y = (bf16_t*)ws.take((size_t)R * D * 2);
  w.qkv = (bf16_t*)ws.take((size_t)R * 3 * D * 2);
  w.att = (bf16_t*)ws.take((size_t)R * D * 2);
  w.h = (bf16_t*)ws.take((size_t)R * I * 2);
  w.patches = (bf16_t*)ws.take((size_t)F * G2 * m->k_pad * 2);
  w.kt = (bf16_t*)ws.take((size_t)F * ntiles * 64 * D * 2);
  w.vt = (bf16_t*)ws.take((size_t)F * ntiles * 64 * D * 2);
  w.seq_desc = (int*)ws.take((size_t)F * 4 * 4);
  w.tile_table = (int*)ws.take((size_t)F * ntiles * 4);
  w.splitk_bytes = (size_t)8 * R * D * 4 <= ((size_t)64 << 20) ? (size_t)8 * R * D * 4 : 0;   // only worth it for a few frames
  if (m->precise == 1 && m->num_layers > 0 && m->layers[0].w14) {
    // level 1 on the MX pipe: fc2's grid of 256 x 256 tiles covers a fraction of the chip (one clip: 19 x 4 = 76 tiles) and runs as K ranges
    // (vt_gemm_mx_resid_launch): room for its fp32 partial slabs
    const int tiles = cdiv(R, 256) * cdiv(D, 256);
    const int ks = tiles * 2 <= 256 ? std::min(8, 256 / tiles) : 0;
    w.splitk_bytes = std::max(w.splitk_bytes, (size_t)ks * R * D * 4);
  }
  w.splitk = w.splitk_bytes ? (float*)ws.take(w.splitk_bytes) : nullptr;
  w.ylo = w.hlo = w.qlo = w.klo = w.attlo = nullptr;
  w.h32 = w.qkv32 = nullptr;
  w.y4 = w.yexp = w.h4 = w.hexp = nullptr;
  if (m->precise >= 1) {
    w.ylo = (bf16_t*)ws.take((size_t)R * D * 2);
    w.hlo = (bf16_t*)ws.take((size_t)R * I * 2);
    w.h32 = (float*)ws.take((size_t)R * I * 4);
  }
  if (m->precise == 1 && m->num_layers > 0 && m->layers[0].w14) {
    w.y4 = (uint8_t*)ws.take((size_t)R * (D / 2));
    w.yexp = (uint8_t*)ws.take(vt_mx4_aexp_bytes(R, D));
    w.h4 = (uint8_t*)ws.take((size_t)R * (I / 2));
    w.hexp = (uint8_t*)ws.take(vt_mx4_aexp_bytes(R, I));
  }
  if (m->precise >= 2) {
    w.qkv32 = (float*)ws.take((size_t)R * 3 * D * 4);
    w.qlo = (bf16_t*)ws.take((size_t)R * D * 2);
    w.klo = (bf16_t*)ws.take((size_t)F * ntiles * 64 * D * 2);
    w.attlo = (bf16_t*)ws.take((size_t)R * D * 2);
  }
  w.total = ws.off + 256;
  return w;
}
}  // namespace

size_t vt_vit_workspace_bytes(const vt_vit_model* m, int B, int T) {
  if (!m) return 0;
  return vit_carve(m, B, T, nullptr, 0).total;
}

int vt_vit_forward(const vt_vit_model* m, const void* pixels, int pix_dtype, int B, int T, int video_layout,
                   uint16_t* out_feats, float* out_hidden, void* workspace, size_t workspace_bytes, void* stream) {
  VT_REQUIRE(m && pixels && out_feats && workspace, "vt_vit_forward: null pointer");
  VT_REQUIRE(B > 0 && T > 0, "vt_vit_forward: empty batch");
  VT_REQUIRE(m->hidden == m->heads * 64, "vt_vit_forward: head_dim must be 64 (hidden=%d heads=%d)", m->hidden, m->heads);
  VT_REQUIRE(m->image_size % m->patch == 0, "vt_vit_forward: image_size %% patch != 0");
  VT_REQUIRE(m->k_pad % 64 == 0 && m->k_pad >= 3 * m->patch * m->patch, "vt_vit_forward: bad k_pad %d", m->k_pad);
  VT_REQUIRE(m->hidden % 64 == 0 && m->intermediate % 64 == 0, "vt_vit_forward: hidden/intermediate must be multiples of 64");
  if (m->add_time_attn) VT_REQUIRE(T == m->num_frames && T <= 8, "vt_vit_forward: video tower built for %d frames, got T=%d", m->num_frames, T);
  hipStream_t s = S(stream);
  VitWs w = vit_carve(m, B, T, workspace, workspace_bytes);
  if (w.total > workspace_bytes) {
    vt_set_error("vt_vit_forward: workspace too small (%zu < %zu)", workspace_bytes, w.total);
    return VT_ERR_WORKSPACE;
  }
  const int G = m->image_size / m->patch, G2 = G * G, N = G2 + 1, F = B * T, R = F * N;
  const int D = m->hidden, I = m->intermediate, heads = m->heads;
  const int AUTO = VT_GEMM_CFG_AUTO;
  const int act_epi = (m->act == VT_ACT_QUICK_GELU) ? VT_EPI_BF16_QGELU : VT_EPI_BF16_GELU;
  const bool precise = m->precise >= 2 && w.qkv32 != nullptr;

  // embeddings: patch GEMM (fp32 out) -> + CLS / position -> pre-LayerNorm -> fp32 residual stream x
  VT_TRY(vt_im2col_launch(pixels, pix_dtype, w.patches, B, T, m->image_size, m->image_size, m->patch, m->k_pad, video_layout, s));
  VT_TRY(vt_gemm_launch(w.patches, m->k_pad, m->w_patch, m->k_pad, w.patch_out, D, nullptr, F * G2, D, m->k_pad, VT_EPI_F32, AUTO, s));
  VT_TRY(vt_vit_embed_launch(w.patch_out, m->cls, m->pos, m->pre_ln_g, m->pre_ln_b, w.x, F, G2, D, m->ln_eps, s));
  VT_TRY(vt_vit_attn_meta_launch(w.seq_desc, w.tile_table, F, N, s));

  for (int l = 0; l < m->num_layers; ++l) {
    const vt_vit_layer& L = m->layers[l];
    if (m->add_time_attn && precise) {
      // precise level 2: the norm output as a pair, q | k | v into fp32 (two launches), the T x T attention in fp32, its output as a pair
      VT_TRY(vt_layernorm_launch(w.x, (T != 1) ? L.t_embed : nullptr, T, N, L.t_ln_g, L.t_ln_b, w.y, R, D, m->ln_eps, s));   // (adds the embedding)
      VT_TRY(vt_layernorm_hilo_launch(w.x, L.t_ln_g, L.t_ln_b, w.y, w.ylo, R, D, m->ln_eps, s));
      VT_TRY(vt_gemm_launch(w.y, D, L.t_wqkv, D, w.qkv32, 3 * D, L.t_bqkv, R, 3 * D, D, VT_EPI_F32, AUTO, s));
      VT_TRY(vt_gemm_resid_launch(w.ylo, D, L.t_wqkv, D, w.qkv32, 3 * D, nullptr, R, 3 * D, D, 0, w.splitk, w.splitk_bytes, s));
      VT_TRY(vt_attn_temporal_f32_launch(w.qkv32, 3 * D, w.att, w.attlo, B, T, N, heads, s));
      VT_TRY(vt_gemm_resid_launch(w.att, D, L.t_wo, D, w.x, D, L.t_bo, R, D, D, 0, w.splitk, w.splitk_bytes, s));
      VT_TRY(vt_gemm_resid_launch(w.attlo, D, L.t_wo, D, w.x, D, nullptr, R, D, D, 0, w.splitk, w.splitk_bytes, s));
      if (L.t_w1) {   // the image tower's temporal MLP, operands as pairs like the spatial MLP below
        VT_REQUIRE(L.t_ln2_g && L.t_ln2_b && L.t_w2 && L.t_b1 && L.t_b2, "vt_vit_forward: layer %d has a temporal MLP with missing tensors", l);
        VT_TRY(vt_layernorm_hilo_launch(w.x, L.t_ln2_g, L.t_ln2_b, w.y, w.ylo, R, D, m->ln_eps, s));
        VT_TRY(vt_gemm_launch(w.y, D, L.t_w1, D, w.h32, I, L.t_b1, R, I, D, VT_EPI_F32, AUTO, s));
        VT_TRY(vt_gemm_resid_launch(w.ylo, D, L.t_w1, D, w.h32, I, nullptr, R, I, D, 0, w.splitk, w.splitk_bytes, s));
        VT_TRY(vt_act_pair_launch(w.h32, I, w.h, w.hlo, R, I, m->act == VT_ACT_QUICK_GELU ? 1 : 0, s));
        VT_TRY(vt_gemm_resid_launch(w.h, I, L.t_w2, I, w.x, D, L.t_b2, R, D, I, 0, w.splitk, w.splitk_bytes, s));
        VT_TRY(vt_gemm_resid_launch(w.hlo, I, L.t_w2, I, w.x, D, nullptr, R, D, I, 0, w.splitk, w.splitk_bytes, s));
      }
    } else if (m->add_time_attn) {
      // x += temporal_embedding[t]; y = temporal_layer_norm1(x); temporal attention over T; x += out_proj
      VT_TRY(vt_layernorm_launch(w.x, (T != 1) ? L.t_embed : nullptr, T, N, L.t_ln_g, L.t_ln_b, w.y, R, D, m->ln_eps, s));
      VT_TRY(vt_gemm_launch(w.y, D, L.t_wqkv, D, w.qkv, 3 * D, L.t_bqkv, R, 3 * D, D, VT_EPI_BF16, AUTO, s));
      VT_TRY(vt_attn_temporal_launch(w.qkv, w.att, B, T, N, heads, s));
      VT_TRY(vt_gemm_launch(w.att, D, L.t_wo, D, w.x, D, L.t_bo, R, D, D, VT_EPI_F32_RESID, AUTO, s));
      if (L.t_w1 && m->precise >= 1) {   // (precise level 1: the temporal MLP's operands as pairs, like the spatial MLP below)
        VT_REQUIRE(L.t_ln2_g && L.t_ln2_b && L.t_w2 && L.t_b1 && L.t_b2, "vt_vit_forward: layer %d has a temporal MLP with missing tensors", l);
        VT_TRY(vt_layernorm_hilo_launch(w.x, L.t_ln2_g, L.t_ln2_b, w.y, w.ylo, R, D, m->ln_eps, s));
        VT_TRY(vt_gemm_launch(w.y, D, L.t_w1, D, w.h32, I, L.t_b1, R, I, D, VT_EPI_F32, AUTO, s));
        VT_TRY(vt_gemm_resid_launch(w.ylo, D, L.t_w1, D, w.h32, I, nullptr, R, I, D, 0, w.splitk, w.splitk_bytes, s));
        VT_TRY(vt_act_pair_launch(w.h32, I, w.h, w.hlo, R, I, m->act == VT_ACT_QUICK_GELU ? 1 : 0, s));
        VT_TRY(vt_gemm_resid_launch(w.h, I, L.t_w2, I, w.x, D, L.t_b2, R, D, I, 0, w.splitk, w.splitk_bytes, s));
        VT_TRY(vt_gemm_resid_launch(w.hlo, I, L.t_w2, I, w.x, D, nullptr, R, D, I, 0, w.splitk, w.splitk_bytes, s));
      } else if (L.t_w1) {   // image tower's add_time_attn variant: x += temporal_mlp(temporal_layer_norm2(x)) (image/modeling_image.py:129-134)
        VT_REQUIRE(L.t_ln2_g && L.t_ln2_b && L.t_w2 && L.t_b1 && L.t_b2, "vt_vit_forward: layer %d has a temporal MLP with missing tensors", l);
        VT_TRY(vt_layernorm_launch(w.x, nullptr, 0, 0, L.t_ln2_g, L.t_ln2_b, w.y, R, D, m->ln_eps, s));
        VT_TRY(vt_gemm_launch(w.y, D, L.t_w1, D, w.h, I, L.t_b1, R, I, D, act_epi, AUTO, s));
        VT_TRY(vt_gemm_resid_launch(w.h, I, L.t_w2, I, w.x, D, L.t_b2, R, D, I, 0, w.splitk, w.splitk_bytes, s));
      }
    }
    // spatial attention
    if (precise) {
      // precise level 2: q and k as operand pairs through the scores (K_hi.(Q_hi + Q_lo)^T + K_lo.Q_hi^T), v from fp32 straight into the V^T
      // tiles' fp16, the attention output as a pair into out_proj -- the same kernels as the decoder's precise prefill, at head_dim 64
      VT_TRY(vt_layernorm_hilo_launch(w.x, L.ln1_g, L.ln1_b, w.y, w.ylo, R, D, m->ln_eps, s));
      VT_TRY(vt_gemm_launch(w.y, D, L.wqkv, D, w.qkv32, 3 * D, L.bqkv, R, 3 * D, D, VT_EPI_F32, AUTO, s));
      VT_TRY(vt_gemm_resid_launch(w.ylo, D, L.wqkv, D, w.qkv32, 3 * D, nullptr, R, 3 * D, D, 0, w.splitk, w.splitk_bytes, s));
      VT_TRY(vt_kv_tiles_precise_launch(w.qkv32, 3 * D, 1, w.qkv, 3 * D, 0, 2 * D, w.qlo, w.kt, w.vt, w.klo, w.tile_table, (const VtAttnSeq*)w.seq_desc,
                                        F, cdiv(N, 64), heads, 64, nullptr, nullptr, nullptr, s));
      VT_TRY(vt_flash_attn_precise_launch(w.qkv, 3 * D, w.qlo, D, w.kt, w.klo, cdiv(N, 64), w.vt, w.tile_table, (const VtAttnSeq*)w.seq_desc, F, N,
                                          w.att, D, w.attlo, heads, 64, 0, 1.0f, s));
      VT_TRY(vt_gemm_resid_launch(w.att, D, L.wo, D, w.x, D, L.bo, R, D, D, 0, w.splitk, w.splitk_bytes, s));
      VT_TRY(vt_gemm_resid_launch(w.attlo, D, L.wo, D, w.x, D, nullptr, R, D, D, 0, w.splitk, w.splitk_bytes, s));
    } else {
      VT_TRY(vt_layernorm_launch(w.x, nullptr, 0, 0, L.ln1_g, L.ln1_b, w.y, R, D, m->ln_eps, s));
      VT_TRY(vt_gemm_launch(w.y, D, L.wqkv, D, w.qkv, 3 * D, L.bqkv, R, 3 * D, D, VT_EPI_BF16, AUTO, s));
      VT_TRY(vt_kv_tiles_launch(w.qkv, 3 * D, 0, D, 2 * D, w.kt, w.vt, w.tile_table, (const VtAttnSeq*)w.seq_desc, F,
                                cdiv(N, 64), heads, 64, nullptr, nullptr, nullptr, s));
      VT_TRY(vt_flash_attn_launch(w.qkv, 3 * D, w.kt, w.vt, w.tile_table, (const VtAttnSeq*)w.seq_desc, F, N, w.att, D,
                                  heads, 64, 0, 1.0f, s));
      VT_TRY(vt_gemm_launch(w.att, D, L.wo, D, w.x, D, L.bo, R, D, D, VT_EPI_F32_RESID, AUTO, s));
    }
    // MLP
    if (m->precise == 1 && L.w14 && L.w1_e && L.w24 && L.w2_e && w.y4) {
      // precise level 1 with MX-FP4 weight images (the towers' share of the decoder's level 3): both MLP products as ONE launch each that adds
      // the 4-bit product of the A operand's rounding remainder -- LayerNorm and the activation epilogue write the remainder's image
      VT_TRY(vt_layernorm_mx_launch(w.x, L.ln2_g, L.ln2_b, w.y, w.y4, w.yexp, R, D, m->ln_eps, s));
      VT_TRY(vt_gemm_mx_launch(w.y, D, w.y4, w.yexp, L.w1, D, L.w14, L.w1_e, w.h, I, L.b1, R, I, D,
                               m->act == VT_ACT_QUICK_GELU ? VT_EPI_QGELU_MX : VT_EPI_GELU_MX, 1, 0, w.h4, w.hexp, s));
      VT_TRY(vt_gemm_mx_resid_launch(w.h, I, w.h4, w.hexp, L.w2, I, L.w24, L.w2_e, w.x, D, L.b2, R, D, I, w.splitk, w.splitk_bytes, s));
      continue;
    }
    if (m->precise >= 1) {
      // precise level 1 / 2 (layer_norm2 -> fc1 and GELU -> fc2 carry half of the tower's distance from fp32): both operands as
      // pairs, every product as two launches accumulating in fp32, the activation as its own fp32 -> pair pass
      VT_TRY(vt_layernorm_hilo_launch(w.x, L.ln2_g, L.ln2_b, w.y, w.ylo, R, D, m->ln_eps, s));
      VT_TRY(vt_gemm_launch(w.y, D, L.w1, D, w.h32, I, L.b1, R, I, D, VT_EPI_F32, AUTO, s));
      VT_TRY(vt_gemm_resid_launch(w.ylo, D, L.w1, D, w.h32, I, nullptr, R, I, D, 0, w.splitk, w.splitk_bytes, s));
      VT_TRY(vt_act_pair_launch(w.h32, I, w.h, w.hlo, R, I, m->act == VT_ACT_QUICK_GELU ? 1 : 0, s));
      VT_TRY(vt_gemm_resid_launch(w.h, I, L.w2, I, w.x, D, L.b2, R, D, I, 0, w.splitk, w.splitk_bytes, s));
      VT_TRY(vt_gemm_resid_launch(w.hlo, I, L.w2, I, w.x, D, nullptr, R, D, I, 0, w.splitk, w.splitk_bytes, s));
      continue;
    }
    VT_TRY(vt_layernorm_launch(w.x, nullptr, 0, 0, L.ln2_g, L.ln2_b, w.y, R, D, m->ln_eps, s));
    VT_TRY(vt_gemm_launch(w.y, D, L.w1, D, w.h, I, L.b1, R, I, D, act_epi, AUTO, s));
    VT_TRY(vt_gemm_resid_launch(w.h, I, L.w2, I, w.x, D, L.b2, R, D, I, 0, w.splitk, w.splitk_bytes, s));
  }
  if (m->precise >= 1 && m->out_feats_lo) {   // the patch tokens of the selected hidden state as a pair (the projector's operand)
    VT_TRY(vt_f32_to_pair_launch(w.x, out_feats, m->out_feats_lo, (size_t)F * G2, G2, D, s));
    if (out_hidden) VT_HIP(hipMemcpyAsync(out_hidden, w.x, (size_t)R * D * 4, hipMemcpyDeviceToDevice, s));
    return VT_OK;
  }
  VT_TRY(vt_drop_cls_launch(w.x, out_feats, F, G2, D, s));
  if (out_hidden) VT_HIP(hipMemcpyAsync(out_hidden, w.x, (size_t)R * D * 4, hipMemcpyDeviceToDevice, s));
  return VT_OK;
}

// ---- LLaMA decoder --------------------------------------------------------------------------------------------------------
namespace {
struct LlamaWs {
  float* x;
  bf16_t *y, *qkv, *att, *h, *yn;
  float *rs_a, *rs_b;   // folded-RMSNorm partial sums of squares (decode steps: [16][H/16]; rows > 64: rs_a = [rows][H/32])
  float* rstd;          // rows > 64: per-row factor of the folded RMSNorm (vt_rowscale_finalize_launch)
  float* splitk;        // fp32 partial products of the split-K residual GEMMs (prefills of 65..~2000 rows)
  size_t splitk_bytes;
  float* attn_scratch;
  size_t attn_scratch_bytes;
  int* row_slot;        // prefill: cache slot of every new row (fused QKV epilogue)
  // pruned last layer of a prefill (<= 16 logit rows): the logit rows as compact [n][.] buffers and their single-query descriptors
  VtAttnSeq* tail_seq;
  bf16_t *y_l, *q_l, *att_l, *h_l;
  float* x_l;
  // precise_qk prefills: the low half of the norm output, the fp32 q | k projection, the low halves of rotated q and of the new keys
  bf16_t *ylo, *qlo, *klo;
  float* qk32;          // level 1: [rows][2H] (q | k); level 2: [rows][3H] (q | k | v)
  int klo_tiles;        // K_lo tiles per sequence
  // precise level 2 (every GEMM A operand a pair): low halves of the attention output, the SwiGLU output and the final norm; fp32 gate/up
  bf16_t *attlo, *hlo, *ynlo;
  float* gu32;
  // precise level 3: MX-FP4 images (codes + block exponents) of the rounding remainders of the norm output, the attention output and the
  // SwiGLU output (vt_mx4.hip); ynlo above for the lm_head's pair
  uint8_t *y4, *yexp, *att4, *attexp, *h4, *hexp;
  // NF4 layers, launches of > 32 rows: one Linear's dequantised weights at a time (max(3H, 2I) x H op16), in front of the tile GEMMs
  bf16_t* wdq;
  // fp8 KV cache, prefills: the 16-bit staging pool of ONE layer (n_stage_tiles K tiles + V^T tiles) and its identity tile table
  bf16_t* stage_k;
  uint16_t* stage_vt;
  int* stage_table;
  size_t total;
};
constexpr int kTailRows = 16;   // most logit rows the pruned last layer takes (the M <= 16 limit of vt_gemm_skinny_norm_launch)
LlamaWs llama_carve(const vt_llama_model* m, int rows, int n_logit, int nseq, int max_kv_len, void* p, size_t n, int n_stage_tiles = 0) {
  Carver ws(p, n);
  LlamaWs w;
  const int H = m->hidden, I = m->intermediate;
  w.x = (float*)ws.take((size_t)rows * H * 4);
  w.y = (bf16_t*)ws.take((size_t)rows * H * 2);
  w.qkv = (bf16_t*)ws.take((size_t)rows * 3 * H * 2);
  w.att = (bf16_t*)ws.take((size_t)rows * H * 2);
  w.h = (bf16_t*)ws.take((size_t)rows * I * 2);
  w.yn = (bf16_t*)ws.take((size_t)(n_logit > 0 ? n_logit : 1) * H * 2);
  w.rs_a = (float*)ws.take(std::max((size_t)16 * (H / 16), rows > 64 ? (size_t)rows * (H / 32) : (size_t)0) * 4);
  w.rs_b = (float*)ws.take((size_t)16 * (H / 16) * 4);
  w.rstd = (float*)ws.take((size_t)(rows > 64 ? rows : 1) * 4);
  // tiles * ksplit <= 256 tiles of 256x256 fp32: 64 MiB covers every case the dispatcher splits
  w.splitk_bytes = (rows > 64) ? ((size_t)256 * 256 * 256 * 4) : 0;
  w.splitk = w.splitk_bytes ? (float*)ws.take(w.splitk_bytes) : nullptr;
  // (the pruned last layer runs one single-query problem per logit row, and several logit rows may sit in one sequence)
  w.attn_scratch_bytes = vt_attn_decode_scratch_bytes(std::max(std::max(nseq, std::min(n_logit, kTailRows)), 1), m->heads, m->head_dim,
                                                      max_kv_len > 0 ? max_kv_len : 64);
  w.attn_scratch = (float*)ws.take(w.attn_scratch_bytes);
  w.row_slot = (int*)ws.take((size_t)rows * 4);
  w.tail_seq = (VtAttnSeq*)ws.take((size_t)kTailRows * sizeof(VtAttnSeq));
  w.y_l = (bf16_t*)ws.take((size_t)kTailRows * H * 2);
  w.q_l = (bf16_t*)ws.take((size_t)kTailRows * H * 2);
  w.att_l = (bf16_t*)ws.take((size_t)kTailRows * H * 2);
  w.h_l = (bf16_t*)ws.take((size_t)kTailRows * I * 2);
  w.x_l = (float*)ws.take((size_t)kTailRows * H * 4);
  w.ylo = w.qlo = w.klo = nullptr;
  w.qk32 = nullptr;
  w.klo_tiles = 0;
  w.attlo = w.hlo = w.ynlo = nullptr;
  w.gu32 = nullptr;
  w.y4 = w.yexp = w.att4 = w.attexp = w.h4 = w.hexp = nullptr;
  w.wdq = nullptr;
  bool nf4 = false;
  for (int l = 0; l < m->num_layers && m->layers; ++l) nf4 = nf4 || m->layers[l].wqkv_nf4 != nullptr;
  if (nf4 && rows > 32) w.wdq = (bf16_t*)ws.take((size_t)std::max(3 * H, 2 * I) * H * 2);
  if (m->precise_qk == 3 && m->head_dim == 128 && rows > 1) {
    w.y4 = (uint8_t*)ws.take((size_t)rows * (H / 2));
    w.yexp = (uint8_t*)ws.take(vt_mx4_aexp_bytes(rows, H));
    w.att4 = (uint8_t*)ws.take((size_t)rows * (H / 2));
    w.attexp = (uint8_t*)ws.take(vt_mx4_aexp_bytes(rows, H));
    w.h4 = (uint8_t*)ws.take((size_t)rows * (I / 2));
    w.hexp = (uint8_t*)ws.take(vt_mx4_aexp_bytes(rows, I));
    w.ynlo = (bf16_t*)ws.take((size_t)(n_logit > 0 ? n_logit : 1) * H * 2);
  } else if (m->precise_qk >= 1 && m->head_dim == 128 && rows > 1) {   // (sized whenever the mode is on: the query does not know max_q_len)
    const bool full = m->precise_qk >= 2;
    w.ylo = (bf16_t*)ws.take((size_t)rows * H * 2);
    w.qlo = (bf16_t*)ws.take((size_t)rows * H * 2);
    w.qk32 = (float*)ws.take((size_t)rows * (full ? 3 : 2) * H * 4);
    // a sequence of q rows touches at most rows / 64 + 2 tiles; every sequence gets the same number of slots
    w.klo_tiles = rows / 64 + 2;
    w.klo = (bf16_t*)ws.take((size_t)(nseq > 0 ? nseq : 1) * w.klo_tiles * H * 64 * 2);
    if (full) {
      w.attlo = (bf16_t*)ws.take((size_t)rows * H * 2);
      w.hlo = (bf16_t*)ws.take((size_t)rows * I * 2);
      w.ynlo = (bf16_t*)ws.take((size_t)(n_logit > 0 ? n_logit : 1) * H * 2);
      w.gu32 = (float*)ws.take((size_t)rows * 2 * I * 4);
    }
  }
  w.stage_k = nullptr;
  w.stage_vt = nullptr;
  w.stage_table = nullptr;
  if (n_stage_tiles > 0 && rows > nseq) {   // (rows > nseq: some sequence brings more than one row, i.e. the pass may be a prefill)
    const size_t tile = (size_t)m->heads * 64 * m->head_dim * 2;
    w.stage_k = (bf16_t*)ws.take((size_t)n_stage_tiles * tile);
    w.stage_vt = (uint16_t*)ws.take((size_t)n_stage_tiles * tile);
    w.stage_table = (int*)ws.take((size_t)n_stage_tiles * 4);
  }
  w.total = ws.off + 256;
  return w;
}
// The decoder pass behind vt_llama_forward (kv16) and vt_llama_forward_kv8 (kv8): exactly one of the two pools is given. The two differ
// only in the "attend" step of a layer: decode steps run the fused kernel of the pool's format; prefills on an fp8 pool run the 16-bit
// kernels on the workspace's staging pool between a dequantisation of the past tiles and a quantisation of the tiles with new rows.
int llama_forward_body(const vt_llama_model* m, const vt_kv_cache* kv16, const vt_kv_cache8* kv8, int n_table_tiles, const uint16_t* x_embeds,
                       int rows, const int* positions, const int* seq_desc, int nseq, int max_q_len, int max_new_tiles, int max_kv_len,
                       const int* tile_table, const int* logit_rows, int n_logit_rows, float* logits, float* out_hidden, void* workspace,
                       size_t workspace_bytes, void* stream) {
  VT_REQUIRE(rows > 0 && nseq > 0 && max_q_len > 0 && max_new_tiles > 0 && max_kv_len > 0, "vt_llama_forward: empty batch");
  VT_REQUIRE(m->head_dim == 128 || m->head_dim == 64, "vt_llama_forward: head_dim %d unsupported", m->head_dim);
  VT_REQUIRE(m->hidden == m->heads * m->head_dim, "vt_llama_forward: hidden != heads*head_dim");
  VT_REQUIRE(m->hidden % 64 == 0 && m->intermediate % 64 == 0, "vt_llama_forward: hidden/intermediate must be multiples of 64");
  VT_REQUIRE(m->rope_cos && m->rope_sin, "vt_llama_forward: rope tables missing");
  if (n_logit_rows > 0) VT_REQUIRE(logits && logit_rows, "vt_llama_forward: logits requested but pointer missing");
  hipStream_t s = S(stream);
  LlamaWs w = llama_carve(m, rows, n_logit_rows, nseq, max_kv_len, workspace, workspace_bytes, kv8 ? n_table_tiles : 0);
  if (w.total > workspace_bytes) {
    vt_set_error("vt_llama_forward: workspace too small (%zu < %zu)", workspace_bytes, w.total);
    return VT_ERR_WORKSPACE;
  }
  const int H = m->hidden, I = m->intermediate, heads = m->heads, HD = m->head_dim;
  const int AUTO = VT_GEMM_CFG_AUTO;
  const float scale = 1.0f / sqrtf((float)HD);
  const size_t layer_stride = (size_t)(kv8 ? kv8->num_pages : kv16->num_pages) * heads * 64 * HD;
  if (kv8 && max_q_len > 1) {   // prefill on an fp8 pool: the staging pool and its identity table (slot = table_off + t)
    VT_REQUIRE(w.stage_k && w.stage_vt && w.stage_table, "vt_llama_forward_kv8: the workspace carries no staging pool (rows %d, nseq %d)", rows, nseq);
    VT_TRY(vt_kv8_iota_launch(w.stage_table, n_table_tiles, s));
  }
  // no sequence has a past when every sequence brings max_q_len rows and none holds more keys than that (sufficient, host-side: seq_desc
  // lives on the device); the dequantisation launch is skipped then
  const bool kv8_no_past = (long)nseq * max_q_len == (long)rows && max_kv_len == max_q_len;

  VT_TRY(vt_bf16_to_f32_launch(x_embeds, w.x, (size_t)rows * H, s));
  if (m->embeds_lo) VT_TRY(vt_add_op_to_f32_launch(w.x, m->embeds_lo, (size_t)rows * H, s));   // the input embeddings as a pair (precise level 2)
  // Decode steps (<= 16 rows, one new token per sequence): every GEMM is the weight-streaming kernel and RMSNorm is folded
  // into them -- the residual GEMMs (o_proj, down_proj) emit bf16(x .* w_next) plus per-block sums of x^2, the GEMMs that
  // follow (gate_up, next layer's qkv) scale their rows by rstd. Only the first norm of layer 0 and the final norm stay
  // separate launches: 6 launches per layer -> 4.
  const bool fold_norm = rows <= 16 && max_q_len == 1 && (H % 1024) == 0 && H <= 8192 && (I % 64) == 0;
  // Opt-in (vt_llama_model.prefill_norm_fold = 1): measured neutral to slightly slower on the C3 step -- the 1.9 ms of RMSNorm
  // launches it removes come back as longer residual epilogues (+12 us each: the y store), the finalize launches and ~1.5 %
  // slower consumer GEMMs (same code, un-normalised operands: the MFMA clock is data dependent on this power-limited part).
  const bool fold_tile = m->prefill_norm_fold == 1 && !fold_norm && vt_gemm_norm_fold_supported(rows, H, H) && (I % 64) == 0;
  VtGemmNormFuse consume_a, consume_b, none;
  consume_a.in_partials = w.rs_a;
  consume_b.in_partials = w.rs_b;
  consume_a.in_n = consume_b.in_n = H / 16;
  consume_a.inv_dim = consume_b.inv_dim = 1.0f / (float)H;
  consume_a.eps = consume_b.eps = m->rms_eps;
  // opt-in (vt_llama_model.qkv_fuse): prefill with the QKV projection on ONE launch of the 256x256 ping-pong kernel whose epilogue
  // writes rotated q / K pages / V^T pages itself (no vt_kv_tiles pass). Bit-identical, measured slower: default off
  const bool fuse_qkv = max_q_len > 1 && !fold_tile && m->qkv_fuse == 1 && vt_gemm_qkv_fused_supported(rows, H, HD);
  // opt-in (vt_llama_model.precise_qk): prefills carry q and k as operand pairs through the QKV projection and the attention scores
  // precise level 3: every decoder Linear of a prefill as ONE launch with the MX-FP4 product of the A operand's remainder folded in
  const bool precise3 = max_q_len > 1 && !fold_norm && m->precise_qk == 3;
  if (precise3) {   // a request the shapes cannot serve is an error, never a silent standard-mode pass
    VT_REQUIRE(HD == 128 && (H % 512) == 0 && (I % 128) == 0 && w.y4 != nullptr, "vt_llama_forward: precise level 3 needs head_dim 128, hidden %% 512 == 0, intermediate %% 128 == 0 (H=%d I=%d)", H, I);
    for (int l = 0; l < m->num_layers; ++l) {
      const vt_llama_layer& L = m->layers[l];
      VT_REQUIRE(L.wqkv4 && L.wqkv_e && L.wo4 && L.wo_e && L.wgu4 && L.wgu_e && L.wdown4 && L.wdown_e, "vt_llama_forward: precise level 3 without the weights' MX-FP4 images (layer %d)", l);
    }
  }
  const bool precise = !precise3 && max_q_len > 1 && !fold_norm && m->precise_qk >= 1 && HD == 128 && w.qk32 != nullptr && max_new_tiles <= w.klo_tiles;
  if (m->precise_qk >= 1 && m->precise_qk <= 2 && max_q_len > 1 && !fold_norm)
    VT_REQUIRE(precise, "vt_llama_forward: precise level %d was requested and cannot run here (head_dim %d, %d new tiles per sequence against %d slots)", m->precise_qk, HD, max_new_tiles, w.klo_tiles);
  const bool precise2 = precise && m->precise_qk >= 2 && w.gu32 != nullptr;
  // The last layer of a prefill, standard mode, when only <= 16 rows are read afterwards (the logit rows; nobody asked for the hidden
  // stream): K and V of every row still go into the pages, but q, the attention, o_proj, the second norm and the MLP run on the logit
  // rows alone -- gathered into compact buffers and pushed through what a decode step runs (weight-streaming GEMMs, single-query split-KV
  // attention with one device-built descriptor per row). The pages are the same bits as on the full path; the logits see the decode
  // step's summation order. vt_llama_model.last_layer_full = 1 keeps the full path (A/B, tests). qkv_fuse = 1 fuses the page writes of the
  // layers in front of it and leaves the pruned layer as it is (its q-less page write has nothing to fuse): qkv_fuse stays bit-identical
  // to the default, pool and logits.
  const bool prune_last = max_q_len > 1 && rows > 32 && !out_hidden && n_logit_rows >= 0 && n_logit_rows <= kTailRows && m->precise_qk == 0 &&
                          m->prefill_norm_fold == 0 && m->last_layer_full == 0;
  for (int l = 0; l < m->num_layers; ++l) {   // NF4 layers: all four matrices in 4 bits, nothing else
    const vt_llama_layer& L = m->layers[l];
    if (!L.wqkv_nf4 && !L.wo_nf4 && !L.wgu_nf4 && !L.wdown_nf4) {
      VT_REQUIRE(L.wqkv && L.wo && L.wgu && L.wdown, "vt_llama_forward: layer %d has no weights", l);
      continue;
    }
    VT_REQUIRE(L.wqkv_nf4 && L.wqkv_absmax && L.wo_nf4 && L.wo_absmax && L.wgu_nf4 && L.wgu_absmax && L.wdown_nf4 && L.wdown_absmax,
               "vt_llama_forward: layer %d has only some of its NF4 matrices", l);
    VT_REQUIRE(!L.wqkv && !L.wo && !L.wgu && !L.wdown, "vt_llama_forward: layer %d carries both 16-bit and NF4 weights", l);
    VT_REQUIRE(m->precise_qk == 0, "vt_llama_forward: precise level %d cannot run on NF4 weights (layer %d)", m->precise_qk, l);
    VT_REQUIRE((H % 128) == 0 && (I % 128) == 0, "vt_llama_forward: NF4 layers need hidden and intermediate %% 128 == 0 (H=%d I=%d)", H, I);
    VT_REQUIRE(rows <= 32 || w.wdq != nullptr, "vt_llama_forward: NF4 dequantisation buffer missing");
  }
  if (fuse_qkv) VT_TRY(vt_row_slot_launch((const VtAttnSeq*)seq_desc, nseq, max_q_len, tile_table, w.row_slot, s));
  for (int l = 0; l < m->num_layers; ++l) {
    const vt_llama_layer& L = m->layers[l];
    if (m->hidden_trace)
      VT_HIP(hipMemcpyAsync(m->hidden_trace + (size_t)l * rows * H, w.x, (size_t)rows * H * 4, hipMemcpyDeviceToDevice, s));
    // the same stream at the logit rows only, rounded once to the operand format (DoLa's candidate layers: DESIGN.md 9.14)
    if (m->logit_row_trace && n_logit_rows > 0 && (!m->logit_row_trace_layers || m->logit_row_trace_layers[l]))
      VT_TRY(vt_gather_f32_to_bf16_launch(w.x, logit_rows, m->logit_row_trace + (size_t)l * n_logit_rows * H, n_logit_rows, H, s));
    // fp8 pool: kt / vt are the staging pool (prefills only; decode steps read k8 / vt8)
    bf16_t* kt = kv8 ? w.stage_k : kv16->k + l * layer_stride;
    bf16_t* vt = kv8 ? w.stage_vt : kv16->vt + l * layer_stride;
    uint8_t* k8 = kv8 ? kv8->k + l * layer_stride : nullptr;
    uint8_t* vt8 = kv8 ? kv8->vt + l * layer_stride : nullptr;
    // the "attend" step of a decode pass: rotary + append + attention + combine in one launch, on the pool's format
    auto attend_decode = [&]() -> int {
      if (kv8)
        return vt_attn_decode_fused_kv8_launch(w.qkv, 3 * H, 0, H, 2 * H, k8, vt8, tile_table, (const VtAttnSeq*)seq_desc, nseq, w.att, H,
                                               heads, HD, scale, m->rope_cos, m->rope_sin, positions, s);
      return vt_attn_decode_fused_launch(w.qkv, 3 * H, 0, H, 2 * H, kt, vt, tile_table, (const VtAttnSeq*)seq_desc, nseq, w.att, H,
                                         heads, HD, scale, m->rope_cos, m->rope_sin, positions, s);
    };
    // ... and of a standard-mode prefill: vt_kv_tiles (unless the QKV epilogue wrote the pages) + the prefill attention; on an fp8 pool
    // the same two launches run on the staging pool, between the dequantisation of the past and the quantisation of the new tiles
    auto attend_prefill = [&](bool tiles) -> int {
      const int* tt = kv8 ? w.stage_table : tile_table;
      if (kv8 && !kv8_no_past)
        VT_TRY(vt_kv8_dequant_past_launch(k8, vt8, kt, vt, tile_table, (const VtAttnSeq*)seq_desc, nseq, max_kv_len, heads, HD, s));
      if (tiles)
        VT_TRY(vt_kv_tiles_launch(w.qkv, 3 * H, 0, H, 2 * H, kt, vt, tt, (const VtAttnSeq*)seq_desc, nseq,
                                  max_new_tiles, heads, HD, m->rope_cos, m->rope_sin, positions, s));
      VT_TRY(vt_flash_attn_launch(w.qkv, 3 * H, kt, vt, tt, (const VtAttnSeq*)seq_desc, nseq, max_q_len, w.att, H,
                                  heads, HD, 1, scale, s));
      if (kv8) VT_TRY(vt_kv8_quant_new_launch(kt, vt, k8, vt8, tile_table, (const VtAttnSeq*)seq_desc, nseq, max_new_tiles, heads, HD, s));
      return VT_OK;
    };
    const bool nf4 = L.wqkv_nf4 != nullptr;
    // one decoder Linear of <= 32 rows: the 16-bit weight-streaming kernel, or its NF4 counterpart on an NF4 layer (same norm folding)
    auto skinny = [&](const bf16_t* A, int lda, const bf16_t* W16, const uint8_t* W4, const float* absmax, void* C, int ldc, int N, int K, int epi,
                      const VtGemmNormFuse& nf) -> int {
      if (nf4) return vt_gemm_nf4_launch(A, lda, W4, absmax, C, ldc, rows, N, K, epi, nf, s);
      return vt_gemm_skinny_norm_launch(A, lda, W16, K, C, ldc, rows, N, K, epi, nf, s);
    };
    if (fold_norm) {
      if (l == 0) {
        VT_TRY(vt_rmsnorm_launch(w.x, nullptr, L.rms1, w.y, rows, H, m->rms_eps, s));
        VT_TRY(skinny(w.y, H, L.wqkv, L.wqkv_nf4, L.wqkv_absmax, w.qkv, 3 * H, 3 * H, H, VT_EPI_BF16, none));
      } else {
        VT_TRY(skinny(w.y, H, L.wqkv, L.wqkv_nf4, L.wqkv_absmax, w.qkv, 3 * H, 3 * H, H, VT_EPI_BF16, consume_a));
      }
      VT_TRY(attend_decode());
      VtGemmNormFuse prod_b;   // x += att Wo^T ; y = bf16(x .* rms2) ; partial sums -> rs_b
      prod_b.out_w = L.rms2;
      prod_b.out_xw = w.y;
      prod_b.ld_xw = H;
      prod_b.out_partials = w.rs_b;
      VT_TRY(skinny(w.att, H, L.wo, L.wo_nf4, L.wo_absmax, w.x, H, H, H, VT_EPI_F32_RESID, prod_b));
      VT_TRY(skinny(w.y, H, L.wgu, L.wgu_nf4, L.wgu_absmax, w.h, I, 2 * I, H, VT_EPI_SWIGLU_BF16, consume_b));
      if (l + 1 < m->num_layers) {
        VtGemmNormFuse prod_a;   // x += h Wdown^T ; y = bf16(x .* next layer's rms1) ; partial sums -> rs_a
        prod_a.out_w = m->layers[l + 1].rms1;
        prod_a.out_xw = w.y;
        prod_a.ld_xw = H;
        prod_a.out_partials = w.rs_a;
        VT_TRY(skinny(w.h, I, L.wdown, L.wdown_nf4, L.wdown_absmax, w.x, H, H, I, VT_EPI_F32_RESID, prod_a));
      } else {
        VT_TRY(skinny(w.h, I, L.wdown, L.wdown_nf4, L.wdown_absmax, w.x, H, H, I, VT_EPI_F32_RESID, none));
      }
      continue;
    }
    if (nf4 && rows <= 32) {   // NF4, <= 32 rows without the fold (17..32 decode rows, padded-batch fix-ups, short prefills): norms as launches
      VT_TRY(vt_rmsnorm_launch(w.x, nullptr, L.rms1, w.y, rows, H, m->rms_eps, s));
      VT_TRY(skinny(w.y, H, nullptr, L.wqkv_nf4, L.wqkv_absmax, w.qkv, 3 * H, 3 * H, H, VT_EPI_BF16, none));
      if (max_q_len == 1) {
        VT_TRY(attend_decode());
      } else {
        VT_TRY(attend_prefill(true));
      }
      VT_TRY(skinny(w.att, H, nullptr, L.wo_nf4, L.wo_absmax, w.x, H, H, H, VT_EPI_F32_RESID, none));
      VT_TRY(vt_rmsnorm_launch(w.x, nullptr, L.rms2, w.y, rows, H, m->rms_eps, s));
      VT_TRY(skinny(w.y, H, nullptr, L.wgu_nf4, L.wgu_absmax, w.h, I, 2 * I, H, VT_EPI_SWIGLU_BF16, none));
      VT_TRY(skinny(w.h, I, nullptr, L.wdown_nf4, L.wdown_absmax, w.x, H, H, I, VT_EPI_F32_RESID, none));
      continue;
    }
    // NF4 layer, > 32 rows: each Linear dequantised into w.wdq right in front of its (unchanged) tile GEMM -- stream order keeps the one
    // buffer safe to reuse. 16-bit layer: the weights as they are.
    auto dq = [&](const bf16_t* W16, const uint8_t* W4, const float* absmax, int N, int K, const bf16_t** out) -> int {
      *out = W16;
      if (!nf4) return VT_OK;
      *out = w.wdq;
      return vt_nf4_dequant_launch(W4, absmax, N, K, w.wdq, K, s);
    };
    const bf16_t *Wqkv, *Wo, *Wgu, *Wdown;
    // Prefill (rows > 64): the same fold on the MFMA tile kernels -- the residual GEMMs (o_proj, down_proj) also store
    // y = bf16(x .* w_next) and per-row sums of x^2 per 32-column group, one small launch turns those into rstd[row], and the GEMM
    // that consumes y (gate_up, the next layer's qkv) scales its accumulator rows by rstd. Saves the 84 MB read of x per norm
    // (opt-in, see above).
    VtGemmNormFuse cons_t;
    cons_t.row_scale = w.rstd;
    if (precise3) {
      VT_TRY(vt_rmsnorm_mx_launch(w.x, nullptr, L.rms1, w.y, w.y4, w.yexp, rows, H, m->rms_eps, s));
      VT_TRY(vt_gemm_mx_launch(w.y, H, w.y4, w.yexp, L.wqkv, H, L.wqkv4, L.wqkv_e, w.qkv, 3 * H, nullptr, rows, 3 * H, H, VT_EPI_BF16, 1, 0, nullptr,
                               nullptr, s));
      VT_TRY(vt_kv_tiles_launch(w.qkv, 3 * H, 0, H, 2 * H, kt, vt, tile_table, (const VtAttnSeq*)seq_desc, nseq, max_new_tiles, heads, HD,
                                m->rope_cos, m->rope_sin, positions, s));
      VT_TRY(vt_flash_attn_launch(w.qkv, 3 * H, kt, vt, tile_table, (const VtAttnSeq*)seq_desc, nseq, max_q_len, w.att, H, heads, HD, 1, scale, s,
                                  w.att4, w.attexp));
      VT_TRY(vt_gemm_mx_resid_launch(w.att, H, w.att4, w.attexp, L.wo, H, L.wo4, L.wo_e, w.x, H, nullptr, rows, H, H, w.splitk, w.splitk_bytes, s));
      VT_TRY(vt_rmsnorm_mx_launch(w.x, nullptr, L.rms2, w.y, w.y4, w.yexp, rows, H, m->rms_eps, s));
      VT_TRY(vt_gemm_mx_launch(w.y, H, w.y4, w.yexp, L.wgu, H, L.wgu4, L.wgu_e, w.h, I, nullptr, rows, 2 * I, H, VT_EPI_SWIGLU_MX, 1, 0, w.h4, w.hexp,
                               s));
      VT_TRY(vt_gemm_mx_resid_launch(w.h, I, w.h4, w.hexp, L.wdown, I, L.wdown4, L.wdown_e, w.x, H, nullptr, rows, H, I, w.splitk, w.splitk_bytes, s));
      continue;
    }
    if (precise2) {
      // precise level 2: EVERY GEMM A operand is a pair (hi + lo), each product as two launches accumulating in fp32: the q | k | v
      // projection into fp32, o_proj / down_proj as two residual launches, gate/up into fp32 with the SwiGLU (pair out) as its own pass
      VT_TRY(vt_rmsnorm_hilo_launch(w.x, nullptr, L.rms1, w.y, w.ylo, rows, H, m->rms_eps, s));
      VT_TRY(vt_gemm_launch(w.y, H, L.wqkv, H, w.qk32, 3 * H, nullptr, rows, 3 * H, H, VT_EPI_F32, AUTO, s));
      VT_TRY(vt_gemm_resid_launch(w.ylo, H, L.wqkv, H, w.qk32, 3 * H, nullptr, rows, 3 * H, H, 0, w.splitk, w.splitk_bytes, s));
      VT_TRY(vt_kv_tiles_precise_launch(w.qk32, 3 * H, 1, w.qkv, 3 * H, 0, 2 * H, w.qlo, kt, vt, w.klo, tile_table, (const VtAttnSeq*)seq_desc, nseq,
                                        max_new_tiles, heads, HD, m->rope_cos, m->rope_sin, positions, s));
      VT_TRY(vt_flash_attn_precise_launch(w.qkv, 3 * H, w.qlo, H, kt, w.klo, max_new_tiles, vt, tile_table, (const VtAttnSeq*)seq_desc, nseq,
                                          max_q_len, w.att, H, w.attlo, heads, HD, 1, scale, s));
      VT_TRY(vt_gemm_resid_launch(w.att, H, L.wo, H, w.x, H, nullptr, rows, H, H, 0, w.splitk, w.splitk_bytes, s));
      VT_TRY(vt_gemm_resid_launch(w.attlo, H, L.wo, H, w.x, H, nullptr, rows, H, H, 0, w.splitk, w.splitk_bytes, s));
      VT_TRY(vt_rmsnorm_hilo_launch(w.x, nullptr, L.rms2, w.y, w.ylo, rows, H, m->rms_eps, s));
      VT_TRY(vt_gemm_launch(w.y, H, L.wgu, H, w.gu32, 2 * I, nullptr, rows, 2 * I, H, VT_EPI_F32, AUTO, s));
      VT_TRY(vt_gemm_resid_launch(w.ylo, H, L.wgu, H, w.gu32, 2 * I, nullptr, rows, 2 * I, H, 0, w.splitk, w.splitk_bytes, s));
      VT_TRY(vt_act_pair_launch(w.gu32, 2 * I, w.h, w.hlo, rows, I, 2, s));
      VT_TRY(vt_gemm_resid_launch(w.h, I, L.wdown, I, w.x, H, nullptr, rows, H, I, 0, w.splitk, w.splitk_bytes, s));
      VT_TRY(vt_gemm_resid_launch(w.hlo, I, L.wdown, I, w.x, H, nullptr, rows, H, I, 0, w.splitk, w.splitk_bytes, s));
      continue;
    }
    if (precise) {
      // precise_qk: the q / k projection as A_hi.W^T + A_lo.W^T into fp32 (two tile GEMMs, the second accumulating), v as usual;
      // rotary in fp32, q / k rounded once into operand pairs; attention on K_hi.(Q_hi + Q_lo)^T + K_lo.Q_hi^T
      VT_TRY(vt_rmsnorm_hilo_launch(w.x, nullptr, L.rms1, w.y, w.ylo, rows, H, m->rms_eps, s));
      VT_TRY(vt_gemm_launch(w.y, H, L.wqkv, H, w.qk32, 2 * H, nullptr, rows, 2 * H, H, VT_EPI_F32, AUTO, s));
      VT_TRY(vt_gemm_resid_launch(w.ylo, H, L.wqkv, H, w.qk32, 2 * H, nullptr, rows, 2 * H, H, 0, w.splitk, w.splitk_bytes, s));
      VT_TRY(vt_gemm_launch(w.y, H, L.wqkv + (size_t)2 * H * H, H, w.qkv + 2 * H, 3 * H, nullptr, rows, H, H, VT_EPI_BF16, AUTO, s));
      VT_TRY(vt_kv_tiles_precise_launch(w.qk32, 2 * H, 0, w.qkv, 3 * H, 0, 2 * H, w.qlo, kt, vt, w.klo, tile_table, (const VtAttnSeq*)seq_desc, nseq,
                                        max_new_tiles, heads, HD, m->rope_cos, m->rope_sin, positions, s));
      VT_TRY(vt_flash_attn_precise_launch(w.qkv, 3 * H, w.qlo, H, kt, w.klo, max_new_tiles, vt, tile_table, (const VtAttnSeq*)seq_desc, nseq,
                                          max_q_len, w.att, H, nullptr, heads, HD, 1, scale, s));
      VT_TRY(vt_gemm_resid_launch(w.att, H, L.wo, H, w.x, H, nullptr, rows, H, H, 0, w.splitk, w.splitk_bytes, s));
      VT_TRY(vt_rmsnorm_launch(w.x, nullptr, L.rms2, w.y, rows, H, m->rms_eps, s));
      VT_TRY(vt_gemm_launch(w.y, H, L.wgu, H, w.h, I, nullptr, rows, 2 * I, H, VT_EPI_SWIGLU_BF16, AUTO, s));
      VT_TRY(vt_gemm_resid_launch(w.h, I, L.wdown, I, w.x, H, nullptr, rows, H, I, 0, w.splitk, w.splitk_bytes, s));
      continue;
    }
    if (prune_last && l == m->num_layers - 1) {
      const int n = n_logit_rows;
      const int* tt = kv8 ? w.stage_table : tile_table;
      VT_TRY(vt_rmsnorm_launch(w.x, nullptr, L.rms1, w.y, rows, H, m->rms_eps, s));
      // k | v projection of every row: the fused weight is [3H][H] with q first, so k | v are its last 2H rows (NF4: only those are dequantised)
      const bf16_t* Wkv = nf4 ? w.wdq : L.wqkv + (size_t)H * H;
      if (nf4) VT_TRY(vt_nf4_dequant_launch(L.wqkv_nf4 + (size_t)H * (H / 2), L.wqkv_absmax + (size_t)H * (H / 64), 2 * H, H, w.wdq, H, s));
      VT_TRY(vt_gemm_launch(w.y, H, Wkv, H, w.qkv + H, 3 * H, nullptr, rows, 2 * H, H, VT_EPI_BF16, AUTO, s));
      if (kv8 && !kv8_no_past)
        VT_TRY(vt_kv8_dequant_past_launch(k8, vt8, kt, vt, tile_table, (const VtAttnSeq*)seq_desc, nseq, max_kv_len, heads, HD, s));
      VT_TRY(vt_kv_tiles_launch(w.qkv, 3 * H, -1, H, 2 * H, kt, vt, tt, (const VtAttnSeq*)seq_desc, nseq, max_new_tiles, heads, HD, m->rope_cos,
                                m->rope_sin, positions, s));
      // one decoder Linear on the n compact rows. NF4 layer: the matrix is dequantised into w.wdq first, as in front of the tile GEMMs of the
      // other layers -- a prefill of > 32 rows on NF4 weights stays bit-equal to the 16-bit decoder built from the dequantised weights
      // (the 4-bit weight-streaming kernel sums in another order)
      auto tail = [&](const bf16_t* A, int lda, const bf16_t* W16, const uint8_t* W4, const float* absmax, void* C, int ldc, int N, int K,
                      int epi) -> int {
        if (nf4) {
          VT_TRY(vt_nf4_dequant_launch(W4, absmax, N, K, w.wdq, K, s));
          W16 = w.wdq;
        }
        return vt_gemm_skinny_norm_launch(A, lda, W16, K, C, ldc, n, N, K, epi, none, s);
      };
      if (n > 0) {   // q of the logit rows (rows 0..H of the fused weight), rotated, against the keys each row sees in the causal pass
        VT_TRY(vt_gather_rows_launch(w.y, logit_rows, w.y_l, n, (size_t)H * 2, s));
        VT_TRY(tail(w.y_l, H, L.wqkv, L.wqkv_nf4, L.wqkv_absmax, w.q_l, H, H, H, VT_EPI_BF16));
        VT_TRY(vt_rope_rows_launch(w.q_l, H, logit_rows, n, positions, m->rope_cos, m->rope_sin, heads, HD, s));
        VT_TRY(vt_attn_tail_desc_launch((const VtAttnSeq*)seq_desc, nseq, logit_rows, n, w.tail_seq, s));
        VT_TRY(vt_attn_decode_launch(w.q_l, H, kt, vt, tt, w.tail_seq, n, w.att_l, H, heads, HD, scale, max_kv_len, w.attn_scratch,
                                     w.attn_scratch_bytes, s));
      }
      if (kv8) VT_TRY(vt_kv8_quant_new_launch(kt, vt, k8, vt8, tile_table, (const VtAttnSeq*)seq_desc, nseq, max_new_tiles, heads, HD, s));
      if (n > 0) {
        VT_TRY(vt_gather_rows_launch(w.x, logit_rows, w.x_l, n, (size_t)H * 4, s));
        VT_TRY(tail(w.att_l, H, L.wo, L.wo_nf4, L.wo_absmax, w.x_l, H, H, H, VT_EPI_F32_RESID));
        VT_TRY(vt_rmsnorm_launch(w.x_l, nullptr, L.rms2, w.y_l, n, H, m->rms_eps, s));
        VT_TRY(tail(w.y_l, H, L.wgu, L.wgu_nf4, L.wgu_absmax, w.h_l, I, 2 * I, H, VT_EPI_SWIGLU_BF16));
        VT_TRY(tail(w.h_l, I, L.wdown, L.wdown_nf4, L.wdown_absmax, w.x_l, H, H, I, VT_EPI_F32_RESID));
      }
      continue;
    }
    VT_TRY(dq(L.wqkv, L.wqkv_nf4, L.wqkv_absmax, 3 * H, H, &Wqkv));
    if (fold_tile && l > 0) {
      VT_TRY(vt_gemm_launch(w.y, H, Wqkv, H, w.qkv, 3 * H, nullptr, rows, 3 * H, H, VT_EPI_BF16, AUTO, s, &cons_t));
    } else if (fuse_qkv) {
      VT_TRY(vt_rmsnorm_launch(w.x, nullptr, L.rms1, w.y, rows, H, m->rms_eps, s));
      VtQkvFuse qf;
      qf.k_pages = kt;
      qf.vt_pages = vt;
      qf.row_slot = w.row_slot;
      qf.positions = positions;
      qf.rope_cos = m->rope_cos;
      qf.rope_sin = m->rope_sin;
      qf.heads = heads;
      VT_TRY(vt_gemm_qkv_fused_launch(w.y, H, Wqkv, H, w.qkv, 3 * H, rows, H, qf, s));
    } else {
      VT_TRY(vt_rmsnorm_launch(w.x, nullptr, L.rms1, w.y, rows, H, m->rms_eps, s));
      VT_TRY(vt_gemm_launch(w.y, H, Wqkv, H, w.qkv, 3 * H, nullptr, rows, 3 * H, H, VT_EPI_BF16, AUTO, s));
    }
    if (max_q_len == 1) {   // decode step: rotary + append + attention + combine in one launch
      VT_TRY(attend_decode());
    } else {
      VT_TRY(attend_prefill(!fuse_qkv));
    }
    if (fold_tile) {
      VtGemmNormFuse prod;
      prod.out_xw = w.y;
      prod.ld_xw = H;
      prod.out_partials = w.rs_a;
      prod.out_np = H / 32;
      prod.out_ldp = rows;
      prod.out_w = L.rms2;
      VT_TRY(dq(L.wo, L.wo_nf4, L.wo_absmax, H, H, &Wo));
      VT_TRY(vt_gemm_resid_launch(w.att, H, Wo, H, w.x, H, nullptr, rows, H, H, 0, w.splitk, w.splitk_bytes, s, &prod));
      VT_TRY(vt_rowscale_finalize_launch(w.rs_a, H / 32, rows, rows, 1.0f / (float)H, m->rms_eps, w.rstd, s));
      VT_TRY(dq(L.wgu, L.wgu_nf4, L.wgu_absmax, 2 * I, H, &Wgu));
      VT_TRY(vt_gemm_launch(w.y, H, Wgu, H, w.h, I, nullptr, rows, 2 * I, H, VT_EPI_SWIGLU_BF16, AUTO, s, &cons_t));
      VT_TRY(dq(L.wdown, L.wdown_nf4, L.wdown_absmax, H, I, &Wdown));
      if (l + 1 < m->num_layers) {
        prod.out_w = m->layers[l + 1].rms1;
        VT_TRY(vt_gemm_resid_launch(w.h, I, Wdown, I, w.x, H, nullptr, rows, H, I, 0, w.splitk, w.splitk_bytes, s, &prod));
        VT_TRY(vt_rowscale_finalize_launch(w.rs_a, H / 32, rows, rows, 1.0f / (float)H, m->rms_eps, w.rstd, s));
      } else {
        VT_TRY(vt_gemm_resid_launch(w.h, I, Wdown, I, w.x, H, nullptr, rows, H, I, 0, w.splitk, w.splitk_bytes, s));
      }
      continue;
    }
    VT_TRY(dq(L.wo, L.wo_nf4, L.wo_absmax, H, H, &Wo));
    VT_TRY(vt_gemm_resid_launch(w.att, H, Wo, H, w.x, H, nullptr, rows, H, H, 0, w.splitk, w.splitk_bytes, s));
    VT_TRY(vt_rmsnorm_launch(w.x, nullptr, L.rms2, w.y, rows, H, m->rms_eps, s));
    VT_TRY(dq(L.wgu, L.wgu_nf4, L.wgu_absmax, 2 * I, H, &Wgu));
    VT_TRY(vt_gemm_launch(w.y, H, Wgu, H, w.h, I, nullptr, rows, 2 * I, H, VT_EPI_SWIGLU_BF16, AUTO, s));
    VT_TRY(dq(L.wdown, L.wdown_nf4, L.wdown_absmax, H, I, &Wdown));
    VT_TRY(vt_gemm_resid_launch(w.h, I, Wdown, I, w.x, H, nullptr, rows, H, I, 0, w.splitk, w.splitk_bytes, s));
  }
  if (out_hidden) VT_HIP(hipMemcpyAsync(out_hidden, w.x, (size_t)rows * H * 4, hipMemcpyDeviceToDevice, s));
  if (n_logit_rows > 0 && (precise2 || precise3)) {   // level 2: the lm_head's operand as a pair too (any number of rows: a last-position-only call included)
    VT_TRY(vt_rmsnorm_hilo_launch(w.x, logit_rows, m->final_norm, w.yn, w.ynlo, n_logit_rows, H, m->rms_eps, s));
    VT_TRY(vt_gemm_launch(w.yn, H, m->lm_head, H, logits, m->vocab, nullptr, n_logit_rows, m->vocab, H, VT_EPI_F32, AUTO, s));
    VT_TRY(vt_gemm_resid_launch(w.ynlo, H, m->lm_head, H, logits, m->vocab, nullptr, n_logit_rows, m->vocab, H, 0, w.splitk, w.splitk_bytes, s));
  } else if (n_logit_rows > 0) {
    // (behind the pruned last layer the logit rows are the compact rows 0..n of x_l)
    VT_TRY(vt_rmsnorm_launch(prune_last ? w.x_l : w.x, prune_last ? nullptr : logit_rows, m->final_norm, w.yn, n_logit_rows, H, m->rms_eps, s));
    VT_TRY(vt_gemm_launch(w.yn, H, m->lm_head, H, logits, m->vocab, nullptr, n_logit_rows, m->vocab, H, VT_EPI_F32, AUTO, s));
  }
  return VT_OK;
}

}  // namespace

size_t vt_llama_workspace_bytes(const vt_llama_model* m, int rows, int n_logit_rows, int nseq, int max_kv_len) {
  if (!m) return 0;
  return llama_carve(m, rows, n_logit_rows, nseq, max_kv_len, nullptr, 0).total;
}

int vt_llama_forward(const vt_llama_model* m, const vt_kv_cache* kv, const uint16_t* x_embeds, int rows,
                     const int* positions, const int* seq_desc, int nseq, int max_q_len, int max_new_tiles, int max_kv_len,
                     const int* tile_table, const int* logit_rows, int n_logit_rows, float* logits,
                     float* out_hidden, void* workspace, size_t workspace_bytes, void* stream) {
  VT_REQUIRE(m && kv && x_embeds && positions && seq_desc && tile_table && workspace, "vt_llama_forward: null pointer");
  return llama_forward_body(m, kv, nullptr, 0, x_embeds, rows, positions, seq_desc, nseq, max_q_len, max_new_tiles, max_kv_len, tile_table,
                            logit_rows, n_logit_rows, logits, out_hidden, workspace, workspace_bytes, stream);
}

size_t vt_llama_workspace_bytes_kv8(const vt_llama_model* m, int rows, int n_logit_rows, int nseq, int max_kv_len, int n_table_tiles) {
  if (!m || n_table_tiles <= 0) return 0;
  return llama_carve(m, rows, n_logit_rows, nseq, max_kv_len, nullptr, 0, n_table_tiles).total;
}

int vt_llama_forward_kv8(const vt_llama_model* m, const vt_kv_cache8* kv, const uint16_t* x_embeds, int rows,
                         const int* positions, const int* seq_desc, int nseq, int max_q_len, int max_new_tiles, int max_kv_len,
                         const int* tile_table, int n_table_tiles, const int* logit_rows, int n_logit_rows, float* logits,
                         float* out_hidden, void* workspace, size_t workspace_bytes, void* stream) {
  VT_REQUIRE(m && kv && x_embeds && positions && seq_desc && tile_table && workspace, "vt_llama_forward_kv8: null pointer");
  VT_REQUIRE(kv->k && kv->vt, "vt_llama_forward_kv8: null pointer (pages)");
  VT_REQUIRE(n_table_tiles > 0, "vt_llama_forward_kv8: n_table_tiles must be the number of entries of tile_table");
  // an error, never a silent 16-bit pass: these modes write or read 16-bit pages directly
  VT_REQUIRE(m->precise_qk == 0, "vt_llama_forward_kv8: precise level %d cannot run on an fp8 KV cache", m->precise_qk);
  VT_REQUIRE(m->qkv_fuse == 0, "vt_llama_forward_kv8: qkv_fuse cannot run on an fp8 KV cache (its epilogue writes 16-bit pages)");
  return llama_forward_body(m, nullptr, kv, n_table_tiles, x_embeds, rows, positions, seq_desc, nseq, max_q_len, max_new_tiles, max_kv_len,
                            tile_table, logit_rows, n_logit_rows, logits, out_hidden, workspace, workspace_bytes, stream);
}

}  // extern "C"
