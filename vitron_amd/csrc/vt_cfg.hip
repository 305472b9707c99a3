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

static_assert(sizeof(vt_cfg_row) == 56 && alignof(vt_cfg_row) == 8, "vt_cfg_row is 56 bytes, 8-byte aligned (ABI)");
static_assert(offsetof(vt_cfg_row, cond) == 0 && offsetof(vt_cfg_row, uncond) == 8 && offsetof(vt_cfg_row, out) == 16 &&
                  offsetof(vt_cfg_row, base) == 24 && offsetof(vt_cfg_row, mask_out) == 32 && offsetof(vt_cfg_row, lse_out) == 40 &&
                  offsetof(vt_cfg_row, scale) == 48 && offsetof(vt_cfg_row, log_beta) == 52,
              "vt_cfg_row offsets are part of the ABI");

namespace {

constexpr int kCfgThreads = 1024;

// the two rows' reductions share their barriers; per row the order is vt_logprob_rows': 6 shuffle levels, then the 16 wave totals serially
__device__ __forceinline__ void cfg_block_max2(float& a, float& b, float (*sh)[16]) {
  a = wave_max(a);
  b = wave_max(b);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = a;
    sh[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  a = sh[0][0];
  b = sh[1][0];
  for (int i = 1; i < 16; ++i) {
    a = fmaxf(a, sh[0][i]);
    b = fmaxf(b, sh[1][i]);
  }
}
__device__ __forceinline__ void cfg_block_sum2(float& a, float& b, float (*sh)[16]) {
  a = wave_sum(a);
  b = wave_sum(b);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = a;
    sh[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  a = 0.f;
  b = 0.f;
  for (int i = 0; i < 16; ++i) {
    a += sh[0][i];
    b += sh[1][i];
  }
}
// The blend, every step rounded to nearest on its own: __fsub_rn / __fmul_rn / __fadd_rn in the header's statement of the contract.
// hipcc compiles those intrinsics as plain operators that carry its default contraction flag, so after inlining it fuses
// ul + s * d into an fma all the same (seen in the assembly: v_fmac_f32); the operators are therefore written out under
// fp contract(off), as vt_llama.hip's add_rounded is, which is what keeps the product and the sum apart.
__device__ __forceinline__ float cfg_blend(float c, float u, float lse_c, float lse_u, float scale) {
#pragma clang fp contract(off)
  const float cl = c - lse_c;
  const float ul = u - lse_u;
  const float d = cl - ul;
  const float p = scale * d;
  return ul + p;
}
// word w of the starting mask: base's word as it is, or the bits [0, V) (vt_ban_rows' convention)
__device__ __forceinline__ uint32_t cfg_base_word(const uint32_t* base, int w, int W, int V) {
  if (base != nullptr) return base[w];
  return (w == W - 1 && (V & 31)) ? (1u << (V & 31)) - 1u : 0xffffffffu;
}

template <bool kReg>
__global__ __launch_bounds__(kCfgThreads) void cfg_rows_kernel(const vt_cfg_row* __restrict__ rows, int V) {
  __shared__ float sh[2][16];
  const vt_cfg_row row = rows[blockIdx.x];
  if (row.cond == nullptr) return;       // block-uniform, before any barrier: the row is skipped entirely
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = (V + 31) >> 5;
  const float* cond = row.cond;          // (no __restrict__: out may alias cond)
  const float* unc = row.uncond;
  float* out = row.out;
  const float scale = row.scale;
  const bool aligned = (((uintptr_t)cond | (uintptr_t)unc | (uintptr_t)out) % 16) == 0;     // block-uniform

  if (kReg && aligned) {
    float c[32], u[32];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i0 = 4 * (tid + 1024 * j);
      if (i0 + 3 < V) {
        const f32x4 vc = *(const f32x4*)(cond + i0);
        const f32x4 vu = *(const f32x4*)(unc + i0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          c[4 * j + k] = vc[k];
          u[4 * j + k] = vu[k];
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          c[4 * j + k] = i0 + k < V ? cond[i0 + k] : -INFINITY;
          u[4 * j + k] = i0 + k < V ? unc[i0 + k] : -INFINITY;
        }
      }
    }
    float mc = -INFINITY, mu = -INFINITY;
#pragma unroll
    for (int s = 0; s < 32; ++s) {
      mc = fmaxf(mc, c[s]);
      mu = fmaxf(mu, u[s]);
    }
    cfg_block_max2(mc, mu, sh);
    float zc = 0.f, zu = 0.f;
#pragma unroll
    for (int s = 0; s < 32; ++s) {       // (a slot past V holds -inf: expf gives 0)
      zc += expf(c[s] - mc);
      zu += expf(u[s] - mu);
    }
    cfg_block_sum2(zc, zu, sh);
    const float lse_c = mc + logf(zc), lse_u = mu + logf(zu);
    if (tid == 0 && row.lse_out != nullptr) {
      row.lse_out[0] = lse_c;
      row.lse_out[1] = lse_u;
    }
    if (row.mask_out != nullptr) {       // block-uniform: every lane takes part in the shuffles
      const float thr = mc + row.log_beta;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i0 = 4 * (tid + 1024 * j);
        uint32_t nib = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) nib |= ((i0 + k >= V) | (c[4 * j + k] >= thr)) ? (1u << k) : 0u;
        uint32_t word = nib << (4 * (tid & 7));
        word |= __shfl_xor(word, 1, 64);
        word |= __shfl_xor(word, 2, 64);
        word |= __shfl_xor(word, 4, 64);
        const int w = (tid >> 3) + 128 * j;
        if ((tid & 7) == 0 && w < W) row.mask_out[w] = word & cfg_base_word(row.base, w, W, V);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i0 = 4 * (tid + 1024 * j);
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = cfg_blend(c[4 * j + k], u[4 * j + k], lse_c, lse_u, scale);
      if (i0 + 3 < V) {
        *(f32x4*)(out + i0) = o;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (i0 + k < V) out[i0 + k] = o[k];
      }
    }
    return;
  }

  float mc = -INFINITY, mu = -INFINITY;
  for (int i = tid; i < V; i += kCfgThreads) {
    mc = fmaxf(mc, cond[i]);
    mu = fmaxf(mu, unc[i]);
  }
  cfg_block_max2(mc, mu, sh);
  float zc = 0.f, zu = 0.f;
  for (int i = tid; i < V; i += kCfgThreads) {
    zc += expf(cond[i] - mc);
    zu += expf(unc[i] - mu);
  }
  cfg_block_sum2(zc, zu, sh);
  const float lse_c = mc + logf(zc), lse_u = mu + logf(zu);
  if (tid == 0 && row.lse_out != nullptr) {
    row.lse_out[0] = lse_c;
    row.lse_out[1] = lse_u;
  }
  const float thr = mc + row.log_beta;
  const bool want_mask = row.mask_out != nullptr;
  for (int b0 = 0; b0 < V; b0 += kCfgThreads) {     // a block-uniform trip count: every lane reaches the ballot
    const int i = b0 + tid;
    const bool in = i < V;
    const float ci = in ? cond[i] : 0.f;
    const float ui = in ? unc[i] : 0.f;
    if (want_mask) {
      const unsigned long long bal = __ballot((!in) | (ci >= thr));
      const int w = ((b0 + 64 * wave) >> 5) + (lane >> 5);
      if ((lane & 31) == 0 && w < W) row.mask_out[w] = (uint32_t)(bal >> (lane & 32)) & cfg_base_word(row.base, w, W, V);
    }
    if (in) out[i] = cfg_blend(ci, ui, lse_c, lse_u, scale);
  }
}

}  // namespace

int vt_cfg_rows_launch(const vt_cfg_row* rows, int n_rows, int V, hipStream_t s) {
  VT_REQUIRE(rows != nullptr, "vt_cfg_rows: rows is NULL");
  VT_REQUIRE(n_rows > 0, "vt_cfg_rows: n_rows=%d (n_rows > 0)", n_rows);
  VT_REQUIRE(V > 0 && V <= VT_LOGPROB_MAX_V, "vt_cfg_rows: V=%d (0 < V <= %d)", V, VT_LOGPROB_MAX_V);
  VT_REQUIRE(((uintptr_t)rows % 8) == 0, "vt_cfg_rows: rows must be 8-byte aligned");
  if (V <= 32 * 1024)
    hipLaunchKernelGGL(cfg_rows_kernel<true>, dim3(n_rows), dim3(kCfgThreads), 0, s, rows, V);
  else
    hipLaunchKernelGGL(cfg_rows_kernel<false>, dim3(n_rows), dim3(kCfgThreads), 0, s, rows, V);
  VT_LAUNCH_CHECK();
  return VT_OK;
}
