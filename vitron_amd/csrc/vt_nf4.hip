// vt_nf4.hip -- NF4 weight-only decoder Linears (load_4bit: reference vitron/model/builder.py:36-45, bitsandbytes
// BitsAndBytesConfig(load_in_4bit=True, bnb_4bit_quant_type="nf4", bnb_4bit_compute_dtype=float16)).
//
// Format (restated from bitsandbytes' algorithm; tests/nf4_ref.py is the numpy restatement the tests compare bytes against):
//   * the weight is taken as fp16 (transformers 4.31 loads 4-bit models in fp16), in blocks of 64 consecutive elements of the
//     row-major [N][K] matrix (K % 64 == 0: a block never straddles a row, so per-row quantisation == bnb's flat one);
//   * absmax = fp32 max |x| of the block; the normalised value x * (1.0f / absmax) goes to the NF4 code whose fp32 midpoints it
//     lies strictly above (bnb dQuantizeNF4); an all-zero block stores absmax 0 and code 7 (0.0) everywhere;
//   * codes packed two per byte, element 2j in the high nibble, 2j+1 in the low one; absmax stays exact fp32 (bnb's layout with
//     bnb_4bit_use_double_quant off -- the reference turns it on);
//   * dequantised weight = op16(fp32(code) * absmax).
// The GEMM reads bnb's layout as it is (codes [N][K/2], absmax [N][K/64]): the "kernel layout" is the bnb order.
//
// GEMM (M <= 32 rows: decode steps, padded-batch fix-up rows, short prefills): C = epi(A . dequant(W)^T), fp32 accumulation.
//   * a block of 8 waves owns 32 weight rows (two 16-row tiles; for SwiGLU one gate + one up block of the interleaved wgu) and
//     splits K eight ways; every wave walks its K range in 128-wide steps with the next step's codes / scales / activations
//     already in flight (register double buffer), reads each weight byte from HBM exactly once (non-temporal),
//   * dequantisation in registers: a 256-entry LDS table byte -> (code_hi, code_lo) as two fp32, one v_pk_mul by the block's absmax,
//     one packed convert to the operand format -- the same op16(code * absmax) vt_nf4_dequant writes, so the decode GEMM and the
//     prefill (dequantised weights on the tile GEMMs) see identical weights,
//   * the products on v_mfma_f32_16x16x32 (weights as "A", activations as "B": lane holds D[n = 4*(lane>>4)+r][m = lane&15]);
//     lane (r = lane&15, g = lane>>4) takes k = 32 g .. 32 g + 31 of the step for its row, the activations the same k,
//   * split-K reduce through LDS, then the epilogues of the decode loop with the folded RMSNorm of vt_gemm_skinny_norm_launch
//     (VtGemmNormFuse: consumer sums in_partials per row; producer writes out_xw and per-16-column partial sums, [M][N/16]).
#include "vt_common.h"
#include "vt_kernels.h"

namespace {

__constant__ float kNf4Code[16] = {-1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f, -0.28444138169288635f,
                                   -0.18477343022823334f, -0.09105003625154495f, 0.0f, 0.07958029955625534f, 0.16093020141124725f,
                                   0.24611230194568634f, 0.33791524171829224f, 0.44070982933044434f, 0.5626170039176941f,
                                   0.7229568362236023f, 1.0f};
// bnb's dQuantizeNF4 thresholds, ascending: code = number of them the normalised value is strictly above
__constant__ float kNf4Mid[15] = {-0.8480964004993439f, -0.6106329262256622f, -0.4599952697753906f, -0.33967943489551544f,
                                  -0.23460740596055984f, -0.13791173323988914f, -0.045525018125772476f, 0.03979014977812767f,
                                  0.1202552504837513f, 0.2035212516784668f, 0.2920137718319893f, 0.3893125355243683f,
                                  0.5016634166240692f, 0.6427869200706482f, 0.8614784181118011f};

// the weight as bnb sees it: cast to fp16 (round to nearest even), back to fp32 exactly
template <int SRC>
__device__ __forceinline__ float nf4_src(const void* W, size_t i) {
  float v;
  if constexpr (SRC == VT_DTYPE_F32) v = ((const float*)W)[i];
  else v = op_to_f32(((const op16_t*)W)[i]);
  return (float)(_Float16)v;
}

// one wave per 64-element block: lane = element; the even lane of a pair writes the byte
template <int SRC>
__global__ __launch_bounds__(256) void nf4_quant_kernel(const void* __restrict__ W, int ldw, int N, int K, uint8_t* __restrict__ codes,
                                                        float* __restrict__ absmax) {
  const int lane = threadIdx.x & 63;
  const long blk = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int bpr = K >> 6;
  if (blk >= (long)N * bpr) return;
  const int n = (int)(blk / bpr), kb = (int)(blk % bpr);
  const float x = nf4_src<SRC>(W, (size_t)n * ldw + (size_t)kb * 64 + lane);
  const float amax = wave_max(fabsf(x));
  int code = 7;
  if (amax > 0.f) {
    const float y = x * __frcp_rn(amax);
    code = 0;
#pragma unroll
    for (int t = 0; t < 15; ++t) code += (y > kNf4Mid[t]) ? 1 : 0;
  }
  const int other = __shfl_xor(code, 1, 64);
  if ((lane & 1) == 0) codes[(size_t)blk * 32 + (lane >> 1)] = (uint8_t)((code << 4) | other);
  if (lane == 0) absmax[blk] = amax;
}

// one thread per code byte -> two operand elements
__global__ __launch_bounds__(256) void nf4_dequant_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ absmax, int N, int K,
                                                          op16_t* __restrict__ W, int ldw) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int half = K >> 1;
  if (i >= (size_t)N * half) return;
  const int n = (int)(i / half), j = (int)(i % half);
  const unsigned b = codes[i];
  const float s = absmax[i >> 5];
  const uint32_t o = pack_op2(kNf4Code[b >> 4] * s, kNf4Code[b & 15] * s);
  *(uint32_t*)(W + (size_t)n * ldw + 2 * j) = o;
}

struct Nf4P {
  const op16_t* A;
  const uint8_t* codes;
  const float* absmax;
  void* C;
  int M, N, K, lda, ldc;
  VtGemmNormFuse nf;
};

// code byte pair -> packed operand pair, exactly op16(code * absmax) (|code * absmax| <= absmax, an fp16 value: no clamp needed)
__device__ __forceinline__ uint32_t nf4_pair(const float2* tab, uint32_t byte, float s) {
  const float2 c = tab[byte];
#if VT_OPERAND_F16
  return pack_f16x2(c.x * s, c.y * s);
#else
  return pack_op2(c.x * s, c.y * s);
#endif
}
// one dword of codes (8 elements) -> one MFMA fragment
__device__ __forceinline__ bf16x8 nf4_frag(const float2* tab, uint32_t d, float s) {
  u32x4 o;
  o.x = nf4_pair(tab, d & 0xffu, s);
  o.y = nf4_pair(tab, (d >> 8) & 0xffu, s);
  o.z = nf4_pair(tab, (d >> 16) & 0xffu, s);
  o.w = nf4_pair(tab, d >> 24, s);
  return __builtin_bit_cast(bf16x8, o);
}

__device__ __forceinline__ u32x4 load_nt16(const void* p) { return __builtin_nontemporal_load((const u32x4*)p); }

template <int EPI, int MB>
__global__ __launch_bounds__(512) void gemm_nf4_kernel(Nf4P p) {
  constexpr int NWAVE = 8, NT = 2;
  __shared__ float2 tab[256];
  __shared__ float red[NWAVE][NT * MB][256];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (threadIdx.x < 256) tab[threadIdx.x] = make_float2(kNf4Code[threadIdx.x >> 4], kNf4Code[threadIdx.x & 15]);

  const int n_base = blockIdx.x * 16 * NT;
  const int steps = p.K >> 7;
  const int s0 = (int)((long)steps * wave / NWAVE), s1 = (int)((long)steps * (wave + 1) / NWAVE);
  const int r = lane & 15, g = lane >> 4;
  const int kpr = p.K >> 6;   // absmax blocks per row
  const uint8_t* csrc[NT];
  const float* ssrc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int row = n_base + t * 16 + r;   // N % 32 == 0: always in range
    csrc[t] = p.codes + (size_t)row * (p.K >> 1) + g * 16;
    ssrc[t] = p.absmax + (size_t)row * kpr + (g >> 1);
  }
  const op16_t* xsrc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) xsrc[mb] = p.A + (size_t)min(mb * 16 + r, p.M - 1) * p.lda + g * 32;   // rows >= M: never stored

  u32x4 cw[NT];
  float sc[NT];
  bf16x8 xa[MB][4];
  auto fetch = [&](int st, u32x4* c, float* s, bf16x8 (*x)[4]) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      c[t] = load_nt16(csrc[t] + (size_t)st * 64);
      s[t] = ssrc[t][st * 2];
    }
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int q = 0; q < 4; ++q) x[mb][q] = *(const bf16x8*)(xsrc[mb] + (size_t)st * 128 + q * 8);
  };

  f32x4 acc[NT][MB];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[t][mb] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (s0 < s1) fetch(s0, cw, sc, xa);
  __syncthreads();   // the table
  for (int st = s0; st < s1; ++st) {
    u32x4 cn[NT];
    float sn[NT];
    bf16x8 xn[MB][4];
    if (st + 1 < s1) fetch(st + 1, cn, sn, xn);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const bf16x8 wf = nf4_frag(tab, cw[t][q], sc[t]);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[t][mb] = VT_MFMA_16x16x32(wf, xa[mb][q], acc[t][mb]);
      }
    }
    if (st + 1 < s1) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        cw[t] = cn[t];
        sc[t] = sn[t];
      }
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int q = 0; q < 4; ++q) xa[mb][q] = xn[mb][q];
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) *(f32x4*)&red[wave][t * MB + mb][lane * 4] = acc[t][mb];
  __syncthreads();

  // epilogue: thread (m = tid >> 4, nn = tid & 15); the 16 threads of a row are 16 consecutive lanes of one wave
  const int m = threadIdx.x >> 4, nn = threadIdx.x & 15;
  if (m >= MB * 16 || m >= p.M) return;
  const int mb = m >> 4, e = (((nn >> 2) * 16 + (m & 15)) << 2) + (nn & 3);
  float v[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    v[t] = 0.f;
#pragma unroll
    for (int w = 0; w < NWAVE; ++w) v[t] += red[w][t * MB + mb][e];
  }
  if (p.nf.in_partials) {   // folded RMSNorm, consumer side: row m's partial sums of squares -> rstd
    const int cnt = p.nf.in_n >> 4;
    const float* pp = p.nf.in_partials + (size_t)m * p.nf.in_n + nn * cnt;
    float ss = 0.f;
    for (int q = 0; q < cnt; ++q) ss += pp[q];
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) ss += __shfl_xor(ss, off, 16);
    const float rstd = rsqrtf(ss * p.nf.inv_dim + p.nf.eps);
#pragma unroll
    for (int t = 0; t < NT; ++t) v[t] *= rstd;
  }
  if constexpr (EPI == VT_EPI_SWIGLU_BF16) {   // rows n_base .. +15 gate, n_base + 16 .. +31 up
    ((op16_t*)p.C)[(size_t)m * p.ldc + blockIdx.x * 16 + nn] = f32_to_op(vt_silu(v[0]) * v[1]);
  } else {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int nc = n_base + t * 16 + nn;
      if constexpr (EPI == VT_EPI_F32_RESID) {
        float* c = (float*)p.C + (size_t)m * p.ldc + nc;
        const float x = *c + v[t];
        *c = x;
        if (p.nf.out_partials) {   // folded RMSNorm, producer side: y = op16(x .* w_next) and the 16 columns' sum of x^2
          p.nf.out_xw[(size_t)m * p.nf.ld_xw + nc] = f32_to_op(x * p.nf.out_w[nc]);
          float ss = x * x;
#pragma unroll
          for (int off = 1; off < 16; off <<= 1) ss += __shfl_xor(ss, off, 16);
          if (nn == 0) p.nf.out_partials[(size_t)m * (p.N >> 4) + blockIdx.x * NT + t] = ss;
        }
      } else if constexpr (EPI == VT_EPI_F32) {
        ((float*)p.C)[(size_t)m * p.ldc + nc] = v[t];
      } else {
        ((op16_t*)p.C)[(size_t)m * p.ldc + nc] = f32_to_op(v[t]);
      }
    }
  }
}

template <int EPI>
int launch_nf4(const Nf4P& p, hipStream_t s) {
  const dim3 grid(p.N / 32), block(512);
  if (p.M <= 16) hipLaunchKernelGGL((gemm_nf4_kernel<EPI, 1>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((gemm_nf4_kernel<EPI, 2>), grid, block, 0, s, p);
  VT_LAUNCH_CHECK();
  return VT_OK;
}

}  // namespace

int vt_nf4_quant_launch(const void* W, int src_dtype, int ldw, int N, int K, uint8_t* codes, float* absmax, hipStream_t s) {
  VT_REQUIRE(W && codes && absmax, "vt_nf4_quant: null pointer");
  VT_REQUIRE(N > 0 && K > 0 && (K % 64) == 0 && ldw >= K, "vt_nf4_quant: K = %d must be a positive multiple of 64 (N = %d, ldw = %d)", K, N, ldw);
  VT_REQUIRE(src_dtype == VT_DTYPE_OP16 || src_dtype == VT_DTYPE_F32, "vt_nf4_quant: source dtype %d unsupported", src_dtype);
  const long blocks = (long)N * (K >> 6);
  const dim3 grid((unsigned)((blocks + 3) / 4)), block(256);
  if (src_dtype == VT_DTYPE_F32) hipLaunchKernelGGL(nf4_quant_kernel<VT_DTYPE_F32>, grid, block, 0, s, W, ldw, N, K, codes, absmax);
  else hipLaunchKernelGGL(nf4_quant_kernel<VT_DTYPE_OP16>, grid, block, 0, s, W, ldw, N, K, codes, absmax);
  VT_LAUNCH_CHECK();
  return VT_OK;
}

int vt_nf4_dequant_launch(const uint8_t* codes, const float* absmax, int N, int K, bf16_t* W, int ldw, hipStream_t s) {
  VT_REQUIRE(codes && absmax && W, "vt_nf4_dequant: null pointer");
  VT_REQUIRE(N > 0 && K > 0 && (K % 64) == 0 && ldw >= K && (ldw % 2) == 0, "vt_nf4_dequant: K = %d must be a positive multiple of 64, ldw >= K even",
             K);
  const size_t threads = (size_t)N * (K >> 1);
  hipLaunchKernelGGL(nf4_dequant_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, codes, absmax, N, K, W, ldw);
  VT_LAUNCH_CHECK();
  return VT_OK;
}

int vt_gemm_nf4_launch(const bf16_t* A, int lda, const uint8_t* codes, const float* absmax, void* C, int ldc, int M, int N, int K, int epi,
                       const VtGemmNormFuse& nf, hipStream_t s) {
  VT_REQUIRE(A && codes && absmax && C, "vt_gemm_nf4: null pointer");
  VT_REQUIRE(M > 0 && M <= 32 && N > 0 && (N % 32) == 0 && K > 0 && (K % 128) == 0,
             "vt_gemm_nf4: needs 1 <= M <= 32, N %% 32 == 0, K %% 128 == 0 (M=%d N=%d K=%d)", M, N, K);
  VT_REQUIRE(lda >= K && (lda % 8) == 0 && ldc > 0, "vt_gemm_nf4: lda must be >= K and a multiple of 8");
  VT_REQUIRE(epi == VT_EPI_BF16 || epi == VT_EPI_F32 || epi == VT_EPI_F32_RESID || epi == VT_EPI_SWIGLU_BF16, "vt_gemm_nf4: epilogue %d unsupported",
             epi);
  if (nf.out_partials)
    VT_REQUIRE(epi == VT_EPI_F32_RESID && nf.out_w && nf.out_xw && nf.ld_xw >= N, "vt_gemm_nf4: producer side needs the residual epilogue, weights and the xw buffer");
  if (nf.in_partials)
    VT_REQUIRE(nf.in_n > 0 && (nf.in_n % 16) == 0 && nf.inv_dim > 0.f, "vt_gemm_nf4: consumer side needs in_n %% 16 == 0 (in_n=%d) and inv_dim", nf.in_n);
  Nf4P p{A, codes, absmax, C, M, N, K, lda, ldc, nf};
  VtProfScope prof(VT_PROF_GEMM_SKINNY, (double)N * (double)K * (0.5 + 4.0 / 64.0), s);
  return vt_with_epi<VtEpisDecode>(epi, "vt_gemm_nf4", [&](auto e) { return launch_nf4<decltype(e)::value>(p, s); });
}
