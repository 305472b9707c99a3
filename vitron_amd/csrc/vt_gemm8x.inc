// vt_gemm8x.inc -- gemm_w4x_kernel: the four-wave 256x256x64 GEMM of vt_gemm8.hip with a SECOND, 4-bit product folded into the same
// accumulators:  C = epi( A.W^T  +  (A4 . 2^ea) . (W4 . 2^ew)^T ),  A, W 16 bit on v_mfma_f32_16x16x32, A4 / W4 MX-FP4 images (vt_mx4.hip) of
// the rounding remainder of A and of W on v_mfma_scale_f32_16x16x128_f8f6f4 -- precise level 3 (DESIGN.md 4). Included by vt_gemm8.hip
// inside its anonymous namespace (shares GemmP8, the epilogues and the DMA helpers).
//
// The MX instruction covers K = 128, so the 4-bit product is taken once per PAIR of K steps: 64 more MFMAs behind the 2 x 128 of the pair
// (+25 % issue slots; the matrix pipe runs them at the same 16 cycles each -- tools/mx_probe.hip: a 4:1 mix costs 1.11x of the 16-bit
// stream on this power-limited part), 8 more LDS-DMA pieces against 32, 16 more fragment reads against 64.
//   LDS: the two 64 KiB K-step buffers of the base kernel + ONE 32 KiB image of the pair's 4-bit tiles (A4 256 rows x 64 B, then W4): 160 KiB,
//   the whole CU. A row of 64 B is four 16-byte chunks, chunk g of row r stored at position g ^ ((-(r >> 2)) & 3): the ds_read_b128 of a
//   fragment (lane = row r % 16, chunk g = lane >> 4) is conflict free in every 16-lane group the hardware forms, and the DMA applies
//   the same XOR on the source side (a piece = 16 rows x 64 B, lane-linear in LDS).
//   Schedule, on top of the base kernel's gap table (K step B = 0, then B = 1, then the 4-bit section "X"):
//     B = 1, gaps 95, 97 .. 125   read the 8 W4 + 8 A4 fragments of this pair           127: lgkmcnt(0)
//     X gap 0                     barrier -> the 4-bit image is free
//     X gaps 1, 3 .. 15           DMA the 8 pieces of the NEXT pair's 4-bit tiles
//     X gap 63                    the two scale dwords of the next pair (buffer loads into the registers the last MX MFMA has just read)
//   vmcnt: the 10 loads of X are older than everything the following K step issues, so its two counted waits grow by 10 (29 / 26
//   instead of 19 / 16); in the step after that (B = 1) they are older than the pieces the waits let fly, so the unchanged waits cover
//   them: the wave's own pieces of the 4-bit tiles have landed at gap 62 of B = 1, the barrier at 63 publishes them, the reads start at 95.
//   Scales: W4 has one exponent per output feature (two dwords per lane, fetched once); A4 one per (row, 32 k) in the layout vt_mx4.hip
//   writes: the dword a lane fetches holds the scales of its row in four consecutive 16-row fragments, picked by the instruction's op_sel.
struct GemmMx {
  const uint8_t* A4;
  const uint8_t* aexp;
  const uint8_t* W4;
  const uint8_t* wexp;
  uint8_t* out4;       // VT_EPI_SWIGLU_MX: the output's own 4-bit image [M][N / 4] ...
  uint8_t* oexp;       // ... and its block exponents (the layout of aexp, K := N / 2): the next GEMM's A4 / aexp
};

typedef __attribute__((ext_vector_type(4))) int i32x4;

// Activation epilogues with the level 3 operand out: C = op16(v) AND the MX-FP4 image of the remainder v - f32(C) (the next GEMM's second
// operand), both parked in LDS row by row and stored as 16-byte row pieces.
//   ACT 2 (VT_EPI_SWIGLU_MX): v = silu(gate) * up over the 16-interleaved gate / up columns -- a wave's 128 x 128 accumulators give 128 rows
//         x 64 outputs = two 32-blocks per row;
//   ACT 0 / 1 (VT_EPI_GELU_MX / VT_EPI_QGELU_MX): v = act(acc + bias) -- 128 rows x 128 outputs = four 32-blocks per row (the towers' fc1).
// A block's 32 values sit in the 4 lanes (lane >> 4) of a row, 8 each (two 16-column fragments x 4 columns).
template <int MT, int ACT>
__device__ __forceinline__ void w4x_epilogue_act_mx(const GemmP8& p, const GemmMx& x, f32x4 (&acc)[MT][8], int bm0, int bn0, int wr, int wc,
                                                    int lane, char* smem, int wave) {
  constexpr bool SW = ACT == 2;
  constexpr int NF = SW ? 4 : 8;                 // 16-column output fragments per row and wave
  constexpr int NB = NF / 2;                     // 32-blocks per row and wave
  constexpr int ROWB = NF * 32, CH = ROWB / 16, RPI = 64 / CH;
  constexpr int ROW4 = NF * 8;                   // bytes of codes per row and wave
  char* const my = smem + wave * (MT * 16 * ROWB);
  char* const my4 = smem + 4 * (MT * 16 * ROWB) + wave * (MT * 16 * ROW4);
  const int r16 = lane & 15, cg = lane >> 4;
  bf16_t* const C = (bf16_t*)p.C;
  const int ncol0 = SW ? ((bn0 >> 1) + wc * 64) : (bn0 + wc * 128);
  const int nout = SW ? (p.N >> 1) : p.N;
  const int KB = nout >> 5;
  const int rg0 = (bm0 + wr * (MT * 16)) >> 6;
  f32x4 b4[8];
  if constexpr (!SW) {
#pragma unroll
    for (int ni = 0; ni < 8; ++ni)
      b4[ni] = p.bias ? *(const f32x4*)(p.bias + min(bn0 + wc * 128 + ni * 16 + (cg << 2), p.N - 4)) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  __builtin_amdgcn_s_barrier();
  uint32_t eb[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) eb[b] = 0u;
#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
    const int row = mi * 16 + r16;
    float lo[NF][4];
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      float v[4];
      if constexpr (SW) {
        const f32x4 g = acc[mi][2 * nf], u2 = acc[mi][2 * nf + 1];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = silu8(g[j]) * u2[j];
      } else {
        const f32x4 a = acc[mi][nf] + b4[nf];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ACT == 0 ? gelu_erf8(a[j]) : quick_gelu8(a[j]);
      }
      u32x2 o;
      o.x = pack_op2(v[0], v[1]);
      o.y = pack_op2(v[2], v[3]);
      *(u32x2*)(my + row * ROWB + (((nf * 2 + (cg >> 1)) ^ (row & (CH - 1))) << 4) + (cg & 1) * 8) = o;
      lo[nf][0] = v[0] - oplo_to_f32(o.x);
      lo[nf][1] = v[1] - ophi_to_f32(o.x);
      lo[nf][2] = v[2] - oplo_to_f32(o.y);
      lo[nf][3] = v[3] - ophi_to_f32(o.y);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float amax = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) amax = fmaxf(amax, fmaxf(fabsf(lo[2 * b][j]), fabsf(lo[2 * b + 1][j])));
      amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
      amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
      const int e = mx4_exponent(amax);
      const float sc = mx4_scale(e);
      *(uint16_t*)(my4 + row * ROW4 + b * 16 + cg * 2) = (uint16_t)mx4_pack4(lo[2 * b][0], lo[2 * b][1], lo[2 * b][2], lo[2 * b][3], sc);
      *(uint16_t*)(my4 + row * ROW4 + b * 16 + 8 + cg * 2) = (uint16_t)mx4_pack4(lo[2 * b + 1][0], lo[2 * b + 1][1], lo[2 * b + 1][2], lo[2 * b + 1][3], sc);
      eb[b] |= (uint32_t)(e + 127) << (8 * (mi & 3));
    }
    if ((mi & 3) == 3) {   // the exponents of four 16-row fragments = one dword per (64-row group, block) and row % 16
      if (cg == 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
          if (ncol0 + b * 32 < nout) *(uint32_t*)(x.oexp + ((size_t)(rg0 + (mi >> 2)) * KB + (ncol0 >> 5) + b) * 64 + r16 * 4) = eb[b];
      }
#pragma unroll
      for (int b = 0; b < NB; ++b) eb[b] = 0u;
    }
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
  const int m_base = bm0 + wr * (MT * 16);
#pragma unroll
  for (int j = 0; j < MT * 16 / RPI; ++j) {
    const int row = j * RPI + lane / CH, ck = lane % CH;
    const u32x4 d = *(const u32x4*)(my + row * ROWB + ((ck ^ (row & (CH - 1))) << 4));
    const int m = m_base + row, n = ncol0 + ck * 8;
    if (m < p.M && n < nout) *(u32x4*)(C + (size_t)m * p.ldc + n) = d;
  }
  constexpr int L4 = ROW4 / 16;                  // lanes per row of codes
#pragma unroll
  for (int j = 0; j < MT * 16 * L4 / 64; ++j) {
    const int row = j * (64 / L4) + lane / L4, part = lane % L4;
    const u32x4 d = *(const u32x4*)(my4 + row * ROW4 + part * 16);
    const int m = m_base + row, n = ncol0 + part * 32;
    if (m < p.M && n < nout) *(u32x4*)(x.out4 + (size_t)m * (nout >> 1) + (n >> 1)) = d;
  }
}

template <int EPI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void gemm_w4x_kernel(GemmP8 p, GemmMx x) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int MT = 8;
  constexpr int BM = MT * 32;
  constexpr int A_BYTES = BM * 128, B_BYTES = 256 * 128, BUFB = A_BYTES + B_BYTES;
  constexpr int LOB = 2 * BUFB, LO_A = BM * 64;      // the 4-bit image: A4 rows, then W4 rows
  constexpr int NPA = MT, NPB = 8, NP = NPA + NPB;
  constexpr int H = MT * 8, NM = 2 * H;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave >> 1, wc = wave & 1;

  const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + 255) / 256;
  const int nwg = tiles_m * tiles_n;
  const int ksplit = (EPI == VT_EPI_F32) ? p.ksplit : 1;
  const int split = (ksplit > 1) ? (int)blockIdx.x / nwg : 0;
  const int sid = xcd_remap((int)blockIdx.x - split * nwg, nwg);
  const int ku = p.K >> 7;
  const int u_begin = (int)((long)ku * split / ksplit), u_end = (int)((long)ku * (split + 1) / ksplit);
  const int GROUP_M = W4_KNOB(3, 8);   // (measured with the knob, round 6: gate/up 836 us at 8, 848 at 4; qkv 474 / 467 -- this kernel keeps 8)
  const int per_group = GROUP_M * tiles_n;
  const int first_m = (sid / per_group) * GROUP_M;
  const int gsz = min(tiles_m - first_m, GROUP_M);
  const int tm = first_m + (sid % per_group) % gsz;
  const int tn = (sid % per_group) / gsz;
  const int bm0 = tm * BM, bn0 = tn * 256;
  const int ld4 = p.K >> 1, KB = p.K >> 5;          // bytes per row of A4 / W4, 32-blocks per row

  const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc((void*)(p.A + (size_t)bm0 * p.lda + u_begin * 128), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_b = __builtin_amdgcn_make_buffer_rsrc((void*)(p.W + (size_t)bn0 * p.ldw + u_begin * 128), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_a4 = __builtin_amdgcn_make_buffer_rsrc((void*)(x.A4 + (size_t)bm0 * ld4 + u_begin * 64), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_b4 = __builtin_amdgcn_make_buffer_rsrc((void*)(x.W4 + (size_t)bn0 * ld4 + u_begin * 64), 0, 0x7fffffff, 0x00020000);
  // this wave's two 64-row groups of the A4 scales: [m / 64][kb][m % 16][(m % 64) / 16]
  const __amdgpu_buffer_rsrc_t rsrc_ae =
      __builtin_amdgcn_make_buffer_rsrc((void*)(x.aexp + ((size_t)((bm0 >> 6) + wr * 2) * KB + u_begin * 4) * 64), 0, 0x7fffffff, 0x00020000);
  const int lrow = lane >> 3, lchk = lane & 7;
  int voff[16];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int row = (i < NPB ? wave * NPB + i : wave * NPA + (i - NPB)) * 8 + lrow;
    const int coff = (lchk ^ ((row >> 1) & 7)) * 16;
    voff[i] = i < NPB ? (min(bn0 + row, p.N - 1) - bn0) * p.ldw * 2 + coff : (min(bm0 + row, p.M - 1) - bm0) * p.lda * 2 + coff;
  }
  int voff4[8];   // pieces 0..3: A4 rows (wave * 4 + j) * 16 + lane / 4, pieces 4..7: the same rows of W4
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = (wave * 4 + j) * 16 + (lane >> 2);
    const int coff = ((lane & 3) ^ ((-(row >> 2)) & 3)) * 16;
    voff4[j] = (min(bm0 + row, p.M - 1) - bm0) * ld4 + coff;
    voff4[4 + j] = (min(bn0 + row, p.N - 1) - bn0) * ld4 + coff;
  }
  const int voff_ae = (lane >> 4) * 64 + (lane & 15) * 4;   // + h * KB * 64 for the second group
#define W4S_DMA_X(BUF, P, KB_, AUX)                                                                               \
  __builtin_amdgcn_raw_ptr_buffer_load_lds(                                                                      \
      (P) < NPB ? rsrc_b : rsrc_a,                                                                               \
      (__attribute__((address_space(3))) void*)(smem + (BUF) * BUFB +                                            \
                                                 ((P) < NPB ? A_BYTES + (wave * NPB + (P)) * 1024 : (wave * NPA + (P) - NPB) * 1024)), \
      16, voff[P], KB_, 0, AUX)
#define W4S_DMA(BUF, P, KB_) W4S_DMA_X(BUF, P, KB_, 0)
  // piece P of the 4-bit image of pair U (byte offset U * 64 along K)
#define W4X_DMA4(P, KO)                                                                                          \
  __builtin_amdgcn_raw_ptr_buffer_load_lds(                                                                      \
      (P) < 4 ? rsrc_a4 : rsrc_b4,                                                                               \
      (__attribute__((address_space(3))) void*)(smem + LOB + ((P) < 4 ? 0 : LO_A) + (wave * 4 + ((P) & 3)) * 1024), 16, voff4[P], KO, 0, 0)

  const int f = (lane >> 1) & 7;
  const int fo[2] = {(lane & 15) * 128 + (((lane >> 4) ^ f) << 4), (lane & 15) * 128 + ((((lane >> 4) | 4) ^ f) << 4)};
  const int a_base = wr * (MT * 16 * 128);
  const int b_base = A_BYTES + wc * (128 * 128);
  const int fo4 = (lane & 15) * 64 + ((((lane >> 4) ^ (-((lane & 15) >> 2))) & 3) << 4);
  const int a4_base = LOB + wr * (128 * 64) + fo4;
  const int b4_base = LOB + LO_A + wc * (128 * 64) + fo4;

  f32x4 acc[MT][8];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int ni = 0; ni < 8; ++ni) acc[mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
  bf16x8 fa[2][MT], fb[2][8];
  i32x4 fa4[MT], fb4[8];
  int sa[2], sb[2];
  // W4 scales: one byte per output feature; the lane's row of fragment ni is bn0 + wc * 128 + ni * 16 + lane % 16
  {
    uint32_t w0 = 0, w1 = 0;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      w0 |= (uint32_t)x.wexp[min(bn0 + wc * 128 + ni * 16 + (lane & 15), p.N - 1)] << (8 * ni);
      w1 |= (uint32_t)x.wexp[min(bn0 + wc * 128 + (ni + 4) * 16 + (lane & 15), p.N - 1)] << (8 * ni);
    }
    sb[0] = (int)w0;
    sb[1] = (int)w1;
  }
#define W4S_MFMA(N)                                                                                              \
  asm volatile(VT_MFMA_16x16x32_ASM " %0, %1, %2, %0"                                                            \
               : "+a"(acc[(((N) % H) >> 3) & 7][(N) & 7]) : "v"(fb[((N) / H) & 1][(N) & 7]), "v"(fa[((N) / H) & 1][(((N) % H) >> 3) % MT]))
  // MX MFMA j of the 4-bit section: accumulator row j >> 3, column j & 7; srcA = W4 fragment (scale: byte ni % 4 of sb[ni / 4]),
  // srcB = A4 fragment (scale: byte mi % 4 of sa[mi / 4])
#define W4X_MFMA(J)                                                                                              \
  asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel:[%5,%6,0] op_sel_hi:[%7,%8,0] cbsz:4 blgp:4" \
               : "+a"(acc[((J) >> 3) & 7][(J) & 7])                                                              \
               : "v"(fb4[(J) & 7]), "v"(fa4[((J) >> 3) & 7]), "v"(sb[((J) >> 2) & 1]), "v"(sa[((J) >> 5) & 1]),  \
                 "n"((J) & 1), "n"(((J) >> 3) & 1), "n"(((J) >> 1) & 1), "n"(((J) >> 4) & 1))
#define W4S_RDB(SET, BUF, KK, I) fb[SET][I] = *(const bf16x8*)(smem + (BUF) * BUFB + b_base + fo[KK] + (I) * 2048)
#define W4S_RDA(SET, BUF, KK, I) fa[SET][I] = *(const bf16x8*)(smem + (BUF) * BUFB + a_base + fo[KK] + (I) * 2048)
#define W4X_RDB4(I) fb4[I] = *(const i32x4*)(smem + b4_base + (I) * 1024)
#define W4X_RDA4(I) fa4[I] = *(const i32x4*)(smem + a4_base + (I) * 1024)
#define W4X_SCALES(KO)                                                                                           \
  do {                                                                                                           \
    sa[0] = __builtin_amdgcn_raw_buffer_load_b32(rsrc_ae, voff_ae, KO, 0);                                   \
    sa[1] = __builtin_amdgcn_raw_buffer_load_b32(rsrc_ae, voff_ae + KB * 64, KO, 0);                         \
  } while (0)
#define W4S_LGKM0() __builtin_amdgcn_s_waitcnt(0xc07f)

  const int nt = (u_end - u_begin) * 2;            // K steps of this workgroup's K range
  const int np = u_end - u_begin;                  // pairs
  const int kb1 = min(1, nt - 1) * 128;
#pragma unroll
  for (int i = 0; i < NP; ++i) W4S_DMA(0, i, 0);
#pragma unroll
  for (int i = 0; i < NP; ++i) W4S_DMA(1, i, kb1);
#pragma unroll
  for (int i = 0; i < 8; ++i) W4X_DMA4(i, 0);
  W4X_SCALES(0);
  __builtin_amdgcn_s_waitcnt(w4_vmcnt_imm(NP + 10));   // K step 0 has landed; K step 1 and the 4-bit image of pair 0 may be in flight
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < 8; ++i) W4S_RDB(0, 0, 0, i);
#pragma unroll
  for (int i = 0; i < MT; ++i) W4S_RDA(0, 0, 0, i);
  W4S_LGKM0();
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 4");

  constexpr int S1_N = NPB + MT;
  constexpr int LG2 = 21 + 2 * S1_N + 2, BAR2 = LG2 + 1;    // 55, 56
  constexpr int NE = 3;
  constexpr int VM3 = BAR2 + 2 * NE, BAR3 = VM3 + 1;        // 62, 63
  constexpr int VM4 = 92, BAR4 = VM4 + 1;                   // 92, 93
#define W4S_IX(x_, m_) ((((x_) % (m_)) + (m_)) % (m_))
  // the base kernel's gap table; B = 0 waits leave the 10 loads of the preceding 4-bit section in flight too
#define W4S_GAP(n, B, KB_)                                                                                       \
  do {                                                                                                           \
    if ((n) < 16) { if (!((n) & 1)) W4S_RDB(1, B, 1, ((n) >> 1) & 7); }                                          \
    else if ((n) == 19 || (n) == LG2) { W4S_LGKM0(); }                                                           \
    else if ((n) == 20 || (n) == BAR2 || (n) == BAR3 || (n) == BAR4) { __builtin_amdgcn_s_barrier(); }           \
    else if ((n) >= 21 && (n) < 21 + 2 * S1_N) {                                                                 \
      if ((n) & 1) {                                                                                             \
        if ((((n) - 21) >> 1) >= 16) { W4S_RDA(1, B, 1, W4S_IX((((n) - 21) >> 1) - 8, MT)); }                    \
        else if (((n) & 3) == 1) { W4S_DMA(B, W4S_IX(((n) - 21) >> 2, 8), KB_); }                                \
        else { if ((((n) - 23) >> 2) < MT) W4S_RDA(1, B, 1, W4S_IX(((n) - 23) >> 2, MT)); }                      \
      }                                                                                                          \
    }                                                                                                            \
    else if ((n) > BAR2 && (n) < VM3) { if (((n) - BAR2) & 1) { W4S_DMA(B, NPB + W4S_IX(((n) - BAR2) >> 1, NE), KB_); } } \
    else if ((n) == VM3) { __builtin_amdgcn_s_waitcnt(w4_vmcnt_imm(NPA + NPB + NE + ((B) == 0 ? 10 : 0))); }     \
    else if ((n) >= H && (n) < VM4) {                                                                            \
      if (!(((n) - H) & 1)) { if ((n) <= H + 14) W4S_RDB(0, (B) ^ 1, 0, W4S_IX(((n) - H) >> 1, 8)); }            \
      else if ((((n) - H) & 3) == 1 && (((n) - H) >> 2) < NPA - NE) { W4S_DMA(B, NPB + NE + W4S_IX(((n) - H) >> 2, NPA - NE), KB_); } \
    }                                                                                                            \
    else if ((n) == VM4) { __builtin_amdgcn_s_waitcnt(w4_vmcnt_imm(NPA + NPB + ((B) == 0 ? 10 : 0))); }          \
    else if ((n) > BAR4 && (n) <= BAR4 + 2 * MT && (((n) - BAR4) & 1)) { W4S_RDA(0, (B) ^ 1, 0, W4S_IX(((n) - BAR4) >> 1, MT)); } \
    if ((B) == 1 && (n) >= 95 && (n) <= 125 && ((n) & 1)) {                                                      \
      if ((((n) - 95) >> 1) < 8) W4X_RDB4(W4S_IX(((n) - 95) >> 1, 8)); else W4X_RDA4(W4S_IX((((n) - 95) >> 1) - 8, 8)); \
    }                                                                                                            \
    if ((B) == 1 && (n) == 127) W4S_LGKM0();                                                                     \
  } while (0)
#define W4X_GAP(j, KO)                                                                                           \
  do {                                                                                                           \
    if ((j) == 0) __builtin_amdgcn_s_barrier();                                                                  \
    else if ((j) < 16 && ((j) & 1)) W4X_DMA4(W4S_IX((j) >> 1, 8), KO);                                           \
    else if ((j) == 63) W4X_SCALES((KO) * 4);                                                                    \
  } while (0)
#define W4S_N(n, B, KB_) W4S_MFMA(n); W4S_GAP(n, B, KB_); __builtin_amdgcn_sched_barrier(0);
#define W4S_8(n, B, KB_) W4S_N((n), B, KB_) W4S_N((n) + 1, B, KB_) W4S_N((n) + 2, B, KB_) W4S_N((n) + 3, B, KB_) \
                         W4S_N((n) + 4, B, KB_) W4S_N((n) + 5, B, KB_) W4S_N((n) + 6, B, KB_) W4S_N((n) + 7, B, KB_)
#define W4S_32(n, B, KB_) W4S_8((n), B, KB_) W4S_8((n) + 8, B, KB_) W4S_8((n) + 16, B, KB_) W4S_8((n) + 24, B, KB_)
#define W4S_KSTEP(B, T)                                                                                          \
  do {                                                                                                           \
    const int _kb = min((T) + 2, nt - 1) * 128;                                                                  \
    W4S_32(0, B, _kb) W4S_32(32, B, _kb) W4S_32(64, B, _kb) W4S_32(96, B, _kb)                                    \
  } while (0)
#define W4X_N(j, KO) W4X_MFMA(j); W4X_GAP(j, KO); __builtin_amdgcn_sched_barrier(0);
#define W4X_8(j, KO) W4X_N((j), KO) W4X_N((j) + 1, KO) W4X_N((j) + 2, KO) W4X_N((j) + 3, KO) \
                     W4X_N((j) + 4, KO) W4X_N((j) + 5, KO) W4X_N((j) + 6, KO) W4X_N((j) + 7, KO)
#define W4X_SECTION(U)                                                                                           \
  do {                                                                                                           \
    const int _ko = min((U) + 1, np - 1) * 64;     /* past the end of K: re-fetch the last pair, harmless */      \
    W4X_8(0, _ko) W4X_8(8, _ko) W4X_8(16, _ko) W4X_8(24, _ko) W4X_8(32, _ko) W4X_8(40, _ko) W4X_8(48, _ko) W4X_8(56, _ko) \
  } while (0)
  for (int t = 0; t < nt; t += 2) {
    W4S_KSTEP(0, t);
    W4S_KSTEP(1, t + 1);
    W4X_SECTION(t >> 1);
    VT_MFMA_TAIL_WAIT(t + 2 >= nt);              // (vt_gemm8.hip: the wait states for the last MFMAs, on the loop's last trip)
  }
  VT_VMCNT(0);
  asm volatile("s_nop 15\n\ts_nop 7");
#undef W4X_SECTION
#undef W4X_8
#undef W4X_N
#undef W4S_KSTEP
#undef W4S_32
#undef W4S_8
#undef W4S_N
#undef W4X_GAP
#undef W4S_GAP
#undef W4S_IX
#undef W4S_LGKM0
#undef W4X_SCALES
#undef W4X_RDA4
#undef W4X_RDB4
#undef W4S_RDA
#undef W4S_RDB
#undef W4X_MFMA
#undef W4S_MFMA
#undef W4X_DMA4
#undef W4S_DMA
#undef W4S_DMA_X
  constexpr bool bf16_store = vt_epi_op16_store(EPI);
  // The epilogue takes the lane id through an opaque copy: whatever it derives from it (row / column offsets, masks) is computed HERE, not hoisted
  // in front of the main loop -- where, with 256 + 256 registers taken, it was spilled between the prologue's DMA pieces and their counted
  // vmcnt wait (a scratch store counts in vmcnt and may retire out of order with the loads: the wait could return a piece early).
  // tests/test_host_logic.py checks the generated code for scratch accesses between the first DMA and the last MFMA.
  int lane_e = lane;
  asm volatile("" : "+v"(lane_e));
  if constexpr (EPI == VT_EPI_SWIGLU_MX) {
    w4x_epilogue_act_mx<MT, 2>(p, x, acc, bm0, bn0, wr, wc, lane_e, smem, wave);
  } else if constexpr (EPI == VT_EPI_GELU_MX) {
    w4x_epilogue_act_mx<MT, 0>(p, x, acc, bm0, bn0, wr, wc, lane_e, smem, wave);
  } else if constexpr (EPI == VT_EPI_QGELU_MX) {
    w4x_epilogue_act_mx<MT, 1>(p, x, acc, bm0, bn0, wr, wc, lane_e, smem, wave);
  } else if constexpr (bf16_store) {
    w4_epilogue_lds<EPI, MT>(p, acc, bm0, bn0, wr, wc, lane_e, smem, wave);
  } else {
    w4_epilogue<EPI, MT>(p, acc, bm0, bn0, wr, wc, lane_e, split);
  }
}

template <int EPI>
int launch_w4x(const GemmP8& p, const GemmMx& x, hipStream_t s) {
  constexpr int smem = 2 * (256 * 128 + 256 * 128) + 2 * 256 * 64;   // 160 KiB: the whole CU
  auto kern = gemm_w4x_kernel<EPI>;
  w4_knobs_once();
  VT_LDS_ATTR_ONCE(kern, smem);
  hipLaunchKernelGGL(kern, dim3(cdiv(p.M, 256) * cdiv(p.N, 256) * (EPI == VT_EPI_F32 ? std::max(p.ksplit, 1) : 1)), dim3(256), smem, s, p, x);
  VT_LAUNCH_CHECK();
  return VT_OK;
}
