// vt_sample.hip -- the samplers: vt_sample_top_p with launch-uniform parameters, vt_sample_rows* with per-row ones. Two __device__
// bodies written once (the row in registers, or streamed at any V); one kernel template and one launch table over them for the
// vt_sample_rows family.
#include "vt_common.h"
#include "vt_kernels.h"
#include "vt_rows.h"

#include <cmath>
#include <vector>

namespace {

// vt_rows.h's (value, index) order in its branch form (see there why): the greedy rows' rule, which is argmax_kernel's (vt_llama.hip)
constexpr RowTakeIf take{};       // (a NaN is never taken)

// ---------------------------------------------------------------------------------------------------------------
// Temperature / top-k-free top-p sampling of one token per row, entirely on the device (no logits copy, no host sync):
//   p = softmax(logits / T);  keep the smallest set of highest-probability tokens whose mass reaches top_p -- exactly
//   transformers' TopPLogitsWarper rule (sort ascending, drop while cumulative mass <= 1 - top_p, always keep one) --
//   found by bisection on the probability threshold instead of a sort; then inverse-CDF sampling over the kept tokens in
//   index order with a counter-based uniform (splitmix64 of seed, step, row). One 1024-thread block per row.
// Replaces GenerationMixin.sample's warper + torch.multinomial (app.py:562-571 passes do_sample=True, temperature, top_p).
// The rule is written ONCE, as two __device__ bodies that read one row's parameters from a SampleArgs (sample_reg_body: the row in
// registers; sample_stream_body: any V). The vt_sample_top_p kernels fill SampleArgs from their launch-uniform scalars, the
// vt_sample_rows kernels from the row's vt_sample_row; their kRows instantiation adds the repetition penalty
// (RepetitionPenaltyLogitsProcessor), greedy rows and the chosen token's log-probability.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// multiplier of transformers' accumulate_hash (h <- (h + d) * M + 1 in wrapping 64-bit arithmetic): kWm, DESIGN.md 9.16
constexpr uint64_t kWmMul = 6364136223846793005ull;
// words of the kWm body's LDS block: the table's bits, three uint64 of state for the write-back, the low words of layer_add
constexpr int kWmStateWord = VT_WM_MAX_TABLE / 32, kWmLayerWord = kWmStateWord + 6, kWmLdsWords = kWmLayerWord + VT_WM_MAX_DEPTH;

// monotone map float -> uint32 (a < b  <=>  key(a) < key(b)); -inf maps below every finite value
__device__ __forceinline__ uint32_t order_key(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One row's sampling parameters as the two sampler bodies read them. vt_sample_top_p fills it from its launch-uniform scalars
// (stream = blockIdx.x: today's draw), vt_sample_rows from the row's vt_sample_row.
struct SampleArgs {
  float inv_temp;
  int top_k;
  float top_p;
  uint64_t seed, counter;
  uint32_t stream;
  bool greedy;            // first index of the maximum instead of a draw (kRows bodies only)
  float penalty;          // RepetitionPenaltyLogitsProcessor factor; applied to the ids of history[0..history_len) (kRows only)
  const int* history;
  int history_len;
};
__device__ __forceinline__ float sample_uniform24(const SampleArgs& a) {   // (0, 1): 24 bits of splitmix64(seed, counter, stream), centred
  const uint64_t r = splitmix64(a.seed ^ splitmix64(a.counter * 0x632be59bd9b4e019ull + a.stream));
  return (float)((r >> 40) + 0.5) * (1.0f / 16777216.0f);
}
// RepetitionPenaltyLogitsProcessor on one logit (transformers 4.31: torch.where(score < 0, score * penalty, score / penalty)), fp32 with
// the correctly rounded divide: torch's fp32 result bit for bit
__device__ __forceinline__ float penalise(float x, float penalty) { return x < 0.f ? x * penalty : __fdiv_rn(x, penalty); }
// One addition of the additive adjustment (kAdj), rounded on its own: hipcc contracts a * b + c into an fma by default
// (__fadd_rn is a plain + to it), which would fuse penalise()'s product with the post term.
__device__ __forceinline__ float add_rounded(float x, float y) {
#pragma clang fp contract(off)
  return x + y;
}

// kMiro (vt_sample_rows_miro): one step of the cutoff, mu - eta * (e - tau), every operation rounded on its own (hipcc
// would contract the product and the difference into an fma): the test recomputes it bit for bit from the cell's own e
__device__ __forceinline__ float miro_step(float mu, float eta, float e, float tau) {
#pragma clang fp contract(off)
  const float d = e - tau;
  const float g = eta * d;
  return mu - g;
}

// kTrunc (vt_sample_rows_trunc): MinP / Typical / Epsilon / Eta warpers on the survivors of top-k and top-p. Both bodies
// work on p = the token's probability over the top-k set; the softmax over the survivors A is q = p / S with S = sum_A p, so every rule
// is stated on p: q < t  <=>  p < t * S, and with T = sum_A p log p:  H = log S - T / S  and  -log q - H = T / S - log p.
__device__ __forceinline__ bool trunc_on(float x) { return x > 0.f && x < 1.f; }      // (NaN: off)
// the bit pattern of d = |T / S - log p|: d >= 0 (or NaN), so the unsigned pattern orders it and is < 2^31
__device__ __forceinline__ uint32_t trunc_d_key(float p, float c) { return __float_as_uint(fabsf(c - __logf(p))); }
__device__ __forceinline__ float trunc_plogp(float p) { return p > 0.f ? p * __logf(p) : 0.f; }
// EtaLogitsWarper's threshold on p
__device__ __forceinline__ float trunc_eta(float e, float S, float T) {
  const float H = __logf(S) - T / S;
  return fminf(e, sqrtf(e) * __expf(-H)) * S;
}

// V-bit "seen" mask of the row's history in LDS: bit id is set for every history id in [0, V). Ids outside that range (the negative
// image / region sentinels of a multimodal prompt, anything >= V) are skipped and index nothing. Returns whether a penalty applies.
__device__ __forceinline__ bool fill_seen_mask(uint32_t* seen, int V, const SampleArgs& a) {
  if (!(a.history && a.history_len > 0) || a.penalty == 1.0f) return false;     // (block-uniform: the barriers below are safe)
  const int words = (V + 31) >> 5;
  for (int w = threadIdx.x; w < words; w += 1024) seen[w] = 0u;
  __syncthreads();
  for (int h = threadIdx.x; h < a.history_len; h += 1024) {
    const int id = a.history[h];
    if (id >= 0 && id < V) atomicOr(&seen[id >> 5], 1u << (id & 31));
  }
  __syncthreads();
  return true;
}

// TopKLogitsWarper (transformers 4.31: scores < topk(scores, k)[..., -1] are removed, ties with the k-th value stay): the
// k-th largest scaled logit is found exactly by bisection on the ordered bit pattern (32 counting passes), no sort.
//
// Streaming form of the sampler, any V: the row is re-read from memory (L2) in every pass. kRows adds what vt_sample_rows needs on
// top of vt_sample_top_p's arithmetic -- the repetition penalty (through `seen`, ceil(V/32) words of LDS), greedy rows and the
// log-probability of the chosen token -- and compiles to nothing in the launch-uniform kernel.
// kAllow (vt_sample_rows_allow): `allow` is the row's V-bit allow mask in GLOBAL memory (ceil(V/32) words, NULL = all
// allowed). val(i) reads word i >> 5 for i < V only -- always inside the mask -- and a token whose bit is clear is -inf BEFORE the penalty,
// i.e. exactly a row with -inf written there. The raw log-sum-exp does not go through val(): logprob stays over the RAW row.
// kAdj (vt_sample_rows_adj): `adj` is the row's additive adjustment in GLOBAL memory, fp32 [V][2] = (pre, post) per token,
// 8-byte aligned, NULL = none. val(i) reads pair i for i < V only; pre is added after the mask and before the penalty, post after it.
// kTrunc (vt_sample_rows_trunc): no V-bit survivor mask is kept (the seen mask has half of the static LDS already). The
// stages reduce to two block-uniform facts about a token's p -- a lower threshold `plo` (min_p, epsilon and eta only ever raise it) and
// the typical stage's (c, key) pair -- and VT_ALIVE(p) re-evaluates them wherever the keep test of the top-p step stands. With every stage
// off plo = 0 and the pair is unused: the sets, sums and the walk are those of the kAdj body.
template <bool kRows, bool kAllow = false, bool kAdj = false, bool kTrunc = false>
__device__ __forceinline__ void sample_stream_body(const float* __restrict__ row, int V, const SampleArgs& a, uint32_t* seen,
                                                   int* __restrict__ out_id, int* __restrict__ kept_out, float* __restrict__ logprob,
                                                   const uint32_t* __restrict__ allow = nullptr, const float* __restrict__ adj = nullptr,
                                                   vt_trunc_row tr = vt_trunc_row{}) {
  __shared__ float sh[16];
  __shared__ float sh_scan[16];
  __shared__ int chosen;
  const int tid = threadIdx.x;
  const float inv_temp = a.inv_temp, top_p = a.top_p;
  const int top_k = a.top_k;
  float lse = 0.f;
  bool pen = false;
  if constexpr (kRows) {
    if (logprob) {       // log-sum-exp of the RAW row (before penalty and temperature): vt_rows.h's, as cross_entropy_rows_kernel
      float rmx;
      lse = row_lse_stream(row, V, tid, sh, rmx);
    }
    pen = fill_seen_mask(seen, V, a);
  }
  auto val = [&](int i) -> float {     // the (penalised) logit i
    float x = row[i];
    if constexpr (kAllow)
      if (allow && !((allow[i >> 5] >> (i & 31)) & 1u)) x = -INFINITY;
    float post = 0.f;
    if constexpr (kAdj) {
      if (adj) {         // block-uniform
        const float2 pq = *(const float2*)(adj + 2 * (size_t)i);
        x = add_rounded(x, pq.x);
        post = pq.y;
      }
    }
    if constexpr (kRows)
      if (pen && ((seen[i >> 5] >> (i & 31)) & 1u)) x = penalise(x, a.penalty);
    if constexpr (kAdj)
      if (adj) x = add_rounded(x, post);
    return x;
  };
  if constexpr (kRows) {
    if (a.greedy) {      // block-uniform
      __shared__ int si[16];
      float best = -INFINITY;
      int bi = kRowNone;
      for (int i = tid; i < V; i += 1024) take(best, bi, val(i), i);
      __syncthreads();
      row_block_argmax(best, bi, sh, si, take);
      if (tid == 0) {
        *out_id = bi;
        if (kept_out) *kept_out = 1;
        if (logprob) *logprob = (unsigned)bi < (unsigned)V ? row[bi] - lse : NAN;
      }
      return;
    }
  }
  float mx = -INFINITY;
  for (int i = tid; i < V; i += 1024) mx = fmaxf(mx, val(i) * inv_temp);
  mx = row_block_max(mx, sh);
  float floor_logit = -INFINITY;   // scaled logits below this are outside the top-k set
  if (top_k > 0 && top_k < V) {
    uint64_t lo = 0, hi = 0x100000000ull;   // invariant: count(key >= lo) >= k, count(key >= hi) < k
    for (int it = 0; it < 32; ++it) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      float c = 0.f;
      for (int i = tid; i < V; i += 1024) c += ((uint64_t)order_key(val(i) * inv_temp) >= mid) ? 1.f : 0.f;
      c = row_block_sum(c, sh);
      if (c >= (float)top_k) lo = mid; else hi = mid;
    }
    const uint32_t k32 = (uint32_t)lo;
    floor_logit = __uint_as_float((k32 & 0x80000000u) ? (k32 & 0x7fffffffu) : ~k32);
  }
#define VT_P_OF(i) ((val(i) * inv_temp >= floor_logit) ? __expf(val(i) * inv_temp - mx) : 0.f)
  float z = 0.f;
  for (int i = tid; i < V; i += 1024) z += VT_P_OF(i);
  z = row_block_sum(z, sh);
  const float inv_z = 1.f / z;
  // bisection on the threshold t in (0, 1]: mass(t) = sum of p_i with p_i >= t is non-increasing in t.
  // keep-set of the warper = {i : mass of tokens strictly above p_i < top_p}  <=>  largest t with mass(t) >= top_p.
  float lo = 0.f, hi = 1.f;   // invariant: mass(lo) >= top_p, mass(hi) < top_p (or hi == 1 when a single token has p >= top_p)
  for (int it = 0; it < 30; ++it) {
    const float mid = 0.5f * (lo + hi);
    float m = 0.f;
    for (int i = tid; i < V; i += 1024) {
      const float p = VT_P_OF(i) * inv_z;
      if (p >= mid) m += p;
    }
    m = row_block_sum(m, sh);
    if (m >= top_p) lo = mid; else hi = mid;
  }
  const float thr = (top_p >= 1.f) ? 0.f : fminf(lo, inv_z);   // inv_z = probability of the arg-max token: always kept
  float kept = 0.f, cnt = 0.f;
  for (int i = tid; i < V; i += 1024) {
    const float p = VT_P_OF(i) * inv_z;
    if (p >= thr && val(i) * inv_temp >= floor_logit) {      // (thr == 0 at top_p >= 1: the top-k filter still applies)
      kept += p;
      cnt += 1.f;
    }
  }
  kept = row_block_sum(kept, sh);
  cnt = row_block_sum(cnt, sh);
  float plo = 0.f, typ_c = 0.f;      // (kTrunc) what the stages leave: p >= plo, and with `typ` the key of |typ_c - log p| <= typ_key
  uint32_t typ_key = 0x7fffffffu;
  bool typ = false;
  // (a macro whose `!kTrunc ||` the front end folds away, not a lambda: the flavours without truncation compile to the code they had)
#define VT_ALIVE(p) (!kTrunc || ((p) >= plo && (!typ || trunc_d_key((p), typ_c) <= typ_key)))
  if constexpr (kTrunc) {
    const bool on_min = tr.min_p > 0.f, on_typ = trunc_on(tr.typical_p), on_eps = trunc_on(tr.epsilon_cutoff),
               on_eta = trunc_on(tr.eta_cutoff);
    if (on_min || on_typ || on_eps || on_eta) {       // block-uniform
      float S = 0.f, top = 0.f, T = 0.f;
      auto stats = [&](bool want_T) {      // mass, maximum and sum of p log p over the current survivors
        float s = 0.f, m = 0.f, t = 0.f;
        for (int i = tid; i < V; i += 1024) {
          const float p = VT_P_OF(i) * inv_z;
          if (p >= thr && val(i) * inv_temp >= floor_logit && VT_ALIVE(p)) {
            s += p;
            m = fmaxf(m, p);
            if (want_T) t += trunc_plogp(p);
          }
        }
        S = row_block_sum(s, sh);
        top = row_block_max(m, sh);
        if (want_T) T = row_block_sum(t, sh);
      };
      // "p < t leaves unless it ties with the maximum" is p >= min(t, top) for those who stay (a NaN t: only the maximum stays)
      if (on_min) {
        stats(false);
        plo = fmaxf(plo, fminf(tr.min_p * top, top));
      }
      if (on_typ) {
        stats(true);
        const float c = T / S, need = tr.typical_p * S;
        // the smallest key whose tokens reach the mass, exactly: 31 counting passes over [0, 2^31) (the sign bit of d is clear). The
        // whole of A has mass S >= need, so the largest key always qualifies: nothing reaches the mass <=> all stay.
        uint32_t lo = 0u, hi = 0x7fffffffu;
        for (int it = 0; it < 31; ++it) {
          const uint32_t mid = lo + ((hi - lo) >> 1);
          float m = 0.f;
          for (int i = tid; i < V; i += 1024) {
            const float p = VT_P_OF(i) * inv_z;
            if (p >= thr && val(i) * inv_temp >= floor_logit && VT_ALIVE(p) && trunc_d_key(p, c) <= mid) m += p;
          }
          m = row_block_sum(m, sh);
          if (m >= need) hi = mid; else lo = mid + 1u;
        }
        typ_c = c;
        typ_key = hi;
        typ = true;
      }
      if (on_eps) {
        stats(false);
        plo = fmaxf(plo, fminf(tr.epsilon_cutoff * S, top));
      }
      if (on_eta) {
        stats(true);
        plo = fmaxf(plo, fminf(trunc_eta(tr.eta_cutoff, S, T), top));
      }
      kept = 0.f;
      cnt = 0.f;
      for (int i = tid; i < V; i += 1024) {
        const float p = VT_P_OF(i) * inv_z;
        if (p >= thr && val(i) * inv_temp >= floor_logit && VT_ALIVE(p)) {
          kept += p;
          cnt += 1.f;
        }
      }
      kept = row_block_sum(kept, sh);
      cnt = row_block_sum(cnt, sh);
    }
  }
  if (tid == 0 && kept_out) *kept_out = (int)cnt;
  // inverse CDF over the kept tokens in index order: thread t owns the contiguous index range [t*chunk, (t+1)*chunk)
  const float u = sample_uniform24(a) * kept;
  const int chunk = (V + 1023) / 1024;
  const int i0 = tid * chunk, i1 = min(V, i0 + chunk);
  float mine = 0.f;
  for (int i = i0; i < i1; ++i) {
    const float p = VT_P_OF(i) * inv_z;
    if (p >= thr && val(i) * inv_temp >= floor_logit && VT_ALIVE(p)) mine += p;
  }
  // exclusive prefix over threads: wave scan + scan of the 16 wave totals
  float incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float v = __shfl_up(incl, o, 64);
    if ((tid & 63) >= o) incl += v;
  }
  __syncthreads();
  if ((tid & 63) == 63) sh_scan[tid >> 6] = incl;
  __syncthreads();
  float base = 0.f;
  for (int w = 0; w < (tid >> 6); ++w) base += sh_scan[w];
  const float excl = base + incl - mine;
  // the owner of u is the thread with excl <= u < excl + mine; fall back to the last kept token against rounding
  if (tid == 0) chosen = -1;
  __syncthreads();
  if (mine > 0.f && u >= excl && u < excl + mine) {
    float c = excl;
    int pick = -1;
    for (int i = i0; i < i1; ++i) {
      const float p = VT_P_OF(i) * inv_z;
      if (p >= thr && val(i) * inv_temp >= floor_logit && VT_ALIVE(p)) {
        pick = i;
        c += p;
        if (u < c) break;
      }
    }
    atomicMax(&chosen, pick);
  }
  __syncthreads();
  if (chosen < 0 && mine > 0.f) {  // u landed on a rounding seam: take the last kept token of the highest owning range
    int last = -1;
    for (int i = i0; i < i1; ++i)
      if (VT_P_OF(i) * inv_z >= thr && val(i) * inv_temp >= floor_logit && VT_ALIVE(VT_P_OF(i) * inv_z)) last = i;
    atomicMax(&chosen, last);
  }
  __syncthreads();
  if (tid == 0) {
    const int id = chosen;
    *out_id = id;
    if constexpr (kRows)
      if (logprob) *logprob = (unsigned)id < (unsigned)V ? row[id] - lse : NAN;
  }
}
#undef VT_P_OF
#undef VT_ALIVE

// Same rule with the row held in registers (V <= 32 * 1024): every thread owns 32 consecutive logits, computes their
// exponentials ONCE, and the 30 bisection passes, the kept-mass pass and the inverse-CDF walk never touch memory again.
// 165 us -> ~20 us per call at V = 32000 (tools/sampler_bench.py).
// kRows: thread t's 32 logits are exactly word t of the seen mask, so the penalty is one LDS word per thread and a static unroll
// (no dynamic register index, no scratch).
// kAllow: word t of the row's allow mask is read straight from global memory (threads past ceil(V/32) read nothing: their slots are
// -inf already) and applied under the same static unroll, after the raw log-sum-exp and before the penalty. Bits >= V of the last
// word meet slots that are -inf whatever the bit says.
// kAdj: the thread's 32 (pre, post) pairs are 256 contiguous bytes of the row's adjustment in global memory, read once -- 16 bytes (two
// pairs) at a time where the adjustment is 16-byte aligned, else 8: pre is added after the mask, then the penalty, then post, slot by
// slot. Slots past V read nothing and stay -inf.
// kTrunc (vt_sample_rows_trunc): the stages run where p holds the kept probabilities and 0 elsewhere. The survivors are the
// slots with p > 0 and a stage zeroes what it removes, so no second array and no mask register lives across the body; the typical
// stage recomputes a slot's d from its p in each of its 31 counting passes instead of keeping 32 keys. With every stage off nothing
// between the top-p step and the prefix scan runs: p, mine and cnt are the kAdj body's.
// kWm (vt_sample_rows_wm): transformers' SynthIDTextWatermarkLogitsProcessor, which GenerationMixin runs behind every
// warper, so it stands behind kTrunc: where p holds the kept probabilities, q = p / kept goes through `depth` tournament rounds
// q *= 1 + g - sum(g q) in place, and the walk draws over sum(q) with the uniform it always had. g of token v at layer i is bit
// (A_v + layer_add[i]) & (table_size - 1) of the sampling table, A_v = ((H + v) * M + 1) * M for the context hash H: the table size is a
// power of two <= 2^16, so only the low 32 bits of that 64-bit sum are ever looked at -- one 64-bit multiply for the thread's first
// token, then 32-bit adds (M * M per slot, layer_add[i] per layer); no A_v is kept, and a slot whose q is 0 is not hashed. The table is
// staged into LDS (`wm_tab`, table_size / 32 words, with the low words of layer_add behind it). The sequence's state (struct vt_wm_row's cell) is read by every thread and written
// by thread 0 alone, behind the last barrier. cnt is not recounted: kept_count stays the truncation's survivors. wm == NULL
// (block-uniform: a row without a cell) runs nothing of this: p, mine and cnt are the kTrunc body's.
// kMiro (vt_sample_rows_miro): Mirostat v2 (Basu et al., ICLR 2021; llama.cpp's mirostat_v2), behind kTrunc and without
// kWm: where p holds the kept probabilities, q = p / kept replaces it, a slot whose surprise -log2f(q) exceeds the cell's mu is zeroed
// (when the maximum's own surprise exceeds mu, every slot but the first index of the maximum), cnt is recounted and the walk draws over
// sum(q) with the uniform it always had. One block sum (kept), one block maximum, one pass over the registers; the arg-max pass runs
// only where nothing survives. The cell {mu, last_surprise} is read by every thread in front of the stage's barriers and written behind the last
// barrier by the one thread that owns the drawn slot: it still holds q_x, so nothing is parked in LDS. mu is compared, never used as an
// index. miro == NULL (block-uniform: a row without a cell or with tau <= 0) runs nothing of this: p, mine and cnt are the kTrunc body's.
template <bool kRows, bool kAllow = false, bool kAdj = false, bool kTrunc = false, bool kWm = false, bool kMiro = false>
__device__ __forceinline__ void sample_reg_body(const float* __restrict__ row, int V, const SampleArgs& a, uint32_t* seen,
                                                int* __restrict__ out_id, int* __restrict__ kept_out, float* __restrict__ logprob,
                                                const uint32_t* __restrict__ allow = nullptr, const float* __restrict__ adj = nullptr,
                                                vt_trunc_row tr = vt_trunc_row{}, const vt_wm_row* __restrict__ wm = nullptr,
                                                uint32_t* wm_tab = nullptr, const vt_miro_row* miro = nullptr) {
  static_assert(!(kWm && kMiro), "sample_reg_body: Mirostat together with the watermark is not built");
  constexpr int NPT = 32;
  __shared__ float sh[2][16];
  __shared__ float sh_scan[16];
  __shared__ int chosen;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = tid * NPT;
  const float inv_temp = a.inv_temp, top_p = a.top_p;
  const int top_k = a.top_k;
  float p[NPT];
#pragma unroll
  for (int j = 0; j < NPT; j += 4) {
    f32x4 v = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (i0 + j + 3 < V) {
      v = *(const f32x4*)(row + i0 + j);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (i0 + j + k < V) v[k] = row[i0 + j + k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) p[j + k] = v[k];
  }
  int buf = 0;
  auto block_sum = [&](float v) -> float {   // one barrier per call: two alternating LDS rows
    v = wave_sum(v);
    if (lane == 0) sh[buf][wave] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += sh[buf][i];
    buf ^= 1;
    return t;
  };
  auto block_max = [&](float v) -> float {
    v = wave_max(v);
    if (lane == 0) sh[buf][wave] = v;
    __syncthreads();
    float t = sh[buf][0];
#pragma unroll
    for (int i = 1; i < 16; ++i) t = fmaxf(t, sh[buf][i]);
    buf ^= 1;
    return t;
  };
  __shared__ float lse;    // (kRows; in LDS, not in a register that would live across the whole body: only thread 0 reads it back)
  if constexpr (kRows) {
    if (logprob) {       // log-sum-exp of the RAW row (before penalty and temperature), expf / logf as cross_entropy_rows_kernel
      float rmx = -INFINITY;
#pragma unroll
      for (int j = 0; j < NPT; ++j) rmx = fmaxf(rmx, p[j]);
      rmx = block_max(rmx);
      float rz = 0.f;
#pragma unroll
      for (int j = 0; j < NPT; ++j) rz += expf(p[j] - rmx);     // exp(-inf) = 0 for the slots past V
      rz = block_sum(rz);
      if (tid == 0) lse = rmx + logf(rz);
    }
    if constexpr (kAllow) {
      if (allow) {       // block-uniform
        const uint32_t ok = tid < ((V + 31) >> 5) ? allow[tid] : 0u;
#pragma unroll
        for (int j = 0; j < NPT; ++j)
          if (!((ok >> j) & 1u)) p[j] = -INFINITY;
      }
    }
    const bool pen = fill_seen_mask(seen, V, a);
    bool adjusted = false;
    if constexpr (kAdj) {
      if (adj) {         // block-uniform: pre, the penalty and post in one pass over the thread's 32 pairs
        adjusted = true;
        const uint32_t word = pen ? seen[tid] : 0u;
        auto apply = [&](float x, float pre, float post, int j) -> float {
          x = add_rounded(x, pre);
          if ((word >> j) & 1u) x = penalise(x, a.penalty);
          return add_rounded(x, post);
        };
        const float* __restrict__ mine = adj + 2 * i0;
        if (((uintptr_t)adj % 16) == 0) {      // block-uniform: two pairs per 16-byte load, half the (lane-strided) load instructions
#pragma unroll
          for (int j = 0; j < NPT; j += 2) {
            if (i0 + j + 1 < V) {
              const f32x4 q = *(const f32x4*)(mine + 2 * j);
              p[j] = apply(p[j], q[0], q[1], j);
              p[j + 1] = apply(p[j + 1], q[2], q[3], j + 1);
            } else if (i0 + j < V) {
              const float2 q = *(const float2*)(mine + 2 * j);
              p[j] = apply(p[j], q.x, q.y, j);
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < NPT; ++j) {
            if (i0 + j < V) {
              const float2 q = *(const float2*)(mine + 2 * j);
              p[j] = apply(p[j], q.x, q.y, j);
            }
          }
        }
      }
    }
    if (pen && !adjusted) {
      const uint32_t word = seen[tid];
#pragma unroll
      for (int j = 0; j < NPT; ++j)
        if ((word >> j) & 1u) p[j] = penalise(p[j], a.penalty);
    }
    if (a.greedy) {      // block-uniform
      __shared__ int si[16];
      float best = -INFINITY;
      int bi = kRowNone;
#pragma unroll
      for (int j = 0; j < NPT; ++j)
        if (i0 + j < V) take(best, bi, p[j], i0 + j);
      __syncthreads();
      row_block_argmax(best, bi, sh[0], si, take);
      if (tid == 0) {
        *out_id = bi;
        if (kept_out) *kept_out = 1;
        if (logprob) *logprob = (unsigned)bi < (unsigned)V ? row[bi] - lse : NAN;
      }
      return;
    }
  }
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < NPT; ++j) {
    p[j] = p[j] * inv_temp;
    mx = fmaxf(mx, p[j]);
  }
  mx = block_max(mx);
  uint32_t valid = 0xffffffffu;   // bit j: slot j is inside the top-k set (all slots when the filter is off)
  if (top_k > 0 && top_k < V) {   // TopKLogitsWarper: everything below the k-th largest scaled logit leaves the distribution
    // the slots hold their ordered keys (as bits) for the 32 passes and get their values back after: a second set of 32 registers for
    // the keys is what used to push this kernel into scratch
#pragma unroll
    for (int j = 0; j < NPT; ++j) p[j] = __uint_as_float(order_key(p[j]));
    uint64_t lo = 0, hi = 0x100000000ull;
    for (int it = 0; it < 32; ++it) {
      const uint64_t mid = lo + ((hi - lo) >> 1);     // < 2^32: mid < hi
      const uint32_t mid32 = (uint32_t)mid;
      float c = 0.f;
#pragma unroll
      for (int j = 0; j < NPT; ++j) c += (__float_as_uint(p[j]) >= mid32) ? 1.f : 0.f;
      c = block_sum(c);
      if (c >= (float)top_k) lo = mid; else hi = mid;
    }
    valid = 0u;
    const uint32_t lo32 = (uint32_t)lo;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
      const uint32_t key = __float_as_uint(p[j]);
      const bool in = key >= lo32;
      valid |= in ? (1u << j) : 0u;
      p[j] = in ? __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key) : -INFINITY;
    }
  }
  float zl = 0.f;
#pragma unroll
  for (int j = 0; j < NPT; ++j) {
    p[j] = __expf(p[j] - mx);     // exp(-inf) = 0 for the slots past V and outside the top-k set
    zl += p[j];
  }
  const float z = block_sum(zl);
  const float inv_z = 1.f / z;
#pragma unroll
  for (int j = 0; j < NPT; ++j) p[j] *= inv_z;
  float lo = 0.f, hi = 1.f;   // invariant: mass(lo) >= top_p, mass(hi) < top_p (or hi == 1 when one token has p >= top_p)
  for (int it = 0; it < 30; ++it) {
    const float mid = 0.5f * (lo + hi);
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < NPT; ++j) m += (p[j] >= mid) ? p[j] : 0.f;
    m = block_sum(m);
    if (m >= top_p) lo = mid; else hi = mid;
  }
  const float thr = (top_p >= 1.f) ? 0.f : fminf(lo, inv_z);   // inv_z = probability of the arg-max token: always kept
  float mine = 0.f, cnt = 0.f;
#pragma unroll
  for (int j = 0; j < NPT; ++j) {
    const bool keep = p[j] >= thr && i0 + j < V && ((valid >> j) & 1u);
    p[j] = keep ? p[j] : 0.f;       // from here on p holds kept probabilities only
    mine += p[j];
    cnt += keep ? 1.f : 0.f;
  }
  if constexpr (kTrunc) {
    const bool on_min = tr.min_p > 0.f, on_typ = trunc_on(tr.typical_p), on_eps = trunc_on(tr.epsilon_cutoff),
               on_eta = trunc_on(tr.eta_cutoff);
    if (on_min || on_typ || on_eps || on_eta) {       // block-uniform
      float S = 0.f, top = 0.f, T = 0.f;
      auto stats = [&](bool want_T) {      // mass, maximum and sum of p log p over the current survivors
        float s = 0.f, m = 0.f, t = 0.f;
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
          s += p[j];
          m = fmaxf(m, p[j]);
          if (want_T) t += trunc_plogp(p[j]);
        }
        S = block_sum(s);
        top = block_max(m);
        if (want_T) T = block_sum(t);
      };
      // "p < t leaves unless it ties with the maximum": those below min(t, top) are zeroed (a NaN t: only the maximum stays)
      auto cut = [&](float t) {
#pragma unroll
        for (int j = 0; j < NPT; ++j) p[j] = p[j] >= t ? p[j] : 0.f;
      };
      if (on_min) {
        stats(false);
        cut(fminf(tr.min_p * top, top));
      }
      if (on_typ) {
        stats(true);
        const float c = T / S, need = tr.typical_p * S;
        // the smallest key whose tokens reach the mass, exactly: 31 counting passes over [0, 2^31) (the sign bit of d is clear). The
        // whole of A has mass S >= need, so the largest key always qualifies: nothing reaches the mass <=> all stay.
        uint32_t lo = 0u, hi = 0x7fffffffu;
        for (int it = 0; it < 31; ++it) {
          const uint32_t mid = lo + ((hi - lo) >> 1);
          float m = 0.f;
#pragma unroll
          for (int j = 0; j < NPT; ++j) m += (trunc_d_key(p[j], c) <= mid) ? p[j] : 0.f;     // (a removed slot adds its 0)
          m = block_sum(m);
          if (m >= need) hi = mid; else lo = mid + 1u;
        }
#pragma unroll
        for (int j = 0; j < NPT; ++j) p[j] = (trunc_d_key(p[j], c) <= hi) ? p[j] : 0.f;
      }
      if (on_eps) {
        stats(false);
        cut(fminf(tr.epsilon_cutoff * S, top));
      }
      if (on_eta) {
        stats(true);
        cut(fminf(trunc_eta(tr.eta_cutoff, S, T), top));
      }
      mine = 0.f;
      cnt = 0.f;
#pragma unroll
      for (int j = 0; j < NPT; ++j) {
        mine += p[j];
        cnt += p[j] > 0.f ? 1.f : 0.f;
      }
    }
  }
  if constexpr (kWm) {
    if (wm) {            // block-uniform. The row's fields are re-read where they are used (scalar loads), not carried through the body
      constexpr uint64_t M = kWmMul;
      const uint64_t* cell = wm->cell;
      const int hs = wm->history_size, ngram = wm->ngram_len;
      const uint64_t calls = cell[0] + 1;
      uint64_t H = 1;
      for (int i = 0; i < ngram - 1; ++i) H = (H + cell[4 + i]) * M + 1;       // (the context ids are data only)
      const bool skipped = wm->skip_first != 0 && calls < (uint64_t)ngram;
      bool repeated = false;
      if (!skipped) {
        const uint32_t* __restrict__ table = wm->table;
        for (int w = tid; w < (wm->table_size >> 5); w += 1024) wm_tab[w] = table[w];
        if (tid < wm->depth) wm_tab[kWmLayerWord + tid] = (uint32_t)wm->layer_add[tid];     // (the low words: no global load per round)
        float hit = 0.f;
        for (int e = tid; e < hs; e += 1024) hit += cell[12 + e] == H ? 1.f : 0.f;     // ALL entries, the zero ones included
        repeated = block_sum(hit) > 0.f;          // (its barrier also publishes wm_tab and ends the reads of the ring)
      }
      if (tid == 0) {    // what the write-back behind the draw needs, parked in LDS: nothing of it lives in a register across the walk
        uint64_t* st = (uint64_t*)(wm_tab + kWmStateWord);
        st[0] = calls;
        st[1] = H;
        st[2] = skipped ? 4u : (repeated ? 2u : 1u);
      }
      const float kept_p = (skipped || repeated) ? 0.f : block_sum(mine);
      if (kept_p > 0.f) {
        const float inv = 1.f / kept_p;
        const uint32_t tmask = (uint32_t)wm->table_size - 1u, slot_add = (uint32_t)(M * M);
        const uint32_t a0 = (uint32_t)(((H + (uint64_t)i0) * M + 1) * M);
        const int depth = wm->depth;
        uint32_t live = 0u;       // bit j: slot j had q > 0 when the rounds began (one a round zeroes stays set: its g meets a 0)
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
          p[j] *= inv;
          live |= p[j] > 0.f ? (1u << j) : 0u;
        }
        for (int i = 0; i < depth; ++i) {
          const uint32_t b = a0 + wm_tab[kWmLayerWord + i];
          uint32_t g = 0u;
          // the table lookups eight slots at a time, skipping an eighth with nothing alive: a rolled loop over the live mask, so that
          // the 32 gathers and their addresses are never in registers together beside p[]
#pragma unroll 1
          for (int j0 = 0; j0 < NPT; j0 += 8) {
            if ((live >> j0) & 0xffu) {
#pragma unroll
              for (int k = 0; k < 8; ++k) {
                const uint32_t t = (b + (uint32_t)(j0 + k) * slot_add) & tmask;
                g |= ((wm_tab[t >> 5] >> (t & 31u)) & 1u) << (j0 + k);
              }
            }
          }
          g &= live;
          float m = 0.f;
#pragma unroll
          for (int j = 0; j < NPT; ++j) m += ((g >> j) & 1u) ? p[j] : 0.f;
          m = block_sum(m);
          const float up = 2.f - m, down = 1.f - m;        // 1 + g - m
#pragma unroll
          for (int j = 0; j < NPT; ++j) p[j] *= ((g >> j) & 1u) ? up : down;
        }
        mine = 0.f;
#pragma unroll
        for (int j = 0; j < NPT; ++j) mine += p[j];
      }
    }
  }
  bool miro_on = false;    // (kMiro; block-uniform) the stage ran: the cell is written behind the draw
  if constexpr (kMiro) {
    if (miro) {          // block-uniform
      const float kept_p = block_sum(mine);
      if (kept_p > 0.f) {
        miro_on = true;
        const float mu = miro->cell[0];           // (every thread's read lies in front of the barriers below; the write is behind the last)
        const float inv = 1.f / kept_p;
        float top = 0.f;
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
          p[j] *= inv;
          top = fmaxf(top, p[j]);
        }
        top = block_max(top);
        if (-log2f(top) <= mu) {                  // block-uniform. The maximum survives, and with it every slot that equals it
#pragma unroll
          for (int j = 0; j < NPT; ++j) p[j] = (p[j] > 0.f && -log2f(p[j]) <= mu) ? p[j] : 0.f;
        } else {         // (a NaN mu too) nothing survives on its own: the first index of the maximum alone. Indices < 2^15 are exact in fp32
          float first = -INFINITY;
#pragma unroll
          for (int j = NPT - 1; j >= 0; --j) first = p[j] == top ? -(float)(i0 + j) : first;
          first = block_max(first);
#pragma unroll
          for (int j = 0; j < NPT; ++j) p[j] = -(float)(i0 + j) == first ? p[j] : 0.f;
        }
        mine = 0.f;
        cnt = 0.f;
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
          mine += p[j];
          cnt += p[j] > 0.f ? 1.f : 0.f;
        }
      }
    }
  }
  const float kept = block_sum(mine);
  cnt = block_sum(cnt);
  if (tid == 0) {
    if (kept_out) *kept_out = (int)cnt;
    chosen = -1;
  }
  const float u = sample_uniform24(a) * kept;
  // exclusive prefix over threads: wave scan + scan of the 16 wave totals
  float incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) sh_scan[wave] = incl;
  __syncthreads();
  float base = 0.f;
  for (int w = 0; w < wave; ++w) base += sh_scan[w];
  const float excl = base + incl - mine;
  if (mine > 0.f && u >= excl && u < excl + mine) {
    float c = excl;
    int pick = -1;
    bool done = false;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
      if (!done && p[j] > 0.f) {
        pick = i0 + j;
        c += p[j];
        done = u < c;
      }
    }
    atomicMax(&chosen, pick);
  }
  __syncthreads();
  if (chosen < 0 && mine > 0.f) {  // u landed on a rounding seam: take the last kept token of the highest owning range
    int last = -1;
    if constexpr (kWm || kMiro) {   // the slot, not the id: the 32 ids i0 + j of the loads are not kept across the body for this rare path
#pragma unroll
      for (int j = 0; j < NPT; ++j)
        if (p[j] > 0.f) last = j;
      last += tid * NPT;   // (mine > 0: a slot was found)
    } else {
#pragma unroll
      for (int j = 0; j < NPT; ++j)
        if (p[j] > 0.f) last = i0 + j;
    }
    atomicMax(&chosen, last);
  }
  __syncthreads();
  if constexpr (kMiro) {
    if (miro_on) {       // block-uniform. The owner of the drawn slot holds q_x; the cell has this one writer
      const int id = chosen;
      if (id >= 0 && id / NPT == tid) {
        float qx = 0.f;
#pragma unroll
        for (int j = 0; j < NPT; ++j) qx = (id % NPT) == j ? p[j] : qx;
        float* cell = miro->cell;
        const float e = -log2f(__fdiv_rn(qx, kept));
        float2 next;
        next.x = miro_step(cell[0], miro->eta, e, miro->tau);
        next.y = e;
        *(float2*)cell = next;
      }
    }
  }
  if (tid == 0) {
    const int id = chosen;
    *out_id = id;
    if constexpr (kRows)
      if (logprob) *logprob = (unsigned)id < (unsigned)V ? row[id] - lse : NAN;
    if constexpr (kWm) {
      if (wm) {          // every thread's reads of the cell lie in front of the barriers above
        const uint64_t* st = (const uint64_t*)(wm_tab + kWmStateWord);
        uint64_t* cell = wm->cell;
        const int hs = wm->history_size, n1 = wm->ngram_len - 1;
        const uint64_t H = st[1], flags = st[2];
        uint64_t head = cell[1] % (uint64_t)hs;       // (whatever the cell holds: inside the ring)
        if (!(flags & 4u)) {                          // (a skipped call returns in front of transformers' history update)
          cell[12 + head] = H;
          head = head + 1 == (uint64_t)hs ? 0 : head + 1;
        }
        cell[0] = st[0];
        cell[1] = head;
        cell[2] = H;
        cell[3] = flags;
        if (id >= 0) {                                // the context: generated ids only, on skipped and repeated calls too
          for (int i = 0; i + 1 < n1; ++i) cell[4 + i] = cell[5 + i];
          cell[4 + n1 - 1] = (uint64_t)id;
        }
      }
    }
  }
}

// vt_sample_top_p: launch-uniform parameters, the row index as the stream of the uniform
__device__ __forceinline__ SampleArgs uniform_args(float inv_temp, int top_k, float top_p, uint64_t seed, uint64_t step) {
  return SampleArgs{inv_temp, top_k, top_p, seed, step, blockIdx.x, false, 1.0f, nullptr, 0};
}
__global__ __launch_bounds__(1024) void sample_top_p_kernel(const float* __restrict__ logits, int V, int ldl,
                                                            float inv_temp, int top_k, float top_p, uint64_t seed, uint64_t step,
                                                            int* __restrict__ out_ids, int* __restrict__ kept_count) {
  sample_stream_body<false>(logits + (size_t)blockIdx.x * ldl, V, uniform_args(inv_temp, top_k, top_p, seed, step), nullptr,
                            out_ids + blockIdx.x, kept_count ? kept_count + blockIdx.x : nullptr, nullptr);
}
__global__ __launch_bounds__(1024) void sample_top_p_reg_kernel(const float* __restrict__ logits, int V, int ldl,
                                                                float inv_temp, int top_k, float top_p, uint64_t seed, uint64_t step,
                                                                int* __restrict__ out_ids, int* __restrict__ kept_count) {
  sample_reg_body<false>(logits + (size_t)blockIdx.x * ldl, V, uniform_args(inv_temp, top_k, top_p, seed, step), nullptr,
                         out_ids + blockIdx.x, kept_count ? kept_count + blockIdx.x : nullptr, nullptr);
}

// vt_sample_rows: the same two bodies, every row with its own vt_sample_row. Nothing a field can hold indexes out of bounds: a
// temperature that is not > 0 (0, negative, NaN) is a greedy row, top_k <= 0 is off, a top_p the bisection cannot reach keeps the whole
// row, history ids are range-checked, a NULL history or a length <= 0 is an empty one.
constexpr int kSampleRowsMaxV = VT_SAMPLE_ROWS_MAX_V;
__device__ __forceinline__ SampleArgs row_args(const vt_sample_row& r) {
  const bool greedy = !(r.temperature > 0.f);
  return SampleArgs{greedy ? 1.0f : __fdiv_rn(1.0f, r.temperature), r.top_k, r.top_p, r.seed, r.counter, r.stream, greedy,
                    r.repetition_penalty, r.history, r.history_len};
}
// A watermark entry the launcher would have refused (it reads the array in front of the launch; the array may have changed since) is a
// row without a watermark in the kernel, so that no field value indexes outside the table, the ring or the context.
__device__ __forceinline__ bool wm_row_ok(const vt_wm_row& w) {
  return w.layer_add && w.table && w.depth >= 1 && w.depth <= VT_WM_MAX_DEPTH && w.table_size >= 32 && w.table_size <= VT_WM_MAX_TABLE
         && (w.table_size & (w.table_size - 1)) == 0 && w.ngram_len >= 2 && w.ngram_len <= VT_WM_MAX_NGRAM && w.history_size >= 1
         && w.history_size <= VT_WM_MAX_HISTORY;
}

// A Mirostat entry the launcher would have refused (see wm_row_ok), or one that is off (tau <= 0, a NULL cell), is a row without Mirostat.
__device__ __forceinline__ bool miro_row_ok(const vt_miro_row& m) {
  return m.cell && ((uintptr_t)m.cell % 8) == 0 && m.tau > 0.f && m.tau < INFINITY && m.eta >= 0.f && m.eta < INFINITY;
}

// The vt_sample_rows family is ONE kernel in two forms (kReg: the register body, else the streaming one) and six flavours. A flavour is
// the highest per-row array the launch carries, and holds every flavour below it (kMiro holds kTrunc and below: not kWm):
//   kPlain  vt_sample_rows        params[r] alone
//   kAllow  vt_sample_rows_allow  + allow[r]: the row's allow mask, ceil(V/32) words in global memory in both forms (the LDS is kPlain's)
//   kAdj    vt_sample_rows_adj    + adjust[r]: the row's additive adjustment, fp32 [V][2]
//   kTrunc  vt_sample_rows_trunc  + trunc[r]: min_p, typical_p, epsilon_cutoff, eta_cutoff
//   kWm     vt_sample_rows_wm     + wm[r]: the SynthID watermark, with wm_tab as its LDS. The register form only: the
//                                 streaming body keeps no per-token state across the rounds.
//   kMiro   vt_sample_rows_miro   kTrunc + miro[r]: Mirostat v2. The register form only: the stage works on the row's
//                                 q in registers. Without kWm: the two together are not built.
// The array that selects the flavour is not NULL (the launcher chose the flavour by it) and is read as it is; every array BELOW it may be
// NULL and is tested -- adjustments without masks, a watermark without truncation. An ENTRY allow[r] / adjust[r] may be NULL in every
// flavour (everything allowed / no adjustment); a wm[r] whose cell is NULL is a row without a watermark. An instantiation reads only the
// kernel arguments that its flavour names, so the lower flavours stay the code they were before the higher ones existed.
// The arguments are separate __restrict__ pointers, not one struct by value: a struct's members cannot be __restrict__, and without it
// the register form of kTrunc grew by 4 % in instructions. `allow` stands beside `params`, the other arrays LAST in the
// flavours' order: what kPlain, kAllow and kAdj read lies within one 64-byte line of the kernel-argument segment, and kAllow's
// arguments lie where a kernel with allow alone would have them (its register form compiles to that kernel's code).
enum : int { kPlain, kAllow, kAdj, kTrunc, kWm, kMiro, kFlavours };
template <bool kReg, bool... kFlags, class... Extra>
__device__ __forceinline__ void sample_rows_body(const float* __restrict__ row, int V, const SampleArgs& a, uint32_t* seen,
                                                 int* __restrict__ out_id, int* __restrict__ kept, float* __restrict__ lp, Extra... extra) {
  if constexpr (kReg)
    sample_reg_body<true, kFlags...>(row, V, a, seen, out_id, kept, lp, extra...);
  else
    sample_stream_body<true, kFlags...>(row, V, a, seen, out_id, kept, lp, extra...);
}
template <bool kReg, int kFlavour>
__global__ __launch_bounds__(1024) void sample_rows_kernel(const float* __restrict__ logits, int V, int ldl,
                                                           const vt_sample_row* __restrict__ params,
                                                           const uint32_t* const* __restrict__ allow, int* __restrict__ out_ids,
                                                           int* __restrict__ kept_count, float* __restrict__ logprob,
                                                           const float* const* __restrict__ adjust,
                                                           const vt_trunc_row* __restrict__ trunc, const vt_wm_row* __restrict__ wm,
                                                           const vt_miro_row* __restrict__ miro) {
  static_assert(kFlavour >= kPlain && kFlavour < kFlavours, "sample_rows_kernel: unknown flavour");
  static_assert(kReg || kFlavour != kWm, "sample_rows_kernel: the watermark runs in the register form only");
  static_assert(kReg || kFlavour != kMiro, "sample_rows_kernel: Mirostat runs in the register form only");
  __shared__ uint32_t seen[(kReg ? 32 * 1024 : kSampleRowsMaxV) / 32];
  const int r = blockIdx.x;
  SampleArgs a = row_args(params[r]);
  const float* row = logits + (size_t)r * ldl;
  int* const out_id = out_ids + r;
  int* const kept = kept_count ? kept_count + r : nullptr;
  float* const lp = logprob ? logprob + r : nullptr;
  const uint32_t* mask = nullptr;
  if constexpr (kFlavour == kAllow) mask = allow[r];
  if constexpr (kFlavour > kAllow) mask = allow ? allow[r] : nullptr;
  const float* adj = nullptr;
  if constexpr (kFlavour == kAdj) adj = adjust[r];
  if constexpr (kFlavour > kAdj) adj = adjust ? adjust[r] : nullptr;
  if constexpr (kFlavour <= kAdj) {
    sample_rows_body<kReg, (kFlavour >= kAllow), (kFlavour >= kAdj)>(row, V, a, seen, out_id, kept, lp, mask, adj);
  } else {
    // A greedy row ignores its stages and never touches its watermark cell: it takes the kAdj body, a sampled row the kTrunc / kWm one --
    // each inlined with `greedy` known, so neither copy carries the other's path (the register form kept the unscaled logits alive for
    // the greedy branch across the stages otherwise).
    if (a.greedy) {        // block-uniform
      a.greedy = true;
      sample_rows_body<kReg, true, true>(row, V, a, seen, out_id, kept, lp, mask, adj);
      return;
    }
    a.greedy = false;
    if constexpr (kFlavour == kTrunc) {
      sample_rows_body<kReg, true, true, true>(row, V, a, seen, out_id, kept, lp, mask, adj, trunc[r]);
    } else if constexpr (kFlavour == kMiro) {
      const vt_miro_row* m = miro + r;
      if (!miro_row_ok(*m)) m = nullptr;
      sample_reg_body<true, true, true, true, false, true>(row, V, a, seen, out_id, kept, lp, mask, adj, trunc ? trunc[r] : vt_trunc_row{},
                                                           nullptr, nullptr, m);
    } else {
      __shared__ __attribute__((aligned(8))) uint32_t wm_tab[kWmLdsWords];
      const vt_wm_row* w = wm + r;
      if (!w->cell || !wm_row_ok(*w)) w = nullptr;
      sample_reg_body<true, true, true, true, true>(row, V, a, seen, out_id, kept, lp, mask, adj, trunc ? trunc[r] : vt_trunc_row{},
                                                    w, wm_tab);
    }
  }
}

}  // namespace

int vt_sample_top_p_launch(const float* logits, int rows, int V, int ldl, float temperature, int top_k, float top_p, uint64_t seed,
                           uint64_t step, int* out_ids, int* kept_count, hipStream_t s) {
  VT_REQUIRE(logits && out_ids && rows > 0 && V > 0, "vt_sample_top_p: bad arguments");
  VT_REQUIRE(temperature > 0.f && top_p > 0.f && top_k >= 0, "vt_sample_top_p: temperature and top_p must be > 0, top_k >= 0");
  if (V <= 32 * 1024 && (ldl % 4) == 0 && ((uintptr_t)logits % 16) == 0)
    hipLaunchKernelGGL(sample_top_p_reg_kernel, dim3(rows), dim3(1024), 0, s, logits, V, ldl, 1.0f / temperature, top_k, top_p, seed,
                       step, out_ids, kept_count);
  else
    hipLaunchKernelGGL(sample_top_p_kernel, dim3(rows), dim3(1024), 0, s, logits, V, ldl, 1.0f / temperature, top_k, top_p, seed,
                       step, out_ids, kept_count);
  VT_LAUNCH_CHECK();
  return VT_OK;
}

// vt_sample_rows_wm refuses a field outside its range by name, and the array is on the device: it is read back in front of the launch,
// rows * 48 bytes on the launch's own stream (so behind whatever uploads it) and a wait for that copy. A stream that is being captured
// cannot wait; there the kernel's own wm_row_ok stands alone (such an entry is a row without a watermark). A row whose cell
// is NULL is not watermarked and its other fields are not looked at.
static int wm_rows_check(const vt_wm_row* wm, int rows, hipStream_t s) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess) (void)hipGetLastError();
  if (cap != hipStreamCaptureStatusNone) return VT_OK;
  std::vector<vt_wm_row> h((size_t)rows);
  VT_HIP(hipMemcpyAsync(h.data(), wm, (size_t)rows * sizeof(vt_wm_row), hipMemcpyDeviceToHost, s));
  VT_HIP(hipStreamSynchronize(s));
  for (int r = 0; r < rows; ++r) {
    const vt_wm_row& w = h[(size_t)r];
    if (!w.cell) continue;
    VT_REQUIRE(((uintptr_t)w.cell % 8) == 0 && w.layer_add && ((uintptr_t)w.layer_add % 8) == 0 && w.table && ((uintptr_t)w.table % 4) == 0,
               "vt_sample_rows_wm: wm[%d]: cell and layer_add must be 8-byte aligned, table 4-byte aligned, layer_add and table not NULL", r);
    VT_REQUIRE(w.depth >= 1 && w.depth <= VT_WM_MAX_DEPTH, "vt_sample_rows_wm: wm[%d].depth=%d (1 <= depth <= %d)", r, w.depth,
               VT_WM_MAX_DEPTH);
    VT_REQUIRE(w.table_size >= 32 && w.table_size <= VT_WM_MAX_TABLE && (w.table_size & (w.table_size - 1)) == 0,
               "vt_sample_rows_wm: wm[%d].table_size=%d (a power of two, 32 <= table_size <= %d)", r, w.table_size, VT_WM_MAX_TABLE);
    VT_REQUIRE(w.ngram_len >= 2 && w.ngram_len <= VT_WM_MAX_NGRAM, "vt_sample_rows_wm: wm[%d].ngram_len=%d (2 <= ngram_len <= %d)", r,
               w.ngram_len, VT_WM_MAX_NGRAM);
    VT_REQUIRE(w.history_size >= 1 && w.history_size <= VT_WM_MAX_HISTORY,
               "vt_sample_rows_wm: wm[%d].history_size=%d (1 <= history_size <= %d)", r, w.history_size, VT_WM_MAX_HISTORY);
    VT_REQUIRE(w.reserved == 0, "vt_sample_rows_wm: wm[%d].reserved=%d (must be 0)", r, w.reserved);
  }
  return VT_OK;
}

// vt_sample_rows_miro's check of its device array: wm_rows_check's pattern (one read-back of rows * 16 bytes on the launch's own stream
// and a wait; not on a stream that is being captured, where the kernel's own miro_row_ok stands alone). A row whose cell is NULL runs no
// Mirostat and its other fields are not looked at.
static int miro_rows_check(const vt_miro_row* miro, int rows, hipStream_t s) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess) (void)hipGetLastError();
  if (cap != hipStreamCaptureStatusNone) return VT_OK;
  std::vector<vt_miro_row> h((size_t)rows);
  VT_HIP(hipMemcpyAsync(h.data(), miro, (size_t)rows * sizeof(vt_miro_row), hipMemcpyDeviceToHost, s));
  VT_HIP(hipStreamSynchronize(s));
  for (int r = 0; r < rows; ++r) {
    const vt_miro_row& m = h[(size_t)r];
    if (!m.cell) continue;
    VT_REQUIRE(((uintptr_t)m.cell % 8) == 0, "vt_sample_rows_miro: miro[%d]: cell must be 8-byte aligned", r);
    VT_REQUIRE(std::isfinite(m.tau), "vt_sample_rows_miro: miro[%d].tau=%g (must be finite; <= 0 is off)", r, (double)m.tau);
    VT_REQUIRE(std::isfinite(m.eta) && m.eta >= 0.f, "vt_sample_rows_miro: miro[%d].eta=%g (must be finite and >= 0)", r, (double)m.eta);
  }
  return VT_OK;
}

int vt_sample_rows_launch(const float* logits, int rows, int V, int ldl, const vt_sample_row* params, const uint32_t* const* allow,
                          int* out_ids, int* kept_count, float* logprob, hipStream_t s, const float* const* adjust,
                          const vt_trunc_row* trunc, const vt_wm_row* wm, const vt_miro_row* miro) {
  VT_REQUIRE(logits && params && out_ids, "vt_sample_rows: null pointer (logits, params and out_ids are required)");
  VT_REQUIRE(rows > 0 && V > 0 && ldl >= V, "vt_sample_rows: rows=%d V=%d ldl=%d (rows, V > 0 and ldl >= V)", rows, V, ldl);
  VT_REQUIRE(((uintptr_t)params % 8) == 0, "vt_sample_rows: params must be 8-byte aligned");
  VT_REQUIRE(((uintptr_t)allow % 8) == 0, "vt_sample_rows_allow: the allow pointer array must be 8-byte aligned");
  VT_REQUIRE(((uintptr_t)adjust % 8) == 0, "vt_sample_rows_adj: the adjust pointer array must be 8-byte aligned");
  VT_REQUIRE(((uintptr_t)trunc % 4) == 0, "vt_sample_rows_trunc: trunc must be 4-byte aligned");
  const bool reg = V <= 32 * 1024 && (ldl % 4) == 0 && ((uintptr_t)logits % 16) == 0;
  if (wm) {
    VT_REQUIRE(((uintptr_t)wm % 8) == 0, "vt_sample_rows_wm: wm must be 8-byte aligned");
    VT_REQUIRE(reg,
               "vt_sample_rows_wm: V=%d ldl=%d: the watermark runs in the register form only (V <= 32768, ldl %% 4 == 0, logits 16-byte "
               "aligned)", V, ldl);
    const int st = wm_rows_check(wm, rows, s);
    if (st != VT_OK) return st;
  }
  if (miro) {
    VT_REQUIRE(!wm, "vt_sample_rows_miro: Mirostat together with the watermark is not built");
    VT_REQUIRE(((uintptr_t)miro % 8) == 0, "vt_sample_rows_miro: miro must be 8-byte aligned");
    VT_REQUIRE(reg,
               "vt_sample_rows_miro: V=%d ldl=%d: Mirostat runs in the register form only (V <= 32768, ldl %% 4 == 0, logits 16-byte "
               "aligned)", V, ldl);
    const int st = miro_rows_check(miro, rows, s);
    if (st != VT_OK) return st;
  }
  VT_REQUIRE(reg || V <= VT_SAMPLE_ROWS_MAX_V, "vt_sample_rows: V=%d is beyond the history mask of the streaming form (V <= %d)", V,
             VT_SAMPLE_ROWS_MAX_V);
  // [form][flavour]; the flavour is the highest array given (sample_rows_kernel); a watermark or Mirostat has been refused above without `reg`
  static const decltype(&sample_rows_kernel<true, kPlain>) kKernels[2][kFlavours] = {
      {sample_rows_kernel<false, kPlain>, sample_rows_kernel<false, kAllow>, sample_rows_kernel<false, kAdj>,
       sample_rows_kernel<false, kTrunc>, nullptr, nullptr},
      {sample_rows_kernel<true, kPlain>, sample_rows_kernel<true, kAllow>, sample_rows_kernel<true, kAdj>,
       sample_rows_kernel<true, kTrunc>, sample_rows_kernel<true, kWm>, sample_rows_kernel<true, kMiro>}};
  const int flavour = miro ? kMiro : wm ? kWm : trunc ? kTrunc : adjust ? kAdj : allow ? kAllow : kPlain;
  hipLaunchKernelGGL(kKernels[reg][flavour], dim3(rows), dim3(1024), 0, s, logits, V, ldl, params, allow, out_ids, kept_count, logprob,
                     adjust, trunc, wm, miro);
  VT_LAUNCH_CHECK();
  return VT_OK;
}
