// vt_llama.hip -- small kernels around the decoder: embedding gather + multimodal splice, the decode-loop feedback, greedy argmax,
// cross entropy. (The samplers, vt_sample_top_p and vt_sample_rows*, are vt_sample.hip.)
//
// embed_splice replaces the tensor surgery of prepare_inputs_labels_for_multimodal in the reference
// (vitron/model/llava_arch.py:306-398 region branch, :479-558 plain branch): embed_tokens gather for text
// ids, visual feature blocks at every -200 sentinel, one region feature row at every -300 sentinel,
// truncation and zero padding. The integer plan (which source row feeds which output row) is computed on
// the host by vitron_amd.model.llava_arch.build_splice_plan, bit-exactly following the reference's list
// logic; this kernel only moves rows.
#include "vt_common.h"
#include "vt_kernels.h"
#include "vt_rows.h"

namespace {

// plan[r] = {kind, index}: kind 0 = token id into tok_table, 1 = row of vis, 2 = row of reg, 3 = zeros
__global__ __launch_bounds__(256) void embed_splice_kernel(const bf16_t* __restrict__ tok_table,
                                                           const bf16_t* __restrict__ vis,
                                                           const bf16_t* __restrict__ reg,
                                                           const int* __restrict__ plan, int rows, int H,
                                                           bf16_t* __restrict__ out, int vocab, int vis_rows, int reg_rows) {
  const int chunks = H >> 3;  // 16-B chunks per row
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)rows * chunks;
       i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / chunks), c = (int)(i % chunks);
    const int kind = plan[2 * r], idx = plan[2 * r + 1];
    u32x4 v = {0u, 0u, 0u, 0u};
    // an index outside its table (a stray sentinel, an id >= the embedding rows) yields a zero row, never an out-of-bounds read;
    // the host mirror range-checks ids and raises like the reference's nn.Embedding would (vitron_amd/model/llava_arch.py)
    if (kind == 0 && (unsigned)idx < (unsigned)vocab) v = *(const u32x4*)(tok_table + (size_t)idx * H + c * 8);
    else if (kind == 1 && (unsigned)idx < (unsigned)vis_rows) v = *(const u32x4*)(vis + (size_t)idx * H + c * 8);
    else if (kind == 2 && (unsigned)idx < (unsigned)reg_rows) v = *(const u32x4*)(reg + (size_t)idx * H + c * 8);
    *(u32x4*)(out + (size_t)r * H + c * 8) = v;
  }
}

// decode-loop feedback, one block per sequence: thread 0 resolves the token this sequence emits (pad once finished), updates
// the finished flag against the EOS set and advances the sequence's device-side step metadata (kv_len, position); the block
// then copies the token's embedding row into the next step's input. Everything the next decoder pass needs is on the device
// after this launch, so the host can enqueue that pass before it has seen the token.
__global__ __launch_bounds__(256) void decode_feed_kernel(const bf16_t* __restrict__ tok_table, int H, int vocab,
                                                          const int* __restrict__ next_ids, int* __restrict__ finished,
                                                          const int* __restrict__ eos_ids, int n_eos, int pad_id,
                                                          int* __restrict__ tokens_out, bf16_t* __restrict__ x,
                                                          int* __restrict__ seq_desc, int* __restrict__ positions, int nseq) {
  __shared__ int tok_s;
  const int i = blockIdx.x;
  if (threadIdx.x == 0) {
    int fin = finished[i];
    const int t = fin ? pad_id : next_ids[i];
    for (int e = 0; e < n_eos; ++e) fin |= (t == eos_ids[e]);
    finished[i] = fin;
    tokens_out[i] = t;
    tokens_out[nseq + i] = fin;
    seq_desc[4 * i + 2] += 1;   // VtAttnSeq::kv_len
    positions[i] += 1;
    tok_s = min(max(t, 0), vocab - 1);
  }
  __syncthreads();
  const bf16_t* src = tok_table + (size_t)tok_s * H;
  bf16_t* dst = x + (size_t)i * H;
  for (int c = threadIdx.x; c < (H >> 3); c += 256) *(u32x4*)(dst + c * 8) = *(const u32x4*)(src + c * 8);
}

// vt_rows.h's (value, index) order in its branch form (see there why): argmax_kernel's rule (vt_sample.hip's greedy rows take the same)
constexpr RowTakeIf take{};       // (a NaN is never taken)

// first index of the maximum of each row (torch.argmax tie rule on CPU: lowest index). 1024 threads per row, 16-B loads,
// every request of the row in flight at once (a 32000-float row is 8 loads per thread).
__global__ __launch_bounds__(1024) void argmax_kernel(const float* __restrict__ logits, int V, int ldl,
                                                      int* __restrict__ out) {
  __shared__ float sv[16];
  __shared__ int si[16];
  const float* row = logits + (size_t)blockIdx.x * ldl;
  float best = -INFINITY;
  int bi = kRowNone;
  const bool vec = (ldl % 4) == 0 && ((uintptr_t)logits % 16) == 0;
  const int V4 = vec ? (V >> 2) : 0;
#pragma unroll 8
  for (int i = threadIdx.x; i < V4; i += 1024) {
    const f32x4 v = *(const f32x4*)(row + 4 * i);
#pragma unroll
    for (int k = 0; k < 4; ++k) take(best, bi, v[k], 4 * i + k);
  }
  for (int i = 4 * V4 + threadIdx.x; i < V; i += 1024) take(best, bi, row[i], i);
  row_block_argmax(best, bi, sv, si, take);
  if (threadIdx.x == 0) out[blockIdx.x] = bi;
}

// ---------------------------------------------------------------------------------------------------------------
// Shifted-token cross entropy of LlamaForCausalLM.forward(labels=...) (ignore_index rows skipped, mean over the rest):
//   nll[r] = logsumexp(logits[r]) - logits[r][label[r]]    one 1024-thread block per row, then one block averages.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void cross_entropy_rows_kernel(const float* __restrict__ logits, int V, int ldl,
                                                                  const int* __restrict__ labels, int ignore_index,
                                                                  float* __restrict__ nll) {
  __shared__ float sh[16];
  const int r = blockIdx.x;
  const int lab = labels[r];
  if (lab == ignore_index || lab < 0 || lab >= V) {     // (an out-of-range label cannot index the row: it is skipped like ignore_index)
    if (threadIdx.x == 0) nll[r] = -1.f;                // marker: not counted
    return;
  }
  const float* row = logits + (size_t)r * ldl;
  float mx;
  const float lse = row_lse_stream(row, V, threadIdx.x, sh, mx);
  if (threadIdx.x == 0) nll[r] = fmaxf(lse - row[lab], 0.f);
}
__global__ __launch_bounds__(1024) void cross_entropy_mean_kernel(const float* __restrict__ nll, int rows, float* __restrict__ loss) {
  __shared__ float sh[16];
  float s = 0.f, c = 0.f;
  for (int i = threadIdx.x; i < rows; i += 1024) {
    const float v = nll[i];
    if (v >= 0.f) {
      s += v;
      c += 1.f;
    }
  }
  s = row_block_sum(s, sh);
  c = row_block_sum(c, sh);
  if (threadIdx.x == 0) loss[0] = s / c;                // no valid row: 0/0 = NaN, as torch's mean over nothing
}

}  // namespace

int vt_cross_entropy_launch(const float* logits, int rows, int V, int ldl, const int* labels, int ignore_index, float* row_nll,
                            float* loss, hipStream_t s) {
  VT_REQUIRE(logits && labels && row_nll && loss && rows > 0 && V > 0, "vt_cross_entropy: bad arguments");
  hipLaunchKernelGGL(cross_entropy_rows_kernel, dim3(rows), dim3(1024), 0, s, logits, V, ldl, labels, ignore_index, row_nll);
  hipLaunchKernelGGL(cross_entropy_mean_kernel, dim3(1), dim3(1024), 0, s, row_nll, rows, loss);
  VT_LAUNCH_CHECK();
  return VT_OK;
}

int vt_embed_splice_launch(const bf16_t* tok_table, int vocab, const bf16_t* vis, int vis_rows, const bf16_t* reg, int reg_rows,
                           const int* plan, int rows, int H, bf16_t* out, hipStream_t s) {
  VT_REQUIRE(tok_table && plan && out, "vt_embed_splice: null pointer");
  VT_REQUIRE(vocab > 0 && vis_rows >= 0 && reg_rows >= 0 && (vis || vis_rows == 0) && (reg || reg_rows == 0),
             "vt_embed_splice: table sizes (vocab=%d vis_rows=%d reg_rows=%d)", vocab, vis_rows, reg_rows);
  VT_REQUIRE(rows > 0 && H % 8 == 0, "vt_embed_splice: rows=%d H=%d (H must be a multiple of 8)", rows, H);
  const long total = (long)rows * (H / 8);
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(embed_splice_kernel, dim3(blocks), dim3(256), 0, s, tok_table, vis, reg, plan, rows, H, out, vocab, vis_rows, reg_rows);
  VT_LAUNCH_CHECK();
  return VT_OK;
}

int vt_decode_feed_launch(const bf16_t* tok_table, int H, int vocab, const int* next_ids, int* finished, const int* eos_ids,
                          int n_eos, int pad_id, int* tokens_out, bf16_t* x, int* seq_desc, int* positions, int nseq,
                          hipStream_t s) {
  VT_REQUIRE(tok_table && next_ids && finished && tokens_out && x && seq_desc && positions, "vt_decode_feed: null pointer");
  VT_REQUIRE(nseq > 0 && vocab > 0 && H > 0 && H % 8 == 0, "vt_decode_feed: nseq=%d vocab=%d H=%d (H must be a multiple of 8)",
             nseq, vocab, H);
  VT_REQUIRE(n_eos == 0 || eos_ids, "vt_decode_feed: n_eos=%d without eos_ids", n_eos);
  hipLaunchKernelGGL(decode_feed_kernel, dim3(nseq), dim3(256), 0, s, tok_table, H, vocab, next_ids, finished, eos_ids,
                     n_eos < 0 ? 0 : n_eos, pad_id, tokens_out, x, seq_desc, positions, nseq);
  VT_LAUNCH_CHECK();
  return VT_OK;
}

int vt_argmax_launch(const float* logits, int rows, int V, int ldl, int* out_ids, hipStream_t s) {
  VT_REQUIRE(logits && out_ids && rows > 0 && V > 0, "vt_argmax: bad arguments");
  hipLaunchKernelGGL(argmax_kernel, dim3(rows), dim3(1024), 0, s, logits, V, ldl, out_ids);
  VT_LAUNCH_CHECK();
  return VT_OK;
}
