// Epoch totals of a validation pass, accumulated on the device (include/bist_hip.h: bist_eval_accumulate).
//
// The reference's validation loop (train.py:32-37 with eval=True) multiplies every per-token loss term by its token count again
// (optimize.py:92-94) and adds the products and the counts to running totals -- a handful of elementwise launches per batch, issued
// from Python.  bist_amd/train.py replays one captured forward pass per length class; this launch is the tail of that graph: thread k
// adds term_k * count_k to total_k and count_k to its running integer total, and one more counter counts the batches.  The host
// reads the totals once, at the end of the pass.
//
// The running sums are doubles: a term times its count is exact in double (24-bit significand times a count below 2^29), and a few
// thousand batches of such products keep every digit an fp32 epoch average can show.  Integer totals are int64.
#include "common.hpp"

namespace {

struct EvalAccK {
  const float* term[BIST_EVAL_MAX_TERMS];
  const long long* term_count[BIST_EVAL_MAX_TERMS];
  const long long* count[BIST_EVAL_MAX_COUNTS];
  int n_terms, n_counts;
};

__global__ void eval_accumulate_kernel(EvalAccK k, double* __restrict__ totals, long long* __restrict__ count_totals) {
  const int t = (int)threadIdx.x;
  if (t < k.n_terms) totals[t] += (double)k.term[t][0] * (double)k.term_count[t][0];
  if (t < k.n_counts) count_totals[t] += k.count[t][0];
  if (t == k.n_counts) count_totals[t] += 1;       // batches
}

}  // namespace

extern "C" int bist_eval_accumulate(const void* const* terms, const void* const* term_counts, int32_t n_terms, const void* const* counts,
                                    int32_t n_counts, double* totals, int64_t* count_totals, void* stream) {
  BIST_REQUIRE(terms && term_counts && counts && totals && count_totals, "bist_eval_accumulate: null argument");
  BIST_REQUIRE(n_terms >= 1 && n_terms <= BIST_EVAL_MAX_TERMS && n_counts >= 0 && n_counts <= BIST_EVAL_MAX_COUNTS,
               "bist_eval_accumulate: 1 <= n_terms <= %d, 0 <= n_counts <= %d", BIST_EVAL_MAX_TERMS, BIST_EVAL_MAX_COUNTS);
  EvalAccK k{};
  for (int i = 0; i < n_terms; ++i) {
    BIST_REQUIRE(terms[i] && term_counts[i], "bist_eval_accumulate: term %d: null pointer", i);
    k.term[i] = (const float*)terms[i];
    k.term_count[i] = (const long long*)term_counts[i];
  }
  for (int i = 0; i < n_counts; ++i) {
    BIST_REQUIRE(counts[i], "bist_eval_accumulate: count %d: null pointer", i);
    k.count[i] = (const long long*)counts[i];
  }
  k.n_terms = n_terms;
  k.n_counts = n_counts;
  hipLaunchKernelGGL(eval_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, k, totals, (long long*)count_totals);
  BIST_LAUNCH_CHECK("bist_eval_accumulate");
  return BIST_OK;
}
