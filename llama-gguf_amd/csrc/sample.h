// sample.h — device sampling (sample.hip): the per-sequence sampler state the kernels read and the launcher.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace lgh {

// One sequence's sampler, device-resident so that a captured graph keeps working when the config changes.  The config half
// is Sampler::new's (sampling/mod.rs:37-62, 150-169); the call half describes the repetition window of the current decode
// call (the host writes it before the first step, the merge kernel advances it).  Under Mirostat the host stores temp 1,
// top_k 0, top_p 1 and min_p 0: sample_mirostat (mod.rs:210-213) returns before any of them is read.
struct SampSeq {
  float temp, inv_t, top_p, rp, fp, pp;   // inv_t = 1.0f / temp in f32, as the reference computes it
  uint32_t top_k, window;                 // window 0 = every token so far
  int32_t eos;                            // -1: none
  int32_t greedy;                         // temp == 0 || top_k == 1
  int32_t step;                           // steps done in this call
  int32_t eos_done;                       // eos sampled earlier in this call: counts are frozen
  // The window's token sequence is S = [last L0 history tokens] ++ [tokens fed in this call].  At step i the token leaving
  // the window is S[lv_a + i] (lv_a = L0 - window; none while negative).  tk[] holds S[0, lv_h) and then the fed tokens:
  // S[j] is tk[j] for j < lv_h and tk[j - lv_g] for j >= L0 (lv_g = L0 - lv_h; no leaving index falls in between).
  int32_t lv_a, lv_h, lv_g;
  int32_t track;                          // 1: append the token and update the counters (decode); 0: a one-off sample
  float min_p;                            // 0: off; ignored under a greedy config (mod.rs:248-258 come after the greedy return)
  int32_t miro;                           // 0: off, 1 / 2: MirostatConfig::version
  float tau, eta;
  // Sampler::mirostat_mu, the one field a decode call does not rewrite: set_sampler stores 2 * tau, the merge kernel updates
  // it after every Mirostat step, and the host's per-call upload ends before it.  Keep it last.
  float mu;
};
constexpr size_t kSampSeqCallBytes = offsetof(SampSeq, mu);   // what a decode call uploads

constexpr int kSampParts = 64;   // partial-pass workgroups per sequence
constexpr int kSampK = 64;       // candidates per workgroup and after the merge

// Device buffers of n_slots samplers and of up to n_rows sequences sampled in one launch.
struct SampBufs {
  uint32_t n_slots = 0, n_rows = 0, vocab = 0, tk_cap = 0, uni_cap = 0;
  SampSeq* ctl = nullptr;     // [slot]
  int* wcnt = nullptr;        // [slot][vocab] occurrences in the repetition window
  int* scnt = nullptr;        // [slot][vocab] times sampled (frequency / presence penalties)
  int* tk = nullptr;          // [slot][tk_cap] window tokens that leave during the call, then the fed tokens
  float* uni = nullptr;       // [slot][uni_cap] the call's uniform draws, one per step
  float* pb = nullptr;        // [row][vocab] probabilities (general path only)
  float* part_m = nullptr;    // [row][kSampParts] block max
  float* part_s = nullptr;    // [row][kSampParts] block exp-sum relative to the block max
  unsigned long long* part_k = nullptr;   // [row][kSampParts][kSampK] block candidates, sorted
  int* stage = nullptr;       // [2 * vocab + 32] (token, count) pairs of a window being loaded
};

// Sample one token per sequence s < n_seq from logits + s * vocab with the sampler of slot slots[s] (slots NULL: slot 0).
// The token goes to state[ST_TOKEN] and tok_log[state[ST_POS]] (when non-NULL) and to tokens_out[s] (when non-NULL).
hipError_t sample_launch(const SampBufs& B, const float* logits, uint32_t vocab, uint32_t n_seq, const int* slots, int* state,
                         int* tok_log, int* tokens_out, hipStream_t st);
// wcnt of `slot` = the n (token, count) pairs in B.stage (the rest zero); run before the call's first step
hipError_t sample_window_launch(const SampBufs& B, uint32_t slot, uint32_t n_pairs, hipStream_t st);

}  // namespace lgh
