// top_logprobs_host.h — what the top-N log-probabilities' host side shares between
// top_logprobs.cpp (plain C++, no HIP: xh_top_logprobs_host, the argument checks) and the units
// that launch the row kernel (decode.hip, prefill.hip).
#pragma once

#include "../../include/xalm_hip.h"

namespace xalm {

constexpr int TOP_MAX_VOCAB = 1 << 17;  // the sampler's (SMP_MAX_VOCAB)

// The checks of the definition's invalid-argument list for a [n_rows][vocab] block; nullptr =
// valid.  min_top: the least n_top allowed (1, or 0 where the top list may be left out);
// targets, target_lp_out and target_rank_out are given together or not at all.
const char* top_args_error(const float* logits, int vocab, int n_rows, int n_top, int min_top, const int* targets,
                           const int* ids_out, const float* lps_out, const float* target_lp_out,
                           const int* target_rank_out);

}  // namespace xalm
