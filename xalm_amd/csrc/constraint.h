// constraint.h — what the byte-DFA constraint's host side shares between constraint.cpp (plain
// C++, no HIP: the regex compiler, xh_constraint_mask, the argument checks) and decode.hip.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/xalm_hip.h"

namespace xalm {

constexpr size_t DFA_MAX_PIECE_BYTES = (size_t)16 << 20;  // the blob's cap
constexpr int DFA_MAX_VOCAB = 1 << 17;                     // the sampler's (SMP_MAX_VOCAB)

// The checks of the definition's invalid-argument list that need no device; nullptr = valid.
const char* dfa_error(const xh_byte_dfa* dfa);
const char* dfa_state_error(const xh_byte_dfa* dfa, uint32_t state);  // state_in: a state or XH_DFA_DEAD
const char* pieces_error(const uint8_t* bytes, const uint32_t* offsets, int vocab);

// The walk of one piece from `state`: where it ends, or XH_DFA_DEAD (also for an empty piece).
inline uint32_t dfa_walk(const uint16_t* next, uint32_t state, const uint8_t* piece, uint32_t len) {
    if (len == 0) return XH_DFA_DEAD;
    for (uint32_t i = 0; i < len && state != XH_DFA_DEAD; i++) state = next[(size_t)state * 256 + piece[i]];
    return state;
}

}  // namespace xalm
