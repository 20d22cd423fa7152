// xalm.h — C++ host mirror of the reference API this path plugs into (jubruckne/Xalm):
//
//   Xalm::load / file_info / tensor_info      src/xalm.h:11-192
//   Config::from_xalm                         src/model.h:25-91
//   InferenceState                            src/model.h:96-156   (host logits only)
//   InferenceMode                             src/model.h:249-252
//   Device + Model::from_xalm / forward       src/model.h:21-23, 254-284; src/model.cpp:48-122
//   Model::active_bytes                       src/model.cpp:12-35
//   Tokenizer                                 src/tokenizer.h/.cpp
//   Sampler                                   src/sampler.h/.cpp
//
// Model::forward goes through the C ABI of libxalm_hip.so (include/xalm_hip.h); Device::HIP
// is the MI355X path.  Device::CPU is the reference's own CPU forward, which this product does
// not ship (its restatement lives in oracle/ as the test checker), so selecting it throws.
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/xalm_hip.h"

namespace xalm {

// ---- .xalm container ------------------------------------------------------------------
struct TensorInfo {
    std::string name;
    int type = 0;              // enum xh_dtype
    std::vector<int> shape;
    size_t offset = 0;         // absolute file offset
    size_t size = 0;           // bytes
};

struct XalmFile {
    std::string file_name;
    std::string arch;
    std::map<std::string, std::string> metadata;  // config values (strings, convert.py:223-245)
    std::map<std::string, TensorInfo> tensors;

    static XalmFile load(const std::string& path);  // Xalm::load, src/xalm.h:90-192
    void read(const TensorInfo& ti, void* dst) const;
    std::vector<uint8_t> read(const std::string& name) const;
    const std::string& meta(const std::string& key) const;
    std::string meta_or(const std::string& key, const std::string& dflt) const;
};

int parse_type(const std::string& s);  // Type::parse, src/types.h:468-499
size_t type_size(int type);
// bytes of one 32-element block of the converter's gguf block types (convert.py:176-187,
// quants.py), 0 for any other type: the one table of their names and sizes (xalm_file.cpp)
size_t block_bytes(int type);
size_t block_elems(int type);  // elements per block of a block type (32; the K-quants 256), else 0

// ---- model ------------------------------------------------------------------------------
enum class Device { CPU, HIP };
enum class InferenceMode { HYDRATE_KV_CACHE = XH_HYDRATE_KV_CACHE, OUTPUT_LOGITS = XH_OUTPUT_LOGITS };
enum class ActivationType { GELU = XH_ACT_GELU, SILU = XH_ACT_SILU };

struct Config {
    int dim = 0, hidden_dim = 0, head_dim = 0, n_layers = 0, n_heads = 0, n_kv_heads = 0, vocab_size = 0;
    int max_seq_len = 0;
    float rope_theta = 0;
    int rotary_dim = 0;
    float norm_eps = 1e-5f;
    ActivationType act = ActivationType::GELU;
    float qkv_clip = 0;
    bool tie_word_embeddings = false;

    static Config from_xalm(const XalmFile& xalm, int context = 0);
    xh_config to_abi() const;
};

struct InferenceState {
    explicit InferenceState(const Config& config) : _logits(config.vocab_size, 0.f) {}
    float* logits() { return _logits.data(); }
    const float* logits() const { return _logits.data(); }

private:
    std::vector<float> _logits;
};

struct Tokenizer;

// A regex constraint for decoding (xh_byte_dfa, include/xalm_hip.h): the trimmed byte DFA of
// xh_regex_compile and the tokenizer's piece table, on the host
struct Constraint {
    std::vector<uint16_t> next;     // [n_states][256]
    std::vector<uint8_t> accept;    // [n_states]
    int n_states = 0, start = 0;
    std::vector<uint8_t> bytes;     // the pieces, back to back
    std::vector<uint32_t> offsets;  // [vocab + 1]
    // throws std::invalid_argument for a pattern xh_regex_compile refuses
    static Constraint compile(const std::string& regex, const Tokenizer& tokenizer);
    xh_byte_dfa dfa() const { return {n_states, start, next.data(), accept.data()}; }
};

class Model {
public:
    // kv_dtype: the KV rings' element type, XH_F16 or XH_F8_E4M3 (xh_create_kv)
    static Model from_xalm(const XalmFile& xalm, int context = 0, Device device = Device::HIP, int ordinal = 0,
                           int kv_dtype = XH_F16);
    Model(Model&& o) noexcept;
    Model& operator=(Model&&) = delete;
    Model(const Model&) = delete;
    Model& operator=(const Model&) = delete;
    ~Model();

    Config config;

    void forward(InferenceState& s, int token, int pos, InferenceMode mode = InferenceMode::OUTPUT_LOGITS) const;
    // the prompt loop (src/main.cpp:94-100) in one call: HYDRATE tokens[0..n-1), the last with
    // logits into s (xh_prefill: batched passes of up to 64 tokens)
    void prefill(InferenceState& s, const std::vector<int>& tokens, int pos0) const;
    // greedy decode on the device (no host round trip per token); returns the tokens
    std::vector<int> decode_greedy(int pos, int n_steps, int stop_a = -1, int stop_b = -1) const;
    // sampled decode on the device (xh_decode_sample): step i drawn at counter pos + i
    std::vector<int> decode_sample(int pos, int n_steps, const xh_sampling& sampling, int stop_a = -1,
                                   int stop_b = -1) const;
    // the same loop with repetition penalties, logit bias and min-p (xh_decode_sample_ext, xh_logit_ctl):
    // `history` = the tokens before pos (prompt and earlier output); logprobs (may be null) receives
    // one log-probability per token
    std::vector<int> decode_sample_ext(int pos, int n_steps, const xh_sampling& sampling, const xh_logit_ctl& ctl,
                                       const std::vector<int>& history, int stop_a = -1, int stop_b = -1,
                                       std::vector<float>* logprobs = nullptr) const;
    // upload a constraint's pieces and DFA (xh_constraint_set_vocab, xh_constraint_set)
    void set_constraint(const Constraint& c) const;
    // decode_sample_ext under the uploaded constraint (xh_decode_sample_dfa): state_in = the DFA's
    // start or an earlier call's *state_out
    std::vector<int> decode_sample_dfa(int pos, int n_steps, const xh_sampling& sampling, const xh_logit_ctl& ctl,
                                       const std::vector<int>& history, uint32_t state_in, int stop_a = -1,
                                       int stop_b = -1, uint32_t* state_out = nullptr,
                                       std::vector<float>* logprobs = nullptr) const;
    // decode_sample_dfa with the adaptive truncation of xh_trunc_ctl (xh_decode_sample_adapt):
    // constrain = mask with the uploaded constraint; mu_in = Mirostat's mu (2 * tau at the start) or
    // an earlier call's *mu_out
    std::vector<int> decode_sample_adapt(int pos, int n_steps, const xh_sampling& sampling, const xh_logit_ctl& ctl,
                                         const xh_trunc_ctl& trunc, const std::vector<int>& history, bool constrain,
                                         uint32_t state_in, float mu_in, int stop_a = -1, int stop_b = -1,
                                         uint32_t* state_out = nullptr, float* mu_out = nullptr,
                                         std::vector<float>* logprobs = nullptr) const;
    // decode_sample_adapt with DRY, the n-gram ban and XTC of xh_seq_ctl (xh_decode_sample_seq)
    std::vector<int> decode_sample_seq(int pos, int n_steps, const xh_sampling& sampling, const xh_logit_ctl& ctl,
                                       const xh_trunc_ctl& trunc, const xh_seq_ctl& seq, const std::vector<int>& history,
                                       bool constrain, uint32_t state_in, float mu_in, int stop_a = -1, int stop_b = -1,
                                       uint32_t* state_out = nullptr, float* mu_out = nullptr,
                                       std::vector<float>* logprobs = nullptr) const;
    // n_top > 0: the device decode loops also record each step's top list and the emitted token's
    // rank (xh_set_top_logprobs); 0 = off
    void set_top_logprobs(int n_top) const;
    // the first n_steps steps of the last decode call (xh_get_top_logprobs): ids and lps
    // [n_steps][n_top], ranks [n_steps]
    struct TopLogprobs {
        int n_top = 0;
        std::vector<int> ids;
        std::vector<float> lps;
        std::vector<int> ranks;
    };
    TopLogprobs top_logprobs(int n_steps) const;
    // prompt scoring (xh_score): for i < tokens.size() - 1 the log-probability and rank of
    // tokens[i + 1] after tokens[i] at pos0 + i, and the top lists [n - 1][n_top]
    struct Score {
        int n_top = 0;
        std::vector<float> logprobs;
        std::vector<int> ranks, top_ids;
        std::vector<float> top_lps;
    };
    Score score(const std::vector<int>& tokens, int pos0, int n_top = 0) const;
    void fetch_logits(InferenceState& s) const;
    // run_perplexity's loop on the device (xh_perplexity): element i = Sampler::sample_prob of
    // tokens[i + 1] after forwarding tokens[i] at pos0 + i
    std::vector<float> token_probs(const std::vector<int>& tokens, int pos0) const;
    [[nodiscard]] size_t active_bytes(size_t pos) const;
    xh_ctx* ctx() const { return _ctx; }

private:
    Model(const Config& c, xh_ctx* ctx) : config(c), _ctx(ctx) {}
    xh_ctx* _ctx = nullptr;
    mutable int _n_top = 0;  // the width set last: the row length of top_logprobs
};

// ---- tokenizer / sampler ------------------------------------------------------------------
struct TokenTrie {
    std::unordered_map<char, std::unique_ptr<TokenTrie>> children;
    int token_id = -1;
};

struct Tokenizer {
    std::vector<std::string> vocab;
    TokenTrie vocab_trie;
    int bos_id = -1, eos_id = -1, eot_id = -1, byte_fallback_start = -1;
    std::string byte_pieces[256];

    explicit Tokenizer(const XalmFile& data);
    std::vector<int> encode(const std::string& text, bool encode_bos) const;
    std::string decode_one(int prev_token, int token) const;
    // the piece table of xh_constraint_set_vocab: the vocab string of every token, the single byte
    // for a byte-fallback token; decode_one's strip of the space after BOS is not applied
    void pieces(std::vector<uint8_t>& bytes, std::vector<uint32_t>& offsets) const;
    // DRY's default sequence breakers: every token whose piece contains a newline, ':', '"' or '*', in
    // ascending id order; only the first XH_SEQ_MAX_BREAKERS (1024) of them are taken
    std::vector<int> default_breakers() const;
};

struct Sampler {
    explicit Sampler(const Config& c) : vocab_size(c.vocab_size) {}
    int vocab_size;
    int sample_argmax(const InferenceState& s) const;
    float sample_prob(int index, const InferenceState& s) const;
    // the n_top most likely tokens of the state's logits with their log-probabilities, and the
    // log-probability and 0-based rank of `token` (xh_top_logprobs_host, the definition of
    // XH_TOP_MAX in include/xalm_hip.h).  Throws std::invalid_argument outside its range.
    void top_logprobs(const InferenceState& s, int n_top, int token, std::vector<int>& ids, std::vector<float>& lps,
                      float& token_lp, int& token_rank) const;
    // temperature / top-k / top-p under the definition of xh_sampling (include/xalm_hip.h) at
    // counter `pos`, the position the token will occupy: the host restatement of the device
    // sampler, sums in double.  Throws std::invalid_argument for parameters outside it.
    int sample(const InferenceState& s, const xh_sampling& sampling, int pos) const;
    // the same on the logits adjusted under `ctl` (xh_logit_ctl, through xh_adjust_logits) over the
    // window `history` gives, with min-p; temperature 0 = sample_argmax of the adjusted logits
    int sample(const InferenceState& s, const xh_sampling& sampling, const xh_logit_ctl& ctl,
               const std::vector<int>& history, int pos) const;
    // the same under a constraint (the definition of xh_byte_dfa, through xh_constraint_mask): the
    // draw from the masked logits, temperature 0 = the first allowed token of the sampler's order;
    // `state` is the DFA state before the token and is advanced by it (XH_DFA_DEAD once stuck)
    int sample(const InferenceState& s, const xh_sampling& sampling, const xh_logit_ctl& ctl,
               const std::vector<int>& history, int pos, const Constraint& constraint, uint32_t& state, int stop_a,
               int stop_b) const;
    // the adaptive draw (the definition of xh_trunc_ctl, through xh_truncate_host): n-sigma, typical
    // and Mirostat cuts over the adjusted and, with a constraint (may be null), masked logits, then
    // top-p and the draw over the survivors; `mu` is Mirostat's state before the token and is
    // updated by it (negative = none yet: 2 * tau)
    int sample(const InferenceState& s, const xh_sampling& sampling, const xh_logit_ctl& ctl, const xh_trunc_ctl& trunc,
               const std::vector<int>& history, int pos, const Constraint* constraint, uint32_t& state, float& mu,
               int stop_a, int stop_b) const;
    // the sequence-aware draw (the definition of xh_seq_ctl, through xh_seq_adjust_host and
    // xh_xtc_host): DRY and the n-gram ban over `history` behind the adjustment and in front of the
    // mask, XTC behind the typical stage at this draw's counter
    int sample(const InferenceState& s, const xh_sampling& sampling, const xh_logit_ctl& ctl, const xh_trunc_ctl& trunc,
               const xh_seq_ctl& seq, const std::vector<int>& history, int pos, const Constraint* constraint,
               uint32_t& state, float& mu, int stop_a, int stop_b) const;
};
// the same on a bare logits vector; *n_kept (may be null) = size of the kept set
// min_p > 0 (xh_logit_ctl): the top-k stage keeps at most the tokens of weight >= min_p
int sample_logits(const float* logits, int vocab, const xh_sampling& sampling, uint64_t pos, int* n_kept,
                  float min_p = 0.f);
// the adaptive draw of Sampler::sample on a bare logits vector (raw: the adjustment is applied here)
int sample_adapt_logits(const float* logits, int vocab, const xh_sampling& sampling, const xh_logit_ctl& ctl,
                        const xh_trunc_ctl& trunc, const std::vector<int>& history, int pos, const Constraint* constraint,
                        uint32_t& state, float& mu, int stop_a, int stop_b);
// the sequence-aware draw of Sampler::sample on a bare logits vector (seq null: sample_adapt_logits)
int sample_seq_logits(const float* logits, int vocab, const xh_sampling& sampling, const xh_logit_ctl& ctl,
                      const xh_trunc_ctl& trunc, const xh_seq_ctl* seq, const std::vector<int>& history, int pos,
                      const Constraint* constraint, uint32_t& state, float& mu, int stop_a, int stop_b);

}  // namespace xalm
