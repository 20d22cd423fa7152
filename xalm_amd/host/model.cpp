// model.cpp — Model::from_xalm / forward over the C ABI (jubruckne/Xalm src/model.cpp:48-122),
// Tokenizer (src/tokenizer.cpp) and Sampler (src/sampler.cpp).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <numeric>
#include <cstdio>
#include <limits>
#include <stdexcept>

#include "xalm.h"

namespace xalm {

namespace {
void check(int rc, xh_ctx* ctx, const char* what) {
    if (rc != 0) throw std::runtime_error(std::string(what) + ": " + xh_last_error(ctx));
}
}  // namespace

// Model::from_xalm, src/model.cpp:48-118: the same tensor names and shape checks; the weights
// stream from the file into device memory through xh_upload_file (mapped, pinned and DMAd; no host
// Tensor buffers).
Model Model::from_xalm(const XalmFile& xalm, const int context, const Device device, const int ordinal,
                       const int kv_dtype) {
    if (device != Device::HIP)
        throw std::invalid_argument(
            "-d cpu: the reference CPU forward is not part of this build (its restatement is the test oracle, "
            "oracle/); use -d hip");
    const Config c = Config::from_xalm(xalm, context);
    xh_config abi = c.to_abi();
    xh_ctx* ctx = nullptr;
    check(xh_create_kv(&abi, ordinal, kv_dtype, &ctx), nullptr, "xh_create_kv");
    Model m(c, ctx);
    auto load = [&](const std::string& name, int kind, int layer, std::vector<int> shape) {
        const TensorInfo& ti = xalm.tensors.at(name);
        // gguf blocks (convert.py:176-187): the header holds the byte shape, 32 elements per block
        if (block_bytes(ti.type) && shape.size() == 2 && shape[1] % (int)block_elems(ti.type) == 0)
            shape[1] = shape[1] / (int)block_elems(ti.type) * (int)block_bytes(ti.type);
        if (ti.shape != shape) {
            std::string a, b;
            for (int v : ti.shape) a += std::to_string(v) + ",";
            for (int v : shape) b += std::to_string(v) + ",";
            throw std::invalid_argument("shape mismatch for " + name + ": [" + a + "] vs [" + b + "] expected!");
        }
        check(xh_upload_file(ctx, kind, layer, ti.type, xalm.file_name.c_str(), ti.offset, ti.size), ctx,
              name.c_str());
    };
    const int q_dim = c.n_heads * c.head_dim, kv_dim = c.n_kv_heads * c.head_dim;
    load("embed.weight", XH_EMBED, 0, {c.vocab_size, c.dim});
    for (int i = 0; i < c.n_layers; ++i) {
        const std::string p = "l." + std::to_string(i) + ".";
        load(p + "attn.norm.weight", XH_ATTN_NORM, i, {c.dim});
        load(p + "mlp.norm.weight", XH_FFN_NORM, i, {c.dim});
        load(p + "attn.q.weight", XH_WQ, i, {q_dim, c.dim});
        load(p + "attn.k.weight", XH_WK, i, {kv_dim, c.dim});
        load(p + "attn.v.weight", XH_WV, i, {kv_dim, c.dim});
        load(p + "attn.down.weight", XH_WO, i, {c.dim, q_dim});
        load(p + "mlp.gate.weight", XH_W1, i, {c.hidden_dim, c.dim});
        load(p + "mlp.down.weight", XH_W2, i, {c.dim, c.hidden_dim});
        load(p + "mlp.up.weight", XH_W3, i, {c.hidden_dim, c.dim});
    }
    load("output.norm.weight", XH_FINAL_NORM, 0, {c.dim});
    if (!c.tie_word_embeddings) load("output.weight", XH_WCLS, 0, {c.vocab_size, c.dim});
    return m;
}

Model::Model(Model&& o) noexcept : config(o.config), _ctx(o._ctx), _n_top(o._n_top) { o._ctx = nullptr; }

Model::~Model() {
    if (_ctx) xh_destroy(_ctx);
}

void Model::forward(InferenceState& s, const int token, const int pos, const InferenceMode mode) const {
    float* out = mode == InferenceMode::OUTPUT_LOGITS ? s.logits() : nullptr;
    check(xh_forward(_ctx, token, pos, (int)mode, out), _ctx, "xh_forward");
}

void Model::prefill(InferenceState& s, const std::vector<int>& tokens, const int pos0) const {
    if (tokens.empty()) return;
    check(xh_prefill(_ctx, tokens.data(), (int)tokens.size(), pos0, 1, s.logits()), _ctx, "xh_prefill");
}

std::vector<int> Model::decode_greedy(const int pos, const int n_steps, const int stop_a, const int stop_b) const {
    std::vector<int> toks((size_t)std::max(n_steps, 1));
    int done = 0;
    check(xh_decode_greedy(_ctx, pos, n_steps, stop_a, stop_b, toks.data(), &done), _ctx, "xh_decode_greedy");
    toks.resize((size_t)done);
    return toks;
}

std::vector<int> Model::decode_sample(const int pos, const int n_steps, const xh_sampling& sampling, const int stop_a,
                                      const int stop_b) const {
    std::vector<int> toks((size_t)std::max(n_steps, 1));
    int done = 0;
    check(xh_decode_sample(_ctx, pos, n_steps, &sampling, stop_a, stop_b, toks.data(), &done), _ctx,
          "xh_decode_sample");
    toks.resize((size_t)done);
    return toks;
}

std::vector<int> Model::decode_sample_ext(const int pos, const int n_steps, const xh_sampling& sampling,
                                          const xh_logit_ctl& ctl, const std::vector<int>& history, const int stop_a,
                                          const int stop_b, std::vector<float>* logprobs) const {
    std::vector<int> toks((size_t)std::max(n_steps, 1));
    std::vector<float> lp((size_t)std::max(n_steps, 1));
    int done = 0;
    check(xh_decode_sample_ext(_ctx, pos, n_steps, &sampling, &ctl, history.data(), (int)history.size(), stop_a, stop_b,
                               toks.data(), lp.data(), &done),
          _ctx, "xh_decode_sample_ext");
    toks.resize((size_t)done);
    lp.resize((size_t)done);
    if (logprobs) *logprobs = lp;
    return toks;
}

void Model::set_constraint(const Constraint& c) const {
    check(xh_constraint_set_vocab(_ctx, c.bytes.data(), c.offsets.data()), _ctx, "xh_constraint_set_vocab");
    const xh_byte_dfa d = c.dfa();
    check(xh_constraint_set(_ctx, &d), _ctx, "xh_constraint_set");
}

std::vector<int> Model::decode_sample_dfa(const int pos, const int n_steps, const xh_sampling& sampling,
                                          const xh_logit_ctl& ctl, const std::vector<int>& history,
                                          const uint32_t state_in, const int stop_a, const int stop_b,
                                          uint32_t* state_out, std::vector<float>* logprobs) const {
    std::vector<int> toks((size_t)std::max(n_steps, 1));
    std::vector<float> lp((size_t)std::max(n_steps, 1));
    int done = 0;
    check(xh_decode_sample_dfa(_ctx, pos, n_steps, &sampling, &ctl, history.data(), (int)history.size(), state_in, stop_a,
                               stop_b, toks.data(), lp.data(), state_out, &done),
          _ctx, "xh_decode_sample_dfa");
    toks.resize((size_t)done);
    lp.resize((size_t)done);
    if (logprobs) *logprobs = lp;
    return toks;
}

std::vector<int> Model::decode_sample_adapt(const int pos, const int n_steps, const xh_sampling& sampling,
                                            const xh_logit_ctl& ctl, const xh_trunc_ctl& trunc,
                                            const std::vector<int>& history, const bool constrain,
                                            const uint32_t state_in, const float mu_in, const int stop_a, const int stop_b,
                                            uint32_t* state_out, float* mu_out, std::vector<float>* logprobs) const {
    std::vector<int> toks((size_t)std::max(n_steps, 1));
    std::vector<float> lp((size_t)std::max(n_steps, 1));
    int done = 0;
    check(xh_decode_sample_adapt(_ctx, pos, n_steps, &sampling, &ctl, &trunc, history.data(), (int)history.size(),
                                 constrain ? 1 : 0, state_in, mu_in, stop_a, stop_b, toks.data(), lp.data(), state_out,
                                 mu_out, &done),
          _ctx, "xh_decode_sample_adapt");
    toks.resize((size_t)done);
    lp.resize((size_t)done);
    if (logprobs) *logprobs = lp;
    return toks;
}

std::vector<int> Model::decode_sample_seq(const int pos, const int n_steps, const xh_sampling& sampling,
                                          const xh_logit_ctl& ctl, const xh_trunc_ctl& trunc, const xh_seq_ctl& seq,
                                          const std::vector<int>& history, const bool constrain, const uint32_t state_in,
                                          const float mu_in, const int stop_a, const int stop_b, uint32_t* state_out,
                                          float* mu_out, std::vector<float>* logprobs) const {
    std::vector<int> toks((size_t)std::max(n_steps, 1));
    std::vector<float> lp((size_t)std::max(n_steps, 1));
    int done = 0;
    check(xh_decode_sample_seq(_ctx, pos, n_steps, &sampling, &ctl, &trunc, &seq, history.data(), (int)history.size(),
                               constrain ? 1 : 0, state_in, mu_in, stop_a, stop_b, toks.data(), lp.data(), state_out, mu_out,
                               &done),
          _ctx, "xh_decode_sample_seq");
    toks.resize((size_t)done);
    lp.resize((size_t)done);
    if (logprobs) *logprobs = lp;
    return toks;
}

Constraint Constraint::compile(const std::string& regex, const Tokenizer& tokenizer) {
    Constraint c;
    int rc = xh_regex_compile(regex.c_str(), nullptr, nullptr, 0, &c.n_states, &c.start);
    if (rc == XH_E_NOMEM) {  // the size query
        c.next.resize((size_t)c.n_states * 256);
        c.accept.resize((size_t)c.n_states);
        rc = xh_regex_compile(regex.c_str(), c.next.data(), c.accept.data(), c.n_states, &c.n_states, &c.start);
    }
    if (rc != XH_OK)
        throw std::invalid_argument("-R: not a supported regular expression, or one no text matches: " + regex);
    tokenizer.pieces(c.bytes, c.offsets);
    return c;
}

std::vector<float> Model::token_probs(const std::vector<int>& tokens, const int pos0) const {
    if (tokens.size() < 2) return {};
    std::vector<float> p(tokens.size() - 1);
    check(xh_perplexity(_ctx, tokens.data(), (int)tokens.size(), pos0, p.data()), _ctx, "xh_perplexity");
    return p;
}

void Model::set_top_logprobs(const int n_top) const {
    check(xh_set_top_logprobs(_ctx, n_top), _ctx, "xh_set_top_logprobs");
    _n_top = n_top;
}

Model::TopLogprobs Model::top_logprobs(const int n_steps) const {
    TopLogprobs t;
    t.n_top = _n_top;
    t.ids.resize((size_t)std::max(n_steps, 1) * (size_t)std::max(_n_top, 1));
    t.lps.resize(t.ids.size());
    t.ranks.resize((size_t)std::max(n_steps, 1));
    check(xh_get_top_logprobs(_ctx, n_steps, t.ids.data(), t.lps.data(), t.ranks.data()), _ctx, "xh_get_top_logprobs");
    t.ids.resize((size_t)n_steps * (size_t)_n_top);
    t.lps.resize(t.ids.size());
    t.ranks.resize((size_t)n_steps);
    return t;
}

Model::Score Model::score(const std::vector<int>& tokens, const int pos0, const int n_top) const {
    Score r;
    r.n_top = n_top;
    if (tokens.size() < 2) return r;
    const size_t m = tokens.size() - 1;
    r.logprobs.resize(m);
    r.ranks.resize(m);
    r.top_ids.resize(m * (size_t)std::max(n_top, 0));
    r.top_lps.resize(r.top_ids.size());
    check(xh_score(_ctx, tokens.data(), (int)tokens.size(), pos0, n_top, r.logprobs.data(), r.ranks.data(),
                   n_top > 0 ? r.top_ids.data() : nullptr, n_top > 0 ? r.top_lps.data() : nullptr, nullptr),
          _ctx, "xh_score");
    return r;
}

void Model::fetch_logits(InferenceState& s) const { check(xh_get_logits(_ctx, s.logits()), _ctx, "xh_get_logits"); }

size_t Model::active_bytes(const size_t pos) const { return xh_active_bytes(_ctx, pos); }

// ---- Tokenizer, src/tokenizer.cpp:23-119 ---------------------------------------------------
namespace {
std::vector<int> parse_ids(const std::string& input) {
    std::vector<int> r;
    if (!input.empty() && input.front() == '[' && input.back() == ']') {
        std::string t = input.substr(1, input.size() - 2);
        size_t i = 0;
        while (i < t.size()) {
            size_t j = t.find(',', i);
            if (j == std::string::npos) j = t.size();
            r.push_back(std::stoi(t.substr(i, j - i)));
            i = j + 1;
        }
    } else {
        r.push_back(std::stoi(input));
    }
    return r;
}
}  // namespace

Tokenizer::Tokenizer(const XalmFile& data) {
    bos_id = parse_ids(data.meta("bos_token_id"))[0];
    eos_id = parse_ids(data.meta("eos_token_id"))[0];
    const TensorInfo& ti = data.tensors.at("tokenizer.tokens");
    if (ti.type != XH_U8) throw std::invalid_argument("tokenizer.tokens must be U8");
    const std::vector<uint8_t> raw = data.read("tokenizer.tokens");
    const char* p = (const char*)raw.data();
    const char* end = p + raw.size();
    while (p < end) {
        const char* s = p;
        while (p < end && *p != '\0') p++;
        vocab.emplace_back(s, (size_t)(p - s));
        p++;
    }
    for (size_t i = 0; i < vocab.size(); i++) {
        if (vocab[i] == "<0x00>") byte_fallback_start = (int)i;
        else if (vocab[i] == "<|eot_id|>" || vocab[i] == "<|end|>" || vocab[i] == "<|im_end|>") eot_id = (int)i;
    }
    for (int i = 0; i < 256; i++) byte_pieces[i] = std::string(1, (char)i);
    for (size_t i = 0; i < vocab.size(); i++) {
        TokenTrie* n = &vocab_trie;
        for (char ch : vocab[i]) {
            auto& child = n->children[ch];
            if (!child) child = std::make_unique<TokenTrie>();
            n = child.get();
        }
        n->token_id = (int)i;
    }
}

std::string Tokenizer::decode_one(const int prev_token, const int token) const {
    const std::string& piece = vocab[token];
    if (prev_token == bos_id && !piece.empty() && piece[0] == ' ') return piece.substr(1);
    if (byte_fallback_start >= 0 && token >= byte_fallback_start && token - byte_fallback_start < 256)
        return byte_pieces[token - byte_fallback_start];
    return piece;
}

void Tokenizer::pieces(std::vector<uint8_t>& bytes, std::vector<uint32_t>& offsets) const {
    bytes.clear();
    offsets.assign(1, 0u);
    for (size_t t = 0; t < vocab.size(); t++) {
        const bool fallback = byte_fallback_start >= 0 && (int)t >= byte_fallback_start && (int)t - byte_fallback_start < 256;
        const std::string& piece = fallback ? byte_pieces[t - (size_t)byte_fallback_start] : vocab[t];
        bytes.insert(bytes.end(), piece.begin(), piece.end());
        offsets.push_back((uint32_t)bytes.size());
    }
    if (bytes.empty()) bytes.push_back(0);  // data() stays non-null
}

std::vector<int> Tokenizer::default_breakers() const {
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> offsets;
    pieces(bytes, offsets);
    std::vector<int> out;
    for (size_t t = 0; t + 1 < offsets.size() && out.size() < (size_t)XH_SEQ_MAX_BREAKERS; t++)
        for (uint32_t i = offsets[t]; i < offsets[t + 1]; i++)
            if (bytes[i] == '\n' || bytes[i] == ':' || bytes[i] == '"' || bytes[i] == '*') {
                out.push_back((int)t);
                break;
            }
    return out;
}

// greedy longest match over the vocab trie with byte fallback (src/tokenizer.cpp:82-119)
std::vector<int> Tokenizer::encode(const std::string& text, const bool encode_bos) const {
    std::vector<int> out;
    if (encode_bos) out.push_back(bos_id);
    for (size_t i = 0; i < text.size();) {
        size_t l = 0, valid_l = 0;
        const TokenTrie* p = &vocab_trie;
        const TokenTrie* valid_p = nullptr;
        while (i + l < text.size()) {
            auto it = p->children.find(text[i + l]);
            if (it == p->children.end()) break;
            p = it->second.get();
            l += 1;
            if (p->token_id >= 0) { valid_p = p; valid_l = l; }
        }
        if (!valid_p) {
            if (byte_fallback_start >= 0) out.push_back((unsigned char)text[i] + byte_fallback_start);
            i += 1;
        } else {
            out.push_back(valid_p->token_id);
            i += valid_l;
        }
    }
    return out;
}

// ---- Sampler, src/sampler.cpp:3-30 (max starts at FLT_MIN; first maximum wins) -------------
int Sampler::sample_argmax(const InferenceState& s) const {
    const float* logits = s.logits();
    int argmax = 0;
    float max_val = std::numeric_limits<float>::min();
    for (int i = 0; i < vocab_size; ++i)
        if (logits[i] > max_val) { max_val = logits[i]; argmax = i; }
    return argmax;
}

void Sampler::top_logprobs(const InferenceState& s, const int n_top, const int token, std::vector<int>& ids,
                           std::vector<float>& lps, float& token_lp, int& token_rank) const {
    ids.assign((size_t)std::max(n_top, 1), 0);
    lps.assign(ids.size(), 0.f);
    if (xh_top_logprobs_host(s.logits(), vocab_size, 1, n_top, &token, ids.data(), lps.data(), &token_lp, &token_rank))
        throw std::invalid_argument("top_logprobs: 1 <= n_top <= min(XH_TOP_MAX, vocab) and a token of the vocabulary");
    ids.resize((size_t)n_top);
    lps.resize((size_t)n_top);
}

float Sampler::sample_prob(const int index, const InferenceState& s) const {
    const float* logits = s.logits();
    float max_val = std::numeric_limits<float>::min();
    for (int i = 0; i < vocab_size; ++i)
        if (logits[i] > max_val) max_val = logits[i];
    float sum = 0;
    for (int i = 0; i < vocab_size; ++i) sum += expf(logits[i] - max_val);
    return expf(logits[index] - max_val) / sum;
}

// ---- seeded sampling: the definition of xh_sampling (include/xalm_hip.h), restated -------------
int sample_logits(const float* logits, const int vocab, const xh_sampling& p, const uint64_t pos, int* n_kept,
                  const float min_p) {
    if (!logits || vocab <= 0) throw std::invalid_argument("sample: no logits");
    if (!(p.temperature >= 0.f) || p.top_k < 0 || !(p.top_p > 0.f && p.top_p <= 1.f))
        throw std::invalid_argument("sample: temperature >= 0, top_k >= 0, top_p in (0, 1]");
    if (!(min_p >= 0.f && min_p <= 1.f)) throw std::invalid_argument("sample: min_p in [0, 1]");
    int kept_n = 1;
    int token = 0;
    const auto done = [&] {
        if (n_kept) *n_kept = kept_n;
        return token;
    };
    if (p.temperature == 0.f) {  // Sampler::sample_argmax
        float max_val = std::numeric_limits<float>::min();
        for (int i = 0; i < vocab; ++i)
            if (logits[i] > max_val) { max_val = logits[i]; token = i; }
        return done();
    }
    float m = logits[0];
    int first_max = 0;
    for (int i = 1; i < vocab; ++i)
        if (logits[i] > m) { m = logits[i]; first_max = i; }
    if (!std::isfinite(m)) {  // no finite logit: token 0 (+inf, outside the definition: the first of them)
        kept_n = m > 0 ? 1 : 0;
        token = m > 0 ? first_max : 0;
        return done();
    }
    std::vector<double> w((size_t)vocab);
    for (int i = 0; i < vocab; ++i)
        w[i] = logits[i] == -std::numeric_limits<float>::infinity() ? 0.0 : (double)expf((logits[i] - m) / p.temperature);
    // logit descending by its f32 bits, then index ascending
    const auto key = [&](const int i) {
        uint32_t u;
        memcpy(&u, &logits[i], 4);
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    };
    std::vector<int> order((size_t)vocab);
    std::iota(order.begin(), order.end(), 0);
    size_t n = p.top_k > 0 && p.top_k < vocab ? (size_t)p.top_k : (size_t)vocab;
    if (min_p > 0.f) {  // a prefix of the order: the weight is monotone in the logit
        size_t n_minp = 0;
        for (int i = 0; i < vocab; ++i)
            n_minp += logits[i] != -std::numeric_limits<float>::infinity() && expf((logits[i] - m) / p.temperature) >= min_p;
        if (n_minp >= 1 && n_minp < n) n = n_minp;
    }
    if (n < (size_t)vocab || p.top_p < 1.f) {
        const auto before = [&](const int a, const int b) {
            const uint32_t ka = key(a), kb = key(b);
            return ka != kb ? ka > kb : a < b;
        };
        if (p.top_p < 1.f) std::sort(order.begin(), order.end(), before);
        else std::partial_sort(order.begin(), order.begin() + (long)n, order.end(), before);
    }
    if (p.top_p < 1.f) {
        double total = 0.0;
        for (size_t j = 0; j < n; ++j) total += w[order[j]];
        const double want = (double)p.top_p * total;
        double cum = 0.0;
        size_t j = 0;
        do cum += w[order[j++]];
        while (j < n && cum < want);
        n = j;
    }
    std::vector<char> kept((size_t)vocab, 0);
    for (size_t j = 0; j < n; ++j) kept[order[j]] = 1;
    kept_n = (int)n;
    uint32_t x[4];
    xh_philox4x32(p.seed, pos, x);
    const double u = (double)(x[0] >> 8) * (1.0 / 16777216.0);
    double total = 0.0;
    for (int i = 0; i < vocab; ++i)
        if (kept[i]) total += w[i];
    const double thr = u * total;
    double cum = 0.0;
    token = first_max;  // rounding left no cumulative weight above thr: cannot happen for u < 1
    for (int i = 0; i < vocab; ++i)
        if (kept[i]) {
            cum += w[i];
            if (cum > thr) { token = i; break; }
        }
    return done();
}

int Sampler::sample(const InferenceState& s, const xh_sampling& sampling, const int pos) const {
    return sample_logits(s.logits(), vocab_size, sampling, (uint64_t)pos, nullptr);
}

int Sampler::sample(const InferenceState& s, const xh_sampling& sampling, const xh_logit_ctl& ctl,
                    const std::vector<int>& history, const int pos) const {
    std::vector<float> adj((size_t)vocab_size);
    const size_t n_win = std::min(history.size(), (size_t)XH_CTL_MAX_WINDOW);
    if (xh_adjust_logits(s.logits(), vocab_size, &ctl, history.data() + (history.size() - n_win), (int)n_win, adj.data()))
        throw std::invalid_argument(std::string("sample: ") + xh_last_error(nullptr));
    return sample_logits(adj.data(), vocab_size, sampling, (uint64_t)pos, nullptr, ctl.min_p);
}

int Sampler::sample(const InferenceState& s, const xh_sampling& sampling, const xh_logit_ctl& ctl,
                    const std::vector<int>& history, const int pos, const Constraint& constraint, uint32_t& state,
                    const int stop_a, const int stop_b) const {
    const int stuck = stop_a >= 0 ? stop_a : stop_b >= 0 ? stop_b : 0;
    if (state == XH_DFA_DEAD) return stuck;
    std::vector<float> adj((size_t)vocab_size);
    const size_t n_win = std::min(history.size(), (size_t)XH_CTL_MAX_WINDOW);
    if (xh_adjust_logits(s.logits(), vocab_size, &ctl, history.data() + (history.size() - n_win), (int)n_win, adj.data()))
        throw std::invalid_argument(std::string("sample: ") + xh_last_error(nullptr));
    std::vector<uint8_t> allowed((size_t)vocab_size);
    std::vector<uint16_t> succ((size_t)vocab_size);
    const xh_byte_dfa d = constraint.dfa();
    if (xh_constraint_mask(&d, constraint.bytes.data(), constraint.offsets.data(), vocab_size, state, stop_a, stop_b,
                           allowed.data(), succ.data()))
        throw std::invalid_argument("sample: bad constraint or state");
    // logit descending by its f32 bits, then index ascending, among the allowed tokens
    const auto key = [&](const int i) {
        uint32_t u;
        memcpy(&u, &adj[(size_t)i], 4);
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    };
    int first = -1;
    for (int i = 0; i < vocab_size; ++i) {
        if (!allowed[(size_t)i]) adj[(size_t)i] = -std::numeric_limits<float>::infinity();
        else if (first < 0 || key(i) > key(first)) first = i;
    }
    if (first < 0) {  // stuck
        state = XH_DFA_DEAD;
        return stuck;
    }
    const int token = sampling.temperature == 0.f
                          ? first
                          : sample_logits(adj.data(), vocab_size, sampling, (uint64_t)pos, nullptr, ctl.min_p);
    state = succ[(size_t)token];
    return token;
}

int Sampler::sample(const InferenceState& s, const xh_sampling& sampling, const xh_logit_ctl& ctl,
                    const xh_trunc_ctl& trunc, const std::vector<int>& history, const int pos,
                    const Constraint* constraint, uint32_t& state, float& mu, const int stop_a, const int stop_b) const {
    return sample_adapt_logits(s.logits(), vocab_size, sampling, ctl, trunc, history, pos, constraint, state, mu, stop_a,
                               stop_b);
}

int Sampler::sample(const InferenceState& s, const xh_sampling& sampling, const xh_logit_ctl& ctl,
                    const xh_trunc_ctl& trunc, const xh_seq_ctl& seq, const std::vector<int>& history, const int pos,
                    const Constraint* constraint, uint32_t& state, float& mu, const int stop_a, const int stop_b) const {
    return sample_seq_logits(s.logits(), vocab_size, sampling, ctl, trunc, &seq, history, pos, constraint, state, mu, stop_a,
                             stop_b);
}

int sample_adapt_logits(const float* logits, const int vocab_size, const xh_sampling& sampling, const xh_logit_ctl& ctl,
                        const xh_trunc_ctl& trunc, const std::vector<int>& history, const int pos,
                        const Constraint* constraint, uint32_t& state, float& mu, const int stop_a, const int stop_b) {
    return sample_seq_logits(logits, vocab_size, sampling, ctl, trunc, nullptr, history, pos, constraint, state, mu, stop_a,
                             stop_b);
}

int sample_seq_logits(const float* logits, const int vocab_size, const xh_sampling& sampling, const xh_logit_ctl& ctl,
                      const xh_trunc_ctl& trunc, const xh_seq_ctl* seq, const std::vector<int>& history, const int pos,
                      const Constraint* constraint, uint32_t& state, float& mu, const int stop_a, const int stop_b) {
    if (!logits || vocab_size <= 0) throw std::invalid_argument("sample: no logits");
    if (seq && trunc.mirostat_tau > 0.f && seq->xtc_probability != 0.f)
        throw std::invalid_argument("sample: Mirostat takes xtc_probability 0");
    constexpr float NEG_INF = -std::numeric_limits<float>::infinity();
    if (mu < 0.f) mu = 2.f * trunc.mirostat_tau;
    const int stuck = stop_a >= 0 ? stop_a : stop_b >= 0 ? stop_b : 0;
    if (constraint && state == XH_DFA_DEAD) return stuck;
    std::vector<float> adj((size_t)vocab_size);
    const size_t n_win = std::min(history.size(), (size_t)XH_CTL_MAX_WINDOW);
    if (xh_adjust_logits(logits, vocab_size, &ctl, history.data() + (history.size() - n_win), (int)n_win, adj.data()))
        throw std::invalid_argument(std::string("sample: ") + xh_last_error(nullptr));
    // DRY and the n-gram ban: behind the adjustment, in front of the mask
    if (seq && xh_seq_adjust_host(adj.data(), vocab_size, seq, history.data() + (history.size() - n_win), (int)n_win,
                                  adj.data(), nullptr, nullptr))
        throw std::invalid_argument("sample: xh_seq_ctl outside its definition");
    std::vector<uint16_t> succ;
    int first = -1;  // the first allowed token of the order
    if (constraint) {
        std::vector<uint8_t> allowed((size_t)vocab_size);
        succ.resize((size_t)vocab_size);
        const xh_byte_dfa d = constraint->dfa();
        if (xh_constraint_mask(&d, constraint->bytes.data(), constraint->offsets.data(), vocab_size, state, stop_a, stop_b,
                               allowed.data(), succ.data()))
            throw std::invalid_argument("sample: bad constraint or state");
        const auto key = [&](const int i) {
            uint32_t u;
            memcpy(&u, &adj[(size_t)i], 4);
            return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        };
        for (int i = 0; i < vocab_size; ++i) {
            if (!allowed[(size_t)i]) adj[(size_t)i] = NEG_INF;
            else if (first < 0 || key(i) > key(first)) first = i;
        }
        if (first < 0) {
            state = XH_DFA_DEAD;
            return stuck;
        }
    }
    int token;
    if (sampling.temperature == 0.f) {
        token = constraint ? first : sample_logits(adj.data(), vocab_size, sampling, (uint64_t)pos, nullptr, 0.f);
    } else {
        std::vector<uint8_t> kept((size_t)vocab_size);
        if (xh_truncate_host(adj.data(), vocab_size, &sampling, ctl.min_p, &trunc, mu, -1, kept.data(), nullptr, nullptr,
                             nullptr))
            throw std::invalid_argument("sample: xh_trunc_ctl outside its definition");
        // XTC over the set the typical stage left, at this draw's counter
        if (seq && seq->xtc_probability > 0.f &&
            xh_xtc_host(adj.data(), vocab_size, sampling.temperature, seq, sampling.seed, (uint64_t)pos, kept.data(), nullptr,
                        nullptr))
            throw std::invalid_argument("sample: xh_seq_ctl outside its definition");
        std::vector<float> cut(adj);
        for (int i = 0; i < vocab_size; ++i)
            if (!kept[(size_t)i]) cut[(size_t)i] = NEG_INF;
        xh_sampling rest = sampling;  // top-p and the draw over the survivors
        rest.top_k = 0;
        token = sample_logits(cut.data(), vocab_size, rest, (uint64_t)pos, nullptr, 0.f);
        if (trunc.mirostat_tau > 0.f)
            xh_truncate_host(adj.data(), vocab_size, &sampling, ctl.min_p, &trunc, mu, token, nullptr, nullptr, nullptr, &mu);
    }
    if (constraint) state = succ[(size_t)token];
    return token;
}

}  // namespace xalm
