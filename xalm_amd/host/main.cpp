// main.cpp — `xalm` CLI: the reference's argument surface (jubruckne/Xalm src/main.cpp:381-549)
// over the MI355X decode path.
//
//   xalm <checkpoint.xalm> [-m completion|perplexity] [-d hip|cpu] [-i prompt | -f file]
//                          [-T context] [-n steps] [-g 0|1] [-t temperature] [-k top_k] [-p top_p] [-s seed]
//                          [-r repeat_penalty] [-w window] [-P presence] [-F frequency] [-M min_p] [-R regex]
//                          [-L top_logprobs] [-y typical_p] [-S n_sigma] [-U mirostat_tau] [-E mirostat_eta]
//                          [-D dry_multiplier] [-B dry_base] [-A dry_allowed_length] [-N no_repeat_ngram]
//                          [-W sequence window] [-X xtc_probability] [-x xtc_threshold]
//
// -d selects the device as in the reference (src/main.cpp:465-477); this build ships the HIP
// device.  -g 1 runs the greedy loop on the device (no host round trip per token); -g 0
// (default) samples on the host each step exactly like run_completion (src/main.cpp:105-115).
// -t > 0 samples (xh_sampling, include/xalm_hip.h): on the device with -g 1, with the host Sampler::sample
// with -g 0.  -r / -w / -P / -F / -M (xh_logit_ctl) penalise the tokens of the last -w ids of prompt +
// output and cut by min-p, at any temperature: xh_decode_sample_ext with -g 1, the host Sampler over
// xh_adjust_logits with -g 0.
// -R constrains the output to a regular expression matched against the whole generated text
// (xh_regex_compile, xh_byte_dfa): xh_decode_sample_dfa with -g 1, the host Sampler over
// xh_constraint_mask with -g 0; eos / eot may end the text where the expression is matched.
// -L n (1 .. 32) prints, per generated token, its rank and the n most likely tokens of the raw logits
// with their log-probabilities (XH_TOP_MAX, include/xalm_hip.h): xh_set_top_logprobs with -g 1, the
// host Sampler over xh_top_logprobs_host with -g 0; in perplexity mode, how often the scored token
// had rank 0 (xh_score).
// -y / -S / -U / -E (xh_trunc_ctl) cut by local typicality, by n standard deviations below the
// maximum logit, or by Mirostat v2's running target: xh_decode_sample_adapt with -g 1, the host
// Sampler over xh_truncate_host with -g 0.
// -D / -B / -A / -N / -W / -X / -x (xh_seq_ctl) penalise the token that would extend a repeat of the
// recent text (DRY), ban the token that would complete an n-gram already in it, and with probability
// -X drop every token above probability -x but the least likely of them (XTC): xh_decode_sample_seq
// with -g 1, the host Sampler over xh_seq_adjust_host and xh_xtc_host with -g 0.  DRY's breakers are
// the tokens whose piece contains a newline, ':', '"' or '*'; only the 1024 (XH_SEQ_MAX_BREAKERS)
// lowest ids of them are taken.
// Stats are wall clock (the reference divides by user+sys CPU time, src/profiler.h:124-129).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "xalm.h"

using namespace xalm;
using clk = std::chrono::steady_clock;

static int g_kv_dtype = XH_F16;  // -K: the KV rings' element type
static int g_attn_kv8 = 0;       // -a: 1 = XH_OPT_PREFILL_ATTN_KV8, 2 = that and XH_OPT_PREFILL_RING_KV8

// the model of a run: -K's rings, -a's prompt attention (and ring passes) on them
static Model load_model(const XalmFile& file, int context, Device dev) {
    Model model = Model::from_xalm(file, context, dev, 0, g_kv_dtype);
    const bool ring = g_attn_kv8 == 2;
    if (g_attn_kv8 && (xh_set_option(model.ctx(), XH_OPT_PREFILL_ATTN_KV8, ring ? 1 : g_attn_kv8) != 0 ||
                       (ring && xh_set_option(model.ctx(), XH_OPT_PREFILL_RING_KV8, 1) != 0)))
        throw std::runtime_error(std::string("-a: ") + xh_last_error(model.ctx()));
    return model;
}

static void error_usage() {
    fprintf(stderr, "Usage:   xalm <checkpoint> [options]\n");
    fprintf(stderr, "Example: xalm model.xalm -i \"Q: What is the meaning of life?\"\n");
    fprintf(stderr, "Options:\n");
    fprintf(stderr, "  -h Display this help message\n");
    fprintf(stderr, "  -d [hip,cpu] which device to use (default - hip)\n");
    fprintf(stderr, "  -m [completion,perplexity] which mode to run in (default - completion)\n");
    fprintf(stderr, "  -T <int> sliding window context length (0 - max)\n");
    fprintf(stderr, "  -n <int> number of steps in completion mode, default 128. 0 = max_seq_len, -1 = infinite\n");
    fprintf(stderr, "  -g <0|1> decode loop on the device (default 0)\n");
    fprintf(stderr, "  -K [f16,f8] KV ring element type (default f16; f8 = e4m3, hip only)\n");
    fprintf(stderr, "  -a <0|1|2> with -K f8: 1 = prompt attention on the MFMA kernels' fp8 tiles, 2 = that and batched\n");
    fprintf(stderr, "     ring passes past the context length (default 0, hip only)\n");
    fprintf(stderr, "  -t <float> sampling temperature (default 0 - greedy)\n");
    fprintf(stderr, "  -k <int> top-k, 0 = off (default 0)\n");
    fprintf(stderr, "  -p <float> top-p in (0, 1], 1 = off (default 1)\n");
    fprintf(stderr, "  -s <int> sampling seed (default 0); -g 0 and -g 1 draw from the same definition and print\n");
    fprintf(stderr, "     the same ids for a seed, except where a draw falls within rounding of a boundary\n");
    fprintf(stderr, "  -r <float> repeat penalty > 0, 1 = off (default 1)\n");
    fprintf(stderr, "  -w <int> penalty window: the last 0 .. 1024 ids of prompt + output (default 64; 0 = penalties off)\n");
    fprintf(stderr, "  -P <float> presence penalty, 0 = off (default 0)\n");
    fprintf(stderr, "  -F <float> frequency penalty, 0 = off (default 0)\n");
    fprintf(stderr, "  -M <float> min-p in [0, 1], 0 = off (default 0)\n");
    fprintf(stderr, "  -R <regex> constrain the generated text to this regular expression (whole match, bytes)\n");
    fprintf(stderr, "  -L <int> per generated token, print its rank and the 1 .. 32 most likely tokens with their\n");
    fprintf(stderr, "     log-probabilities; in perplexity mode, how often the scored token had rank 0 (default 0 - off)\n");
    fprintf(stderr, "  -y <float> locally typical sampling: typical-p in (0, 1], 1 = off (default 1)\n");
    fprintf(stderr, "  -S <float> top-n-sigma: keep logits within n standard deviations of the maximum, 0 = off (default 0)\n");
    fprintf(stderr, "  -U <float> Mirostat v2 target surprise tau in bits, 0 = off (default 0); takes -k 0 -p 1 -M 0 -y 1 -S 0\n");
    fprintf(stderr, "  -E <float> Mirostat v2 learning rate eta > 0 (default 0.1)\n");
    fprintf(stderr, "  -D <float> DRY multiplier, 0 = off (default 0): the penalty is D * B^(repeat length - A)\n");
    fprintf(stderr, "  -B <float> DRY base >= 1 (default 1.75)\n");
    fprintf(stderr, "  -A <int> DRY allowed length 1 .. 64: shorter repeats are free (default 2)\n");
    fprintf(stderr, "     breakers: the tokens holding a newline, ':', '\"' or '*', the 1024 lowest ids of them at most\n");
    fprintf(stderr, "  -N <int> ban the token that would complete an n-gram already present, 2 .. 64, 0 = off (default 0)\n");
    fprintf(stderr, "  -W <int> sequence window of -D and -N: the last 0 .. 1024 ids of prompt + output (default 1024)\n");
    fprintf(stderr, "  -X <float> XTC probability in [0, 1], 0 = off (default 0); not with -U\n");
    fprintf(stderr, "  -x <float> XTC threshold in (0, 1] (default 0.1)\n");
    fprintf(stderr, "  Choose one:\n");
    fprintf(stderr, "    -i <string> input prompt\n");
    fprintf(stderr, "    -f <filepath> input file with prompt\n");
    exit(1);
}

static double secs(clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); }

static void print_ids(const std::vector<int>& ids) {
    printf("tokens: [");
    for (size_t i = 0; i < ids.size(); i++) printf(i ? ",%d" : "%d", ids[i]);
    printf("]\n");
}

// run_completion, src/main.cpp:44-128
static void print_top(int token, int rank, const int* ids, const float* lps, int n) {
    printf("top: token %d rank %d |", token, rank);
    for (int j = 0; j < n; j++) printf(" %d:%.6g", ids[j], lps[j]);
    printf("\n");
}

static void run_completion(const std::string& path, Device dev, const std::string& prompt, int context, int num_steps,
                           bool device_loop, const xh_sampling& sampling, const xh_logit_ctl& ctl,
                           const xh_trunc_ctl& trunc, xh_seq_ctl seq, const std::string& regex, int top_n) {
    const XalmFile file = XalmFile::load(path);
    const Model model = load_model(file, context, dev);
    InferenceState state(model.config);
    const Sampler sampler(model.config);
    const Tokenizer tokenizer(file);
    printf("Model active bytes(m): %zu\n", model.active_bytes(model.config.max_seq_len) / (1024 * 1024));
    if (num_steps == 0) num_steps = model.config.max_seq_len;
    model.forward(state, 0, 0);  // warm-up, as the reference (src/main.cpp:72)

    std::vector<int> encoding = tokenizer.encode(prompt, true);
    const size_t n_prompt = encoding.size();
    const auto t0 = clk::now();
    size_t read_bytes = 0;
    // the hydrate loop (src/main.cpp:94-100) as one xh_prefill call
    model.prefill(state, encoding, 0);
    for (size_t pos = 0; pos < encoding.size(); pos++) read_bytes += model.active_bytes(pos);
    const auto t1 = clk::now();
    // any control on: the extended draw on both routes, prompt + output as the history
    const bool ext = ctl.repeat_penalty != 1.f || ctl.presence_penalty != 0.f || ctl.frequency_penalty != 0.f ||
                     ctl.min_p != 0.f;
    // any truncation on: the adaptive draw on both routes
    const bool adapt = trunc.typical_p != 1.f || trunc.top_n_sigma != 0.f || trunc.mirostat_tau != 0.f;
    // any sequence stage on: the sequence-aware draw on both routes, with the default breakers
    const bool seq_on = seq.dry_multiplier != 0.f || seq.no_repeat_ngram != 0 || seq.xtc_probability != 0.f;
    const std::vector<int> breakers = seq_on ? tokenizer.default_breakers() : std::vector<int>();
    seq.n_breakers = (int)breakers.size();
    seq.breaker_token = breakers.data();
    float mu = 2.f * trunc.mirostat_tau;
    Constraint constraint;
    uint32_t dfa_state = 0;
    if (!regex.empty()) {
        constraint = Constraint::compile(regex, tokenizer);
        dfa_state = (uint32_t)constraint.start;
        if (device_loop) model.set_constraint(constraint);
    }
    // -L: the generated tokens' top lists, printed after the text
    Model::TopLogprobs tops;
    tops.n_top = top_n;
    if (device_loop && num_steps > 0) {
        if (top_n > 0) model.set_top_logprobs(top_n);
        const std::vector<int> gen =
            seq_on ? model.decode_sample_seq((int)encoding.size(), num_steps, sampling, ctl, trunc, seq, encoding,
                                             !regex.empty(), dfa_state, mu, tokenizer.eos_id, tokenizer.eot_id)
            : adapt ? model.decode_sample_adapt((int)encoding.size(), num_steps, sampling, ctl, trunc, encoding,
                                              !regex.empty(), dfa_state, mu, tokenizer.eos_id, tokenizer.eot_id)
            : !regex.empty() ? model.decode_sample_dfa((int)encoding.size(), num_steps, sampling, ctl, encoding, dfa_state,
                                                     tokenizer.eos_id, tokenizer.eot_id)
            : ext ? model.decode_sample_ext((int)encoding.size(), num_steps, sampling, ctl, encoding, tokenizer.eos_id,
                                          tokenizer.eot_id)
            : sampling.temperature > 0.f
                ? model.decode_sample((int)encoding.size(), num_steps, sampling, tokenizer.eos_id, tokenizer.eot_id)
                : model.decode_greedy((int)encoding.size(), num_steps, tokenizer.eos_id, tokenizer.eot_id);
        if (top_n > 0) tops = model.top_logprobs((int)gen.size());
        for (int t : gen) {
            std::cout << tokenizer.decode_one(encoding.back(), t) << std::flush;
            encoding.push_back(t);
            read_bytes += model.active_bytes(encoding.size() - 1);
        }
    } else {
        for (int i = 0; i < num_steps || num_steps == -1; i++) {
            const int token_id = seq_on ? sampler.sample(state, sampling, ctl, trunc, seq, encoding, (int)encoding.size(),
                                                         regex.empty() ? nullptr : &constraint, dfa_state, mu,
                                                         tokenizer.eos_id, tokenizer.eot_id)
                                 : adapt ? sampler.sample(state, sampling, ctl, trunc, encoding, (int)encoding.size(),
                                                        regex.empty() ? nullptr : &constraint, dfa_state, mu,
                                                        tokenizer.eos_id, tokenizer.eot_id)
                                 : !regex.empty() ? sampler.sample(state, sampling, ctl, encoding, (int)encoding.size(),
                                                                 constraint, dfa_state, tokenizer.eos_id, tokenizer.eot_id)
                                 : ext ? sampler.sample(state, sampling, ctl, encoding, (int)encoding.size())
                                 : sampling.temperature > 0.f ? sampler.sample(state, sampling, (int)encoding.size())
                                                              : sampler.sample_argmax(state);
            if (top_n > 0) {
                std::vector<int> ids;
                std::vector<float> lps;
                float lp = 0.f;
                int rank = 0;
                sampler.top_logprobs(state, top_n, token_id, ids, lps, lp, rank);
                tops.ids.insert(tops.ids.end(), ids.begin(), ids.end());
                tops.lps.insert(tops.lps.end(), lps.begin(), lps.end());
                tops.ranks.push_back(rank);
            }
            std::cout << tokenizer.decode_one(encoding.back(), token_id) << std::flush;
            encoding.push_back(token_id);
            if (token_id == tokenizer.eos_id || token_id == tokenizer.eot_id) break;
            model.forward(state, token_id, (int)encoding.size() - 1);
            read_bytes += model.active_bytes(encoding.size() - 1);
        }
    }
    const auto t2 = clk::now();
    std::cout << "\n" << std::endl;
    for (size_t i = 0; i < tops.ranks.size(); i++)
        print_top(encoding[n_prompt + i], tops.ranks[i], tops.ids.data() + i * (size_t)top_n, tops.lps.data() + i * (size_t)top_n,
                  top_n);
    const double elapsed = secs(t0, t2), decode = secs(t1, t2);
    const size_t gen = encoding.size() - n_prompt;
    printf("Generation stats (wall clock):\n  %zu tokens (%zu prompt + %zu generated)\n  throughput: %.5g tok/s\n"
           "  decode: %.5g tok/s\n  hydrate: %.5gs\n  bandwidth: %.5g GB/s\n  total: %.5gs\n",
           encoding.size(), n_prompt, gen, encoding.size() / elapsed, gen ? gen / decode : 0.0, secs(t0, t1),
           (double)read_bytes / 1e9 / elapsed, elapsed);
    print_ids(encoding);
}

// run_perplexity, src/main.cpp:198-268
static void run_perplexity(const std::string& path, Device dev, const std::string& prompt, int context, int top_n) {
    const XalmFile file = XalmFile::load(path);
    const Model model = load_model(file, context, dev);
    InferenceState state(model.config);
    const Tokenizer tokenizer(file);
    model.forward(state, 0, 0);
    const std::vector<int> encoding = tokenizer.encode(prompt, true);
    double sum_logprob = 0.0, ss_logprob = 0.0;
    const size_t N = encoding.size() - 1;
    const auto t0 = clk::now();
    // the forward + sample_prob loop runs on the device (logits never cross to the host); the
    // log and the double sums stay here, as in the reference
    const std::vector<float> probs = model.token_probs(encoding, 0);
    for (size_t pos = 0; pos < N; pos++) {
        const double logprob = std::log(probs[pos]);
        sum_logprob += logprob;
        ss_logprob += logprob * logprob;
    }
    const double elapsed = secs(t0, clk::now());
    const double ppl = std::exp(-sum_logprob / N);
    const double err = ppl * std::sqrt((ss_logprob - sum_logprob * sum_logprob / N) / N / N);
    printf("Stats:\n  %zu tokens\n  perplexity: %.5g +- %.5g\n  throughput: %.5g tok/s\n  total: %.5gs\n", N, ppl, err,
           N / elapsed, elapsed);
    printf("perplexity: %.9g\n", ppl);
    if (top_n > 0) {
        const Model::Score sc = model.score(encoding, 0, 0);
        size_t first = 0;
        for (int r : sc.ranks) first += r == 0 ? 1 : 0;
        printf("rank 0: %zu of %zu scored tokens (%.4g%%)\n", first, N, 100.0 * (double)first / (double)N);
    }
}

int main(int argc, char** argv) {
    std::string path, mode = "completion", prompt = "Q: What is the meaning of life? A:", prompt_path;
    std::string device = "hip", regex;
    int context = 0, num_steps = 128, device_loop = 0, top_n = 0;
    xh_sampling sampling{0.f, 0, 1.f, 0};
    xh_logit_ctl ctl{1.f, 0.f, 0.f, 64, 0.f, 0, nullptr, nullptr};
    xh_trunc_ctl trunc{1.f, 0.f, 0.f, 0.1f};
    xh_seq_ctl seq{0.f, 1.75f, 2, 0, XH_CTL_MAX_WINDOW, 0, nullptr, 0.f, 0.1f};
    if (argc >= 2) path = argv[1];
    else error_usage();
    for (int i = 2; i < argc;) {
        if (i + 1 >= argc || argv[i][0] != '-' || strlen(argv[i]) != 2) error_usage();
        const char f = argv[i][1];
        const std::string v = argv[i + 1];
        if (f == 'm') {
            if (std::string("completion").rfind(v, 0) == 0) mode = "completion";
            else if (std::string("perplexity").rfind(v, 0) == 0) mode = "perplexity";
            else error_usage();
        } else if (f == 'd') {
            if (std::string("hip").rfind(v, 0) == 0 || std::string("cuda").rfind(v, 0) == 0) device = "hip";
            else if (std::string("cpu").rfind(v, 0) == 0) device = "cpu";
            else error_usage();
        } else if (f == 'i') prompt = v;
        else if (f == 'f') prompt_path = v;
        else if (f == 'T') context = std::stoi(v);
        else if (f == 'n') num_steps = std::stoi(v);
        else if (f == 'g') device_loop = std::stoi(v);
        else if (f == 'K') {
            if (v == "f16") g_kv_dtype = XH_F16;
            else if (v == "f8") g_kv_dtype = XH_F8_E4M3;
            else error_usage();
        }
        else if (f == 'a') g_attn_kv8 = std::stoi(v);
        else if (f == 't') sampling.temperature = std::stof(v);
        else if (f == 'k') sampling.top_k = std::stoi(v);
        else if (f == 'p') sampling.top_p = std::stof(v);
        else if (f == 's') sampling.seed = std::stoull(v);
        else if (f == 'r') ctl.repeat_penalty = std::stof(v);
        else if (f == 'w') ctl.last_n = std::stoi(v);
        else if (f == 'P') ctl.presence_penalty = std::stof(v);
        else if (f == 'F') ctl.frequency_penalty = std::stof(v);
        else if (f == 'M') ctl.min_p = std::stof(v);
        else if (f == 'R') regex = v;
        else if (f == 'L') top_n = std::stoi(v);
        else if (f == 'y') trunc.typical_p = std::stof(v);
        else if (f == 'S') trunc.top_n_sigma = std::stof(v);
        else if (f == 'U') trunc.mirostat_tau = std::stof(v);
        else if (f == 'E') trunc.mirostat_eta = std::stof(v);
        else if (f == 'D') seq.dry_multiplier = std::stof(v);
        else if (f == 'B') seq.dry_base = std::stof(v);
        else if (f == 'A') seq.dry_allowed_length = std::stoi(v);
        else if (f == 'N') seq.no_repeat_ngram = std::stoi(v);
        else if (f == 'W') seq.seq_last_n = std::stoi(v);
        else if (f == 'X') seq.xtc_probability = std::stof(v);
        else if (f == 'x') seq.xtc_threshold = std::stof(v);
        else error_usage();
        i += 2;
    }
    if (!prompt_path.empty()) {
        std::ifstream file(prompt_path);
        if (!file.is_open()) {
            std::cerr << "Error: could not open file " << prompt_path << std::endl;
            return 1;
        }
        std::stringstream buffer;
        buffer << file.rdbuf();
        prompt = buffer.str();
    }
    if (top_n < 0 || top_n > XH_TOP_MAX) {
        fprintf(stderr, "error: -L takes 0 .. %d\n", XH_TOP_MAX);
        return 1;
    }
    if (g_kv_dtype != XH_F16 && device == "cpu") error_usage();  // the fp8 KV ring is the HIP device's
    if (g_attn_kv8 && device == "cpu") error_usage();
    const Device dev = device == "cpu" ? Device::CPU : Device::HIP;
    try {
        if (mode == "completion") run_completion(path, dev, prompt, context, num_steps, device_loop != 0, sampling, ctl, trunc, seq, regex, top_n);
        else run_perplexity(path, dev, prompt, context, top_n);
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
