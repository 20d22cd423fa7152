// constraint.cpp — the host side of regex-constrained decoding (the definition: include/xalm_hip.h,
// xh_byte_dfa): xh_regex_compile (Thompson NFA, subset construction, trimming), xh_constraint_mask
// and the argument checks decode.hip shares.  Plain C++: it builds and runs without HIP.
#include "constraint.h"

#include <algorithm>
#include <array>
#include <bitset>
#include <map>
#include <string>
#include <vector>

namespace xalm {

const char* dfa_error(const xh_byte_dfa* d) {
    if (!d) return "null dfa";
    if (d->n_states < 1 || d->n_states > XH_DFA_MAX_STATES) return "n_states outside 1 .. XH_DFA_MAX_STATES";
    if (d->start < 0 || d->start >= d->n_states) return "start state out of range";
    if (!d->next || !d->accept) return "null dfa table";
    const size_t n = (size_t)d->n_states * 256;
    for (size_t i = 0; i < n; i++)
        if (d->next[i] != XH_DFA_DEAD && d->next[i] >= (uint32_t)d->n_states) return "next entry out of range";
    return nullptr;
}

const char* dfa_state_error(const xh_byte_dfa* d, const uint32_t state) {
    return state == XH_DFA_DEAD || state < (uint32_t)d->n_states ? nullptr : "state out of range";
}

const char* pieces_error(const uint8_t* bytes, const uint32_t* offsets, const int vocab) {
    if (vocab <= 0 || vocab > DFA_MAX_VOCAB) return "vocab outside 1 .. 2^17";
    if (!bytes || !offsets) return "null piece table";
    if (offsets[0] != 0) return "offsets must start at 0";
    for (int t = 0; t < vocab; t++)
        if (offsets[t + 1] < offsets[t]) return "offsets must ascend";
    if (offsets[vocab] > DFA_MAX_PIECE_BYTES) return "piece blob over 16 MiB";
    return nullptr;
}

namespace {

using ByteSet = std::bitset<256>;

// ---- the pattern's syntax tree -----------------------------------------------------------------
struct Node {
    enum Kind { SET, CAT, ALT, REP } kind = SET;
    ByteSet set;            // SET
    std::vector<int> kids;  // CAT / ALT: any number (none = the empty string / CAT only); REP: one
    int lo = 0, hi = 0;     // REP: lo .. hi copies, hi < 0 = unbounded
};

constexpr int MAX_COUNT = 256;
constexpr int MAX_DEPTH = 256;  // nested groups: the parser and the NFA builder recurse per level
constexpr size_t MAX_NFA = (size_t)1 << 22;

struct Parser {
    const unsigned char* p;
    std::vector<Node> nodes;
    bool bad = false;
    int depth = 0;

    int add(Node n) { nodes.push_back(std::move(n)); return (int)nodes.size() - 1; }
    static int hex(unsigned char c) {
        if (c >= '0' && c <= '9') return c - '0';
        if (c >= 'a' && c <= 'f') return c - 'a' + 10;
        if (c >= 'A' && c <= 'F') return c - 'A' + 10;
        return -1;
    }
    static ByteSet range(int a, int b) {
        ByteSet s;
        for (int c = a; c <= b; c++) s.set((size_t)c);
        return s;
    }
    // after the backslash: a class (\d \w \s) or one byte
    bool escape(ByteSet& out, int& single) {
        const unsigned char c = *p;
        single = -1;
        if (!c) return false;
        p++;
        switch (c) {
            case 'd': out = range('0', '9'); return true;
            case 'w': out = range('0', '9') | range('a', 'z') | range('A', 'Z'); out.set('_'); return true;
            case 's': out.reset(); for (char w : {' ', '\t', '\n', '\r', '\f', '\v'}) out.set((unsigned char)w); return true;
            case 'n': single = '\n'; break;
            case 't': single = '\t'; break;
            case 'r': single = '\r'; break;
            case 'x': {
                const int h = hex(p[0]), l = h < 0 ? -1 : hex(p[1]);
                if (l < 0) return false;
                single = h * 16 + l;
                p += 2;
                break;
            }
            default:
                // an escaped metacharacter or punctuation stands for itself; other letters and digits
                // (back-references, \b, \D ...) are not part of the syntax
                if ((c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z')) return false;
                single = c;
        }
        out.reset();
        out.set((size_t)single);
        return true;
    }
    bool char_class(ByteSet& out) {  // after '['
        bool neg = false;
        if (*p == '^') { neg = true; p++; }
        out.reset();
        bool first = true;
        for (;;) {
            if (!*p) return false;
            if (*p == ']' && !first) { p++; break; }
            first = false;
            ByteSet item;
            int lo = -1;
            if (*p == '\\') {
                p++;
                if (!escape(item, lo)) return false;
            } else {
                lo = *p++;
                item.set((size_t)lo);
            }
            if (lo >= 0 && p[0] == '-' && p[1] && p[1] != ']') {
                p++;
                int hi = -1;
                if (*p == '\\') {
                    ByteSet e;
                    p++;
                    if (!escape(e, hi) || hi < 0) return false;
                } else {
                    hi = *p++;
                }
                if (hi < lo) return false;
                item = range(lo, hi);
            }
            out |= item;
        }
        if (neg) out = ~out;
        return true;
    }
    // {m} {m,} {m,n} after '{'
    bool counts(int& lo, int& hi) {
        const auto number = [&](int& v) {
            if (!(*p >= '0' && *p <= '9')) return false;
            v = 0;
            while (*p >= '0' && *p <= '9') {
                v = v * 10 + (*p++ - '0');
                if (v > MAX_COUNT) return false;
            }
            return true;
        };
        if (!number(lo)) return false;
        hi = lo;
        if (*p == ',') {
            p++;
            if (*p == '}') hi = -1;
            else if (!number(hi) || hi < lo) return false;
        }
        if (*p != '}') return false;
        p++;
        return true;
    }
    int atom() {
        const unsigned char c = *p;
        Node n;
        if (c == '(') {
            p++;
            if (++depth > MAX_DEPTH) { bad = true; return -1; }
            const int r = alt();
            depth--;
            if (bad || *p != ')') { bad = true; return -1; }
            p++;
            return r;
        }
        if (c == '[') {
            p++;
            if (!char_class(n.set)) { bad = true; return -1; }
        } else if (c == '.') {
            p++;
            n.set.set();
            n.set.reset('\n');
        } else if (c == '\\') {
            p++;
            int single;
            if (!escape(n.set, single)) { bad = true; return -1; }
        } else if (c == '*' || c == '+' || c == '?' || c == '{') {
            bad = true;  // nothing to repeat; a literal brace is escaped
            return -1;
        } else {
            p++;
            n.set.set(c);
        }
        return add(n);
    }
    int repeat() {
        int a = atom();
        if (bad) return -1;
        const unsigned char c = *p;
        if (c == '*' || c == '+' || c == '?' || c == '{') {
            Node n;
            n.kind = Node::REP;
            n.kids = {a};
            p++;
            if (c == '*') { n.lo = 0; n.hi = -1; }
            else if (c == '+') { n.lo = 1; n.hi = -1; }
            else if (c == '?') { n.lo = 0; n.hi = 1; }
            else if (!counts(n.lo, n.hi)) { bad = true; return -1; }
            a = add(n);
            // a second quantifier (lazy, possessive, stacked) is outside the syntax
            if (*p == '*' || *p == '+' || *p == '?' || *p == '{') { bad = true; return -1; }
        }
        return a;
    }
    int cat() {
        Node n;
        n.kind = Node::CAT;
        while (*p && *p != '|' && *p != ')') {
            const int k = repeat();
            if (bad) return -1;
            n.kids.push_back(k);
        }
        return add(n);
    }
    int alt() {
        Node n;
        n.kind = Node::ALT;
        for (;;) {
            const int k = cat();
            if (bad) return -1;
            n.kids.push_back(k);
            if (*p != '|') break;
            p++;
        }
        return n.kids.size() == 1 ? n.kids[0] : add(n);
    }
};

// ---- Thompson NFA --------------------------------------------------------------------------------
struct NState {
    int set = -1;              // index into Nfa::sets, -1 = no byte edge
    int out = -1;              // target of the byte edge
    int eps[2] = {-1, -1};
};
struct Nfa {
    std::vector<NState> st;
    std::vector<ByteSet> sets;
    bool overflow = false;
    int fresh() {
        if (st.size() >= MAX_NFA) { overflow = true; return 0; }
        st.emplace_back();
        return (int)st.size() - 1;
    }
    void eps(int from, int to) {
        NState& s = st[(size_t)from];
        (s.eps[0] < 0 ? s.eps[0] : s.eps[1]) = to;
    }
};
struct Frag { int in, out; };  // `out` has no edges yet

Frag build(Nfa& nfa, const std::vector<Node>& nodes, const int id, const std::vector<int>& set_of) {
    const Node& n = nodes[(size_t)id];
    if (nfa.overflow) return {0, 0};
    switch (n.kind) {
        case Node::SET: {
            const int a = nfa.fresh(), b = nfa.fresh();
            nfa.st[(size_t)a].set = set_of[(size_t)id];
            nfa.st[(size_t)a].out = b;
            return {a, b};
        }
        case Node::CAT: {
            const int a = nfa.fresh();
            int cur = a;
            for (int k : n.kids) {
                const Frag f = build(nfa, nodes, k, set_of);
                nfa.eps(cur, f.in);
                cur = f.out;
            }
            return {a, cur};
        }
        case Node::ALT: {
            // a chain of two-way forks, one per alternative
            const int b = nfa.fresh();
            int fork = nfa.fresh();
            const int a = fork;
            for (size_t i = 0; i < n.kids.size(); i++) {
                const Frag f = build(nfa, nodes, n.kids[i], set_of);
                nfa.eps(fork, f.in);
                nfa.eps(f.out, b);
                if (i + 1 < n.kids.size()) {
                    const int nf = nfa.fresh();
                    nfa.eps(fork, nf);
                    fork = nf;
                }
            }
            return {a, b};
        }
        case Node::REP: {
            const int a = nfa.fresh();
            int cur = a;
            for (int i = 0; i < n.lo; i++) {
                const Frag f = build(nfa, nodes, n.kids[0], set_of);
                nfa.eps(cur, f.in);
                cur = f.out;
            }
            if (n.hi < 0) {  // x*: loop -> x -> loop, loop -> end
                const int loop = nfa.fresh(), end = nfa.fresh();
                nfa.eps(cur, loop);
                const Frag f = build(nfa, nodes, n.kids[0], set_of);
                nfa.eps(loop, f.in);
                nfa.eps(loop, end);
                nfa.eps(f.out, loop);
                return {a, end};
            }
            const int end = nfa.fresh();
            for (int i = n.lo; i < n.hi; i++) {  // (x(x(x)?)?)?
                const int opt = nfa.fresh();
                nfa.eps(cur, opt);
                const Frag f = build(nfa, nodes, n.kids[0], set_of);
                nfa.eps(opt, f.in);
                nfa.eps(opt, end);
                cur = f.out;
            }
            nfa.eps(cur, end);
            return {a, end};
        }
    }
    return {0, 0};
}

void closure(const Nfa& nfa, std::vector<int>& set, std::vector<char>& mark) {
    std::vector<int> stack(set);
    for (int s : set) mark[(size_t)s] = 1;
    while (!stack.empty()) {
        const int s = stack.back();
        stack.pop_back();
        for (int e : nfa.st[(size_t)s].eps)
            if (e >= 0 && !mark[(size_t)e]) {
                mark[(size_t)e] = 1;
                set.push_back(e);
                stack.push_back(e);
            }
    }
    for (int s : set) mark[(size_t)s] = 0;
    std::sort(set.begin(), set.end());
}

}  // namespace
}  // namespace xalm

using namespace xalm;

extern "C" {

int xh_regex_compile(const char* pattern, uint16_t* next, uint8_t* accept, int cap_states, int* n_states, int* start) {
    if (!pattern || !n_states || !start || cap_states < 0 || (cap_states > 0 && (!next || !accept))) return XH_E_INVALID;
    *n_states = 0;
    *start = 0;
    Parser ps;
    ps.p = (const unsigned char*)pattern;
    const int root = ps.alt();
    if (ps.bad || *ps.p) return XH_E_INVALID;  // a stray ')' ends alt() early

    Nfa nfa;
    std::vector<int> set_of(ps.nodes.size(), -1);
    for (size_t i = 0; i < ps.nodes.size(); i++)
        if (ps.nodes[i].kind == Node::SET) {
            set_of[i] = (int)nfa.sets.size();
            nfa.sets.push_back(ps.nodes[i].set);
        }
    const Frag f = build(nfa, ps.nodes, root, set_of);
    if (nfa.overflow) return XH_E_INVALID;
    const int final_state = f.out;

    // subset construction; only the states with a byte edge (and the final one) tell subsets apart
    std::vector<char> mark(nfa.st.size(), 0);
    std::map<std::vector<int>, int> ids;
    std::vector<std::vector<int>> subsets;
    std::vector<std::array<int, 256>> trans;
    const auto intern = [&](std::vector<int>& raw) {
        closure(nfa, raw, mark);
        std::vector<int> core;
        for (int s : raw)
            if (nfa.st[(size_t)s].set >= 0 || s == final_state) core.push_back(s);
        if (core.empty()) return -1;
        const auto it = ids.find(core);
        if (it != ids.end()) return it->second;
        const int id = (int)subsets.size();
        ids.emplace(core, id);
        subsets.push_back(std::move(core));
        return id;
    };
    std::vector<int> s0{f.in};
    if (intern(s0) < 0) return XH_E_INVALID;  // the start closure reaches neither a byte edge nor the end
    for (size_t d = 0; d < subsets.size(); d++) {
        if (subsets.size() > (size_t)XH_DFA_MAX_STATES) return XH_E_INVALID;
        std::array<int, 256> row;
        row.fill(-1);
        const std::vector<int> cur = subsets[d];
        ByteSet any;
        for (int s : cur)
            if (nfa.st[(size_t)s].set >= 0) any |= nfa.sets[(size_t)nfa.st[(size_t)s].set];
        // bytes that select the same edges share the successor: remember it per edge selection
        std::map<std::vector<int>, int> by_targets;
        for (int b = 0; b < 256; b++) {
            if (!any[(size_t)b]) continue;
            std::vector<int> tg;
            for (int s : cur) {
                const NState& ns = nfa.st[(size_t)s];
                if (ns.set >= 0 && nfa.sets[(size_t)ns.set][(size_t)b]) tg.push_back(ns.out);
            }
            std::sort(tg.begin(), tg.end());
            tg.erase(std::unique(tg.begin(), tg.end()), tg.end());
            const auto it = by_targets.find(tg);
            if (it != by_targets.end()) { row[(size_t)b] = it->second; continue; }
            std::vector<int> raw(tg);
            const int id = intern(raw);
            by_targets.emplace(std::move(tg), id);
            row[(size_t)b] = id;
        }
        trans.push_back(row);
    }
    const int nd = (int)subsets.size();
    if (nd > XH_DFA_MAX_STATES) return XH_E_INVALID;

    // trim: keep the states from which an accepting state is reachable (backward search)
    std::vector<char> acc((size_t)nd, 0), live((size_t)nd, 0);
    std::vector<std::vector<int>> pred((size_t)nd);
    for (int d = 0; d < nd; d++) {
        acc[(size_t)d] = std::binary_search(subsets[(size_t)d].begin(), subsets[(size_t)d].end(), final_state);
        for (int b = 0; b < 256; b++)
            if (trans[(size_t)d][(size_t)b] >= 0) pred[(size_t)trans[(size_t)d][(size_t)b]].push_back(d);
    }
    std::vector<int> stack;
    for (int d = 0; d < nd; d++)
        if (acc[(size_t)d]) { live[(size_t)d] = 1; stack.push_back(d); }
    while (!stack.empty()) {
        const int d = stack.back();
        stack.pop_back();
        for (int q : pred[(size_t)d])
            if (!live[(size_t)q]) { live[(size_t)q] = 1; stack.push_back(q); }
    }
    if (!live[0]) return XH_E_INVALID;  // the empty language
    std::vector<int> renum((size_t)nd, -1);
    int n_live = 0;
    for (int d = 0; d < nd; d++)
        if (live[(size_t)d]) renum[(size_t)d] = n_live++;
    *n_states = n_live;
    *start = renum[0];
    if (n_live > cap_states) return XH_E_NOMEM;
    for (int d = 0; d < nd; d++) {
        if (!live[(size_t)d]) continue;
        const int r = renum[(size_t)d];
        accept[r] = acc[(size_t)d] ? 1 : 0;
        for (int b = 0; b < 256; b++) {
            const int t = trans[(size_t)d][(size_t)b];
            next[(size_t)r * 256 + (size_t)b] = t >= 0 && live[(size_t)t] ? (uint16_t)renum[(size_t)t] : (uint16_t)XH_DFA_DEAD;
        }
    }
    return XH_OK;
}

int xh_constraint_mask(const xh_byte_dfa* dfa, const uint8_t* bytes, const uint32_t* offsets, int vocab, uint32_t state,
                       int stop_token_a, int stop_token_b, uint8_t* allowed_out, uint16_t* next_state_out) {
    if (dfa_error(dfa) || pieces_error(bytes, offsets, vocab) || dfa_state_error(dfa, state) || !allowed_out ||
        !next_state_out)
        return XH_E_INVALID;
    const bool stuck = state == XH_DFA_DEAD;
    for (int t = 0; t < vocab; t++) {
        uint32_t to = XH_DFA_DEAD;
        if (!stuck) {
            if (t == stop_token_a || t == stop_token_b) to = dfa->accept[state] ? state : (uint32_t)XH_DFA_DEAD;
            else to = dfa_walk(dfa->next, state, bytes + offsets[t], offsets[t + 1] - offsets[t]);
        }
        allowed_out[t] = to != XH_DFA_DEAD;
        next_state_out[t] = (uint16_t)to;
    }
    return XH_OK;
}

}  // extern "C"
