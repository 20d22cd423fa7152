// constraint_check.cpp — the regex compiler and xh_constraint_mask in a stand-alone host program,
// for a sanitizer build (no HIP, no device):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o constraint_check tools/constraint_check.cpp xalm_amd/csrc/constraint.cpp && ./constraint_check
// It compiles valid, invalid and large patterns (with exact, too small and zero capacities), checks
// a few matches by walking the tables, and runs the mask over pieces that include an empty one, a
// 300-byte one and end tokens, from a live state and from XH_DFA_DEAD.  Exit status 0 = all held.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/xalm_hip.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

struct Dfa {
    std::vector<uint16_t> next;
    std::vector<uint8_t> accept;
    int n = 0, start = 0, rc = 0;
    xh_byte_dfa abi() const { return {n, start, next.data(), accept.data()}; }
    bool match(const std::string& s) const {
        uint32_t st = (uint32_t)start;
        for (unsigned char b : s) {
            st = next[(size_t)st * 256 + b];
            if (st == XH_DFA_DEAD) return false;
        }
        return accept[st] != 0;
    }
};

static Dfa compile(const char* pattern) {
    Dfa d;
    d.rc = xh_regex_compile(pattern, nullptr, nullptr, 0, &d.n, &d.start);
    if (d.rc != XH_E_NOMEM) return d;
    if (d.n > 1) {  // one state short: refused again, nothing written past the cap
        std::vector<uint16_t> small((size_t)(d.n - 1) * 256);
        std::vector<uint8_t> acc((size_t)d.n - 1);
        int n2 = 0, s2 = 0;
        CHECK(xh_regex_compile(pattern, small.data(), acc.data(), d.n - 1, &n2, &s2) == XH_E_NOMEM && n2 == d.n);
    }
    d.next.resize((size_t)d.n * 256);
    d.accept.resize((size_t)d.n);
    d.rc = xh_regex_compile(pattern, d.next.data(), d.accept.data(), d.n, &d.n, &d.start);
    return d;
}

int main() {
    const Dfa num = compile("\\d+(\\.\\d+)?");
    CHECK(num.rc == XH_OK && num.n == 4);
    CHECK(num.match("12.5") && num.match("7") && !num.match("7.") && !num.match(""));
    const Dfa cls = compile("[^a-c\\d]{2,3}|\\x41+|(ab|a)*\\s");
    CHECK(cls.rc == XH_OK && cls.match("xyz") && cls.match("AAA") && cls.match("aba ") && !cls.match("a1"));
    const Dfa big = compile("(a{200}){200}");
    CHECK(big.rc == XH_OK && big.n == 40001 && big.match(std::string(40000, 'a')) && !big.match(std::string(39999, 'a')));
    for (const char* bad : {"a**", "(", "a)", "[a", "[", "a{2", "a{3,2}", "a{257}", "*", "\\", "\\x4", "\\q", "a{",
                            "a[^\\x00-\\xff]", "(a{256}){256}b", "[a-", "[z-a]", "(|", "a|*"})
        CHECK(compile(bad).rc == XH_E_INVALID);
    // nesting: 256 groups deep compiles, deeper is refused before the recursion can exhaust the stack
    CHECK(compile((std::string(256, '(') + "a" + std::string(256, ')')).c_str()).rc == XH_OK);
    CHECK(compile((std::string(300000, '(') + "a" + std::string(300000, ')')).c_str()).rc == XH_E_INVALID);
    int n = 0, s = 0;
    CHECK(xh_regex_compile(nullptr, nullptr, nullptr, 0, &n, &s) == XH_E_INVALID);

    // the mask: pieces with an empty one, a long one, bytes above 127 and two end tokens
    std::vector<std::string> pieces = {"zz", "1", "12", ".", "", "</s>", std::string(300, '7'), "1.5", "\xc3\xa9", "7."};
    std::vector<uint8_t> blob;
    std::vector<uint32_t> offsets{0};
    for (const std::string& p : pieces) {
        blob.insert(blob.end(), p.begin(), p.end());
        offsets.push_back((uint32_t)blob.size());
    }
    const int V = (int)pieces.size();
    std::vector<uint8_t> allowed((size_t)V);
    std::vector<uint16_t> succ((size_t)V);
    const xh_byte_dfa d = num.abi();
    CHECK(xh_constraint_mask(&d, blob.data(), offsets.data(), V, (uint32_t)num.start, 5, -1, allowed.data(), succ.data()) == XH_OK);
    CHECK(!allowed[0] && allowed[1] && allowed[2] && !allowed[3] && !allowed[4] && !allowed[5] && allowed[6] && allowed[7] &&
          !allowed[8] && allowed[9]);
    CHECK(xh_constraint_mask(&d, blob.data(), offsets.data(), V, succ[1], -1, 5, allowed.data(), succ.data()) == XH_OK);
    CHECK(allowed[5] && allowed[3] && !allowed[4]);  // after a digit the text may end, or go on with "."
    CHECK(xh_constraint_mask(&d, blob.data(), offsets.data(), V, XH_DFA_DEAD, 5, -1, allowed.data(), succ.data()) == XH_OK);
    for (int t = 0; t < V; t++) CHECK(!allowed[t] && succ[t] == XH_DFA_DEAD);
    CHECK(xh_constraint_mask(&d, blob.data(), offsets.data(), V, 4, 5, -1, allowed.data(), succ.data()) == XH_E_INVALID);
    offsets[3] = offsets[2] - 1;
    CHECK(xh_constraint_mask(&d, blob.data(), offsets.data(), V, 0, 5, -1, allowed.data(), succ.data()) == XH_E_INVALID);
    printf(failures ? "%d check(s) failed\n" : "constraint_check: all held\n", failures);
    return failures ? 1 : 0;
}
