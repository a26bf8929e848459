// search_check.cpp -- the host build of `gffx search`'s regex compiler (gffx_amd/csrc/host/regex_dfa.cpp) and of
// device/search_core.hpp (the DFA match loop, the pair set and the line test that the kernels of device/search.hip run) under
// AddressSanitizer + UndefinedBehaviorSanitizer (`make -C gffx_amd/csrc search_check`), driven by tests/test_search_cpu.py.
// Every value and every line the core reads is a heap allocation of exactly its size, so a read past it is reported.
//   search_check syntax                      the parser's accept / reject table below: one case per rejected construct, with the
//                                            byte offset the message must name.  "ok <cases>", or the first difference and exit 1
//   search_check dfa PATTERNS VALUES [CAP]   one pattern / one value per line.  Per pattern a line of '0' / '1', one per value:
//                                            the DFA's answer -- after it has been compared with the direct NFA simulation
//                                            (a difference ends the run with exit 1); "-" for a pattern that does not compile
//   search_check union PATTERNS VALUES CAP   all patterns as one list under the cap: "groups <first>:<n>:<states> ...", then
//                                            one line of '0' / '1' per value (DFA groups ORed, compared with the NFA of the list)
//   search_check filter TEXT VALUES KEY MATCHED [-T TYPES]
//                                            the lines of TEXT (cut behind every '\n'; a non-empty rest is the last line) as
//                                            lines of the block of root 5, VALUES the `.atn` strings (aid = line number),
//                                            MATCHED the strings whose class forms a pair with root 5: per line "1" or "0"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "../gffx_amd/csrc/device/search_core.hpp"
#include "../gffx_amd/csrc/host/regex_dfa.hpp"
#include "../gffx_amd/csrc/host/text.hpp"

using namespace gffx;

namespace {
std::vector<uint8_t> read_file(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        std::exit(2);
    }
    static uint8_t buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

std::unique_ptr<uint8_t[]> exact(const void *p, size_t n) {
    std::unique_ptr<uint8_t[]> c(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(c.get(), p, n);
    return c;
}

std::vector<std::string> lines_of(const std::vector<uint8_t> &v, bool keep_nl = false) {
    std::vector<std::string> out;
    size_t a = 0;
    for (size_t i = 0; i < v.size(); ++i)
        if (v[i] == '\n') {
            out.emplace_back(reinterpret_cast<const char *>(v.data() + a), i - a + (keep_nl ? 1 : 0));
            a = i + 1;
        }
    if (a < v.size()) out.emplace_back(reinterpret_cast<const char *>(v.data() + a), v.size() - a);
    return out;
}

// the pair set built in order, with the device's hash and probing
void pair_insert_host(std::vector<ids::u64> *slot, uint32_t cls, uint32_t root) {
    const uint32_t mask = (uint32_t)slot->size() - 1;
    const ids::u64 w = search::pair_word(cls, root);
    for (uint32_t i = search::pair_hash(w) & mask;; i = (i + 1) & mask) {
        if ((*slot)[i] == w) return;
        if ((*slot)[i] == ids::kEmptyWord) {
            (*slot)[i] = w;
            return;
        }
    }
}

bool dfa_on_exact_copy(const regex::Compiled &c, const std::string &value) {
    const auto copy = exact(value.data(), value.size());
    for (const regex::Dfa &g : c.groups) {
        const search::Dfa d{g.cls, g.trans.data(), g.n_states, g.n_classes, g.init};
        if (search::dfa_match(d, copy.get(), value.size())) return true;
    }
    return false;
}

struct SyntaxCase {
    const char *pattern;
    long at;  // -1: accepted
    const char *what;
};
const std::string kDeep = std::string(101, '(') + "a" + std::string(101, ')'), kDeepOk = std::string(100, '(') + "a" + std::string(100, ')');
const SyntaxCase kSyntax[] = {
    {"TP53", -1, ""}, {"", -1, ""}, {"a|", -1, ""}, {"|", -1, ""}, {"(|a)", -1, ""}, {"(?:ab)+", -1, ""}, {"^a$", -1, ""},
    {"a{2}", -1, ""}, {"a{2,}", -1, ""}, {"a{2,5}?", -1, ""}, {"a{0,255}", -1, ""}, {"a*?b+?c??", -1, ""}, {"[]a]", -1, ""},
    {"[^]a]", -1, ""}, {"[a-]", -1, ""}, {"[-a]", -1, ""}, {"[a^]", -1, ""}, {"[a-c0-9_]", -1, ""}, {"[\\]\\-\\\\]", -1, ""},
    {"\\\\\\.\\+\\*\\?\\(\\)\\|\\[\\]\\{\\}\\^\\$\\-", -1, ""}, {"\xC3\xA9+", -1, ""}, {"a]b}c", -1, ""}, {".", -1, ""}, {"(^)*", -1, ""},
    {"\\d", 0, "the escape '\\d'"}, {"a\\w", 1, "the escape '\\w'"}, {"\\s", 0, "the escape '\\s'"}, {"x\\bx", 1, "the escape '\\b'"},
    {"\\n", 0, "the escape '\\n'"}, {"a\\", 1, "a '\\' at the end"}, {"\\\xC3\xA9", 0, "the escape"},
    {"(?i)a", 0, "inline flag"}, {"a(?P<n>b)", 1, "named group"}, {"(?=a)", 0, "inline flag"},
    {"[\xC3\xA9]", 1, "non-ASCII member"}, {"[a-\xC3\xA9]", 3, "non-ASCII member"}, {"[a[b]]", 2, "unescaped '['"}, {"[[:alpha:]]", 1, "unescaped '['"},
    {"[a&&b]", 2, "'&&'"}, {"[a--b]", 2, "'--'"}, {"[a~~b]", 2, "'~~'"}, {"[z-a]", 1, "runs backwards"}, {"[abc", 0, "unclosed '['"},
    {"[]", 0, "unclosed '['"}, {"[a-\\d]", 3, "the escape '\\d'"},
    {"a{", 1, "malformed '{'"}, {"a{x}", 1, "malformed '{'"}, {"a{,3}", 1, "malformed '{'"}, {"a{2,1}", 1, "malformed '{'"},
    {"a{2", 1, "malformed '{'"}, {"a{2,3", 1, "malformed '{'"}, {"a{256}", 1, "above 255"}, {"a{1,256}", 1, "above 255"},
    {"a**", 2, "directly after a quantifier"}, {"a+*", 2, "directly after a quantifier"}, {"a?{2}", 2, "directly after a quantifier"},
    {"a{2}{3}", 4, "directly after a quantifier"}, {"a*?+", 3, "directly after a quantifier"},
    {"^*", 1, "after an anchor"}, {"a$+", 2, "after an anchor"}, {"^{2}", 1, "after an anchor"},
    {"*a", 0, "nothing before it"}, {"a|+", 2, "nothing before it"}, {"(?:?)", 3, "nothing before it"}, {"{2}", 0, "nothing before it"},
    {"(*)", 1, "nothing before it"},
    {"(a", 0, "unclosed '('"}, {kDeep.c_str(), 100, "nested more than 100 deep"}, {kDeepOk.c_str(), -1, ""}, {"a)", 1, "unmatched ')'"}, {"\xff", 0, "not valid UTF-8"},
};

int run_syntax() {
    int n = 0;
    for (const SyntaxCase &c : kSyntax) {
        const std::string msg = regex::check_syntax(c.pattern);
        ++n;
        if (c.at < 0) {
            if (!msg.empty()) {
                std::printf("case %d: \"%s\" should be accepted, got: %s\n", n, c.pattern, msg.c_str());
                return 1;
            }
            continue;
        }
        const std::string head = "unsupported regex syntax at byte " + std::to_string(c.at) + " of \"" + c.pattern + "\": ";
        if (msg.compare(0, head.size(), head) != 0 || msg.find(c.what) == std::string::npos) {
            std::printf("case %d: \"%s\" should be refused at byte %ld (%s), got: %s\n", n, c.pattern, c.at, c.what, msg.c_str());
            return 1;
        }
        // ... and compile() refuses it with the same text
        try {
            (void)regex::compile({c.pattern});
            std::printf("case %d: compile() took \"%s\"\n", n, c.pattern);
            return 1;
        } catch (const Error &e) {
            if (msg != e.what()) {
                std::printf("case %d: compile() says: %s\n", n, e.what());
                return 1;
            }
        }
    }
    std::printf("ok %d\n", n);
    return 0;
}

int run_dfa(int argc, char **argv) {
    const std::vector<std::string> patterns = lines_of(read_file(argv[2])), values = lines_of(read_file(argv[3]));
    const uint32_t cap = argc > 4 ? (uint32_t)std::atoi(argv[4]) : 0;
    for (const std::string &p : patterns) {
        regex::Compiled c;
        try {
            c = regex::compile({p}, cap);
        } catch (const Error &) {
            std::printf("-\n");
            continue;
        }
        std::string row;
        for (const std::string &v : values) {
            const bool d = dfa_on_exact_copy(c, v), n = regex::nfa_match({p}, v);
            if (d != n) {
                std::printf("DFA %d, NFA %d: pattern \"%s\", value \"%s\"\n", d, n, p.c_str(), v.c_str());
                return 1;
            }
            row += d ? '1' : '0';
        }
        std::printf("%s\n", row.c_str());
    }
    return 0;
}

int run_union(char **argv) {
    const std::vector<std::string> patterns = lines_of(read_file(argv[2])), values = lines_of(read_file(argv[3]));
    regex::Compiled c;
    try {
        c = regex::compile(patterns, (uint32_t)std::atoi(argv[4]));
    } catch (const Error &e) {
        std::printf("error %s\n", e.what());
        return 0;
    }
    std::printf("groups");
    uint32_t next = 0;
    for (const regex::Dfa &g : c.groups) {
        if (g.first_pattern != next || g.n_states > c.max_states) {
            std::printf("\ngroup at %u, expected %u; %u states under a cap of %u\n", g.first_pattern, next, g.n_states, c.max_states);
            return 1;
        }
        next += g.n_patterns;
        std::printf(" %u:%u:%u", g.first_pattern, g.n_patterns, g.n_states);
    }
    std::printf("\n");
    if (next != patterns.size()) return 1;
    for (const std::string &v : values) {
        const bool d = dfa_on_exact_copy(c, v), n = regex::nfa_match(patterns, v);
        if (d != n) {
            std::printf("DFA %d, NFA %d on value \"%s\"\n", d, n, v.c_str());
            return 1;
        }
        std::printf("%c\n", d ? '1' : '0');
    }
    return 0;
}

int run_filter(int argc, char **argv) {
    const std::vector<std::string> lines = lines_of(read_file(argv[2]), true), values = lines_of(read_file(argv[3]));
    const std::string key = argv[4];
    const std::vector<std::string> matched = lines_of(read_file(argv[5]));
    std::optional<std::string> types_arg;
    if (argc > 7 && std::string(argv[6]) == "-T") types_arg = argv[7];
    std::string bytes;
    std::vector<ids::u64> off{0};
    for (const std::string &v : values) {
        bytes += v;
        off.push_back(bytes.size());
    }
    const auto vb = exact(bytes.data(), bytes.size());
    std::vector<ids::u64> slot;
    std::vector<uint32_t> val;
    ids::table_build_host(values.size(), vb.get(), off.data(), -1, &slot, &val);
    const ids::Table t{slot.data(), val.data(), vb.get(), off.data(), (uint32_t)slot.size() - 1, 0xFFFFFFFFu};
    const uint32_t root = 5;
    std::vector<ids::u64> pairs(ids::table_slots(matched.size() + 1), ids::kEmptyWord);
    for (const std::string &m : matched) {
        const auto mc = exact(m.data(), m.size());
        const uint32_t c = ids::table_find(t, mc.get(), m.size());
        if (c != ids::kNone) pair_insert_host(&pairs, c, root);
    }
    pair_insert_host(&pairs, 0, root + 1);  // (a pair of another root)
    std::string type_bytes;
    std::vector<uint32_t> type_off{0};
    for (const std::string &s : split_types(types_arg)) {
        type_bytes += s;
        type_off.push_back((uint32_t)type_bytes.size());
    }
    const auto tb = exact(type_bytes.data(), type_bytes.size());
    const ids::Types types{tb.get(), type_off.data(), (uint32_t)type_off.size() - 1, types_arg ? 1 : 0};
    const auto kb = exact(key.data(), key.size());
    for (const std::string &l : lines) {
        const auto lc = exact(l.data(), l.size());
        const bool k = search::keep_line_value(t, pairs.data(), (uint32_t)pairs.size() - 1, types, kb.get(), (uint32_t)key.size(), lc.get(), l.size(), root);
        std::printf("%d\n", k ? 1 : 0);
    }
    return 0;
}
}  // namespace

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "syntax") return run_syntax();
    if (mode == "dfa" && argc >= 4) return run_dfa(argc, argv);
    if (mode == "union" && argc >= 5) return run_union(argv);
    if (mode == "filter" && argc >= 6) return run_filter(argc, argv);
    std::fprintf(stderr, "usage: search_check syntax | dfa PATTERNS VALUES [CAP] | union PATTERNS VALUES CAP | filter TEXT VALUES KEY MATCHED [-T TYPES]\n");
    return 2;
}
