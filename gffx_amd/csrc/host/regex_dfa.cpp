// regex_dfa.cpp -- see regex_dfa.hpp: the parser of the subset, the Thompson construction over bytes, the subset
// construction with the state cap and the grouping of a pattern list.
#include "regex_dfa.hpp"

#include <algorithm>
#include <cstdlib>
#include <map>
#include <memory>

#include "../device/search_core.hpp"
#include "text.hpp"

namespace gffx::regex {

namespace {

// ---- the syntax tree ------------------------------------------------------------------------------------------------------
struct Node {
    enum Kind { Empty, Bytes, Set, Cat, Alt, Repeat, Start, End } kind = Empty;
    std::string bytes;          // Bytes: one scalar's UTF-8 sequence
    bool ascii[128] = {};       // Set
    bool non_ascii = false;     // Set: every non-ASCII scalar too
    std::vector<std::unique_ptr<Node>> kids;
    int min = 0, max = 0;       // Repeat; max < 0: no upper bound
};
using NodeP = std::unique_ptr<Node>;

struct SyntaxError {
    size_t at;
    std::string what;
};

constexpr int kMaxCount = 255;
constexpr size_t kMaxNfaStates = 200000;
constexpr int kMaxDepth = 100;  // nested groups: the parser recurses once per level

struct Parser {
    const std::string &s;
    size_t pos = 0;
    int depth = 0;
    explicit Parser(const std::string &p) : s(p) {}

    [[noreturn]] void bad(size_t at, const std::string &what) const { throw SyntaxError{at, what}; }
    bool more() const { return pos < s.size(); }
    static bool is_escapable(char c) { return std::string_view("\\.+*?()|[]{}^$-").find(c) != std::string_view::npos; }

    NodeP parse() {
        NodeP n = alt();
        if (more()) bad(pos, "unmatched ')'");  // alt() only stops at ')' or at the end
        return n;
    }

    NodeP alt() {
        auto n = std::make_unique<Node>();
        n->kind = Node::Alt;
        n->kids.push_back(cat());
        while (more() && s[pos] == '|') {
            ++pos;
            n->kids.push_back(cat());
        }
        if (n->kids.size() == 1) return std::move(n->kids[0]);
        return n;
    }

    NodeP cat() {
        auto n = std::make_unique<Node>();
        n->kind = Node::Cat;
        while (more() && s[pos] != '|' && s[pos] != ')') n->kids.push_back(repeat());
        if (n->kids.empty()) n->kind = Node::Empty;
        return n;
    }

    static bool quantifier_at(char c) { return c == '*' || c == '+' || c == '?' || c == '{'; }

    NodeP repeat() {
        NodeP a = atom();
        if (!more() || !quantifier_at(s[pos])) return a;
        if (a->kind == Node::Start || a->kind == Node::End) bad(pos, "a quantifier after an anchor");
        const size_t q_at = pos;
        int lo = 0, hi = -1;
        const char q = s[pos];
        if (q == '*') {
            ++pos;
        } else if (q == '+') {
            lo = 1;
            ++pos;
        } else if (q == '?') {
            hi = 1;
            ++pos;
        } else {
            counted(q_at, &lo, &hi);
        }
        if (more() && s[pos] == '?') ++pos;  // the lazy form: the same set of matching texts
        if (more() && quantifier_at(s[pos])) bad(pos, "a quantifier directly after a quantifier");
        auto r = std::make_unique<Node>();
        r->kind = Node::Repeat;
        r->min = lo;
        r->max = hi;
        r->kids.push_back(std::move(a));
        return r;
    }

    // {m} {m,} {m,n}
    void counted(size_t at, int *lo, int *hi) {
        ++pos;  // '{'
        auto number = [&](int *v) {
            const size_t from = pos;
            long x = 0;
            while (more() && s[pos] >= '0' && s[pos] <= '9') {
                x = std::min<long>(x * 10 + (s[pos] - '0'), 1000000);
                ++pos;
            }
            if (pos == from) return false;
            if (x > kMaxCount) bad(at, "a repetition count above 255");
            *v = (int)x;
            return true;
        };
        if (!number(lo)) bad(at, "a malformed '{' (expected {m}, {m,} or {m,n})");
        if (more() && s[pos] == '}') {
            ++pos;
            *hi = *lo;
            return;
        }
        if (!more() || s[pos] != ',') bad(at, "a malformed '{' (expected {m}, {m,} or {m,n})");
        ++pos;
        if (more() && s[pos] == '}') {
            ++pos;
            *hi = -1;
            return;
        }
        if (!number(hi) || !more() || s[pos] != '}') bad(at, "a malformed '{' (expected {m}, {m,} or {m,n})");
        ++pos;
        if (*hi < *lo) bad(at, "a malformed '{' (n < m in {m,n})");
    }

    static size_t scalar_len(unsigned char c) { return c < 0x80 ? 1 : c < 0xE0 ? 2 : c < 0xF0 ? 3 : 4; }

    NodeP atom() {
        const size_t at = pos;
        const char c = s[pos];
        auto n = std::make_unique<Node>();
        switch (c) {
            case '(': {
                ++pos;
                if (more() && s[pos] == '?') {
                    if (pos + 1 < s.size() && s[pos + 1] == ':')
                        pos += 2;
                    else
                        bad(at, "an inline flag or a named group '(?...'");
                }
                if (++depth > kMaxDepth) bad(at, "groups nested more than " + std::to_string(kMaxDepth) + " deep");
                n = alt();
                --depth;
                if (!more() || s[pos] != ')') bad(at, "an unclosed '('");
                ++pos;
                return n;
            }
            case '[': return char_class();
            case '.':
                ++pos;
                n->kind = Node::Set;
                for (int b = 0; b < 128; ++b) n->ascii[b] = b != '\n';
                n->non_ascii = true;
                return n;
            case '^':
                ++pos;
                n->kind = Node::Start;
                return n;
            case '$':
                ++pos;
                n->kind = Node::End;
                return n;
            case '\\':
                n->kind = Node::Bytes;
                n->bytes = std::string(1, escape());
                return n;
            case '*':
            case '+':
            case '?':
            case '{': bad(at, "a quantifier with nothing before it");
            default: break;
        }
        const size_t len = scalar_len((unsigned char)c);  // (the pattern is valid UTF-8: checked before parsing)
        n->kind = Node::Bytes;
        n->bytes = s.substr(pos, len);
        pos += len;
        return n;
    }

    char escape() {  // at '\\'
        const size_t at = pos;
        if (pos + 1 >= s.size()) bad(at, "a '\\' at the end");
        const char e = s[pos + 1];
        if (!is_escapable(e)) {
            const size_t len = scalar_len((unsigned char)e);
            bad(at, "the escape '\\" + s.substr(pos + 1, len) + "' (only \\\\ \\. \\+ \\* \\? \\( \\) \\| \\[ \\] \\{ \\} \\^ \\$ \\- are taken)");
        }
        pos += 2;
        return e;
    }

    NodeP char_class() {
        const size_t at = pos;
        ++pos;  // '['
        auto n = std::make_unique<Node>();
        n->kind = Node::Set;
        bool negate = false;
        if (more() && s[pos] == '^') {
            negate = true;
            ++pos;
        }
        bool in[128] = {};
        bool first = true;
        while (true) {
            if (!more()) bad(at, "an unclosed '['");
            char c = s[pos];
            if (c == ']' && !first) {
                ++pos;
                break;
            }
            const size_t item_at = pos;
            if ((unsigned char)c >= 0x80) bad(item_at, "a non-ASCII member of a class");
            if (c == '[') bad(item_at, "an unescaped '[' inside a class");
            if (pos + 1 < s.size() && (c == '&' || c == '-' || c == '~') && s[pos + 1] == c)
                bad(item_at, std::string("'") + c + c + "' inside a class");
            char lo;
            if (c == '\\')
                lo = escape();
            else
                lo = c, ++pos;
            first = false;
            // a range lo-hi?  a '-' that is last in the class (before ']') is literal, as is a leading one (lo itself)
            if (more() && s[pos] == '-' && pos + 1 < s.size() && s[pos + 1] != ']') {
                if (s[pos + 1] == '-') bad(pos, "'--' inside a class");
                ++pos;  // '-'
                char h = s[pos];
                if ((unsigned char)h >= 0x80) bad(pos, "a non-ASCII member of a class");
                if (h == '[') bad(pos, "an unescaped '[' inside a class");
                if (h == '\\')
                    h = escape();
                else
                    ++pos;
                if ((unsigned char)h < (unsigned char)lo) bad(item_at, "a class range that runs backwards");
                for (int b = (unsigned char)lo; b <= (unsigned char)h; ++b) in[b] = true;
            } else {
                in[(unsigned char)lo] = true;
            }
        }
        for (int b = 0; b < 128; ++b) n->ascii[b] = negate ? !in[b] : in[b];
        n->non_ascii = negate;
        return n;
    }
};

NodeP parse_pattern(const std::string &p) {
    if (!utf8_valid(p)) throw SyntaxError{0, "a pattern that is not valid UTF-8"};
    Parser ps(p);
    return ps.parse();
}

std::string syntax_message(const std::string &pattern, const SyntaxError &e) {
    return "unsupported regex syntax at byte " + std::to_string(e.at) + " of \"" + pattern + "\": " + e.what;
}

// ---- Thompson NFA over bytes ------------------------------------------------------------------------------------------------
struct NState {
    enum Kind : uint8_t { Range, Split, AssertStart, AssertEnd, Match } kind;
    uint8_t lo = 0, hi = 0;
    int out = -1, out1 = -1;
};

struct Nfa {
    std::vector<NState> st;
    int start = -1;

    int add(NState s) {
        if (st.size() >= kMaxNfaStates) throw Error("regex too large: more than " + std::to_string(kMaxNfaStates) + " NFA states");
        st.push_back(s);
        return (int)st.size() - 1;
    }
    int range(int lo, int hi, int next) { return add(NState{NState::Range, (uint8_t)lo, (uint8_t)hi, next, -1}); }
    int split(int a, int b) { return add(NState{NState::Split, 0, 0, a, b}); }
    int any_of(const std::vector<int> &entries, int dead_next) {
        if (entries.empty()) return range(1, 0, dead_next);  // an empty class: a range no byte is in
        int e = entries.back();
        for (size_t i = entries.size() - 1; i-- > 0;) e = split(entries[i], e);
        return e;
    }
    int cont(int n, int next) {  // n continuation bytes
        for (int i = 0; i < n; ++i) next = range(0x80, 0xBF, next);
        return next;
    }
    void non_ascii_scalars(std::vector<int> *entries, int next) {  // the well-formed multi-byte sequences
        entries->push_back(range(0xC2, 0xDF, cont(1, next)));
        entries->push_back(range(0xE0, 0xE0, range(0xA0, 0xBF, cont(1, next))));
        entries->push_back(range(0xE1, 0xEC, cont(2, next)));
        entries->push_back(range(0xED, 0xED, range(0x80, 0x9F, cont(1, next))));
        entries->push_back(range(0xEE, 0xEF, cont(2, next)));
        entries->push_back(range(0xF0, 0xF0, range(0x90, 0xBF, cont(2, next))));
        entries->push_back(range(0xF1, 0xF3, cont(3, next)));
        entries->push_back(range(0xF4, 0xF4, range(0x80, 0x8F, cont(2, next))));
    }

    // the entry of a fragment for n that continues at next
    int compile(const Node &n, int next) {
        switch (n.kind) {
            case Node::Empty: return next;
            case Node::Bytes: {
                for (size_t i = n.bytes.size(); i-- > 0;) next = range((uint8_t)n.bytes[i], (uint8_t)n.bytes[i], next);
                return next;
            }
            case Node::Set: {
                std::vector<int> entries;
                for (int b = 0; b < 128;) {
                    if (!n.ascii[b]) {
                        ++b;
                        continue;
                    }
                    int e = b;
                    while (e + 1 < 128 && n.ascii[e + 1]) ++e;
                    entries.push_back(range(b, e, next));
                    b = e + 1;
                }
                if (n.non_ascii) non_ascii_scalars(&entries, next);
                return any_of(entries, next);
            }
            case Node::Cat: {
                for (size_t i = n.kids.size(); i-- > 0;) next = compile(*n.kids[i], next);
                return next;
            }
            case Node::Alt: {
                std::vector<int> entries;
                for (const auto &k : n.kids) entries.push_back(compile(*k, next));
                return any_of(entries, next);
            }
            case Node::Repeat: {
                const Node &k = *n.kids[0];
                int tail = next;
                if (n.max < 0) {
                    const int loop = split(-1, next);
                    st[loop].out = compile(k, loop);
                    tail = loop;
                } else {
                    for (int i = n.min; i < n.max; ++i) tail = split(compile(k, tail), next);
                }
                for (int i = 0; i < n.min; ++i) tail = compile(k, tail);
                return tail;
            }
            case Node::Start: return add(NState{NState::AssertStart, 0, 0, next, -1});
            case Node::End: return add(NState{NState::AssertEnd, 0, 0, next, -1});
        }
        return next;
    }
};

Nfa build_nfa(const std::vector<const Node *> &trees) {
    Nfa nfa;
    const int match = nfa.add(NState{NState::Match, 0, 0, -1, -1});
    std::vector<int> entries;
    for (const Node *t : trees) entries.push_back(nfa.compile(*t, match));
    nfa.start = nfa.any_of(entries, match);
    return nfa;
}

// the states that decide what a set does (ranges, assertions, the match state) reachable from `core` without a byte; the
// assertions stay in the set, so closing a closed set again with more of them true follows them
struct Closer {
    const Nfa &nfa;
    std::vector<uint32_t> seen;
    uint32_t stamp = 0;
    std::vector<int> stack;
    explicit Closer(const Nfa &n) : nfa(n), seen(n.st.size(), 0) {}

    std::vector<int> close(const std::vector<int> &core, bool at_start, bool at_end, bool *matched) {
        ++stamp;
        std::vector<int> out;
        *matched = false;
        stack.assign(core.begin(), core.end());
        while (!stack.empty()) {
            const int s = stack.back();
            stack.pop_back();
            if (s < 0 || seen[s] == stamp) continue;
            seen[s] = stamp;
            const NState &x = nfa.st[s];
            switch (x.kind) {
                case NState::Split:
                    stack.push_back(x.out);
                    stack.push_back(x.out1);
                    break;
                case NState::AssertStart:
                    out.push_back(s);
                    if (at_start) stack.push_back(x.out);
                    break;
                case NState::AssertEnd:
                    out.push_back(s);
                    if (at_end) stack.push_back(x.out);
                    break;
                case NState::Match:
                    *matched = true;
                    out.push_back(s);
                    break;
                case NState::Range: out.push_back(s); break;
            }
        }
        std::sort(out.begin(), out.end());
        return out;
    }

    std::vector<int> step(const std::vector<int> &set, uint8_t b) const {
        std::vector<int> core;
        for (int s : set) {
            const NState &x = nfa.st[s];
            if (x.kind == NState::Range && x.lo <= b && b <= x.hi) core.push_back(x.out);
        }
        core.push_back(nfa.start);  // the unanchored search: a match may begin at every position
        return core;
    }
};

// ---- subset construction -------------------------------------------------------------------------------------------------------
// the default cap: the table (states x classes x 2 bytes) and the 256-byte class map together stay within 64 KiB, the LDS a
// block of k_attr_match_dfa stages them in
uint32_t default_cap(uint32_t n_classes) { return std::max<uint32_t>(2, std::min<uint32_t>(65535, (32768 - 128) / n_classes)); }

uint32_t cap_from_env() {
    const char *e = std::getenv("GFFX_SEARCH_DFA_STATES");
    if (e && *e) {
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 2 && v <= 65535) return (uint32_t)v;
    }
    return 0;
}

// false: more than the cap's states
bool determinise(const Nfa &nfa, uint32_t max_states, Dfa *d, uint32_t *cap_used) {
    // byte classes from the ranges' ends (known before the construction, so the default cap can follow the table's width)
    bool cut[257] = {};
    cut[0] = true;
    for (const NState &x : nfa.st)
        if (x.kind == NState::Range && x.lo <= x.hi) cut[x.lo] = true, cut[(int)x.hi + 1] = true;
    uint8_t rep[256];
    int n_cls = 0;
    for (int b = 0; b < 256; ++b) {
        if (cut[b]) rep[n_cls++] = (uint8_t)b;
        d->cls[b] = (uint8_t)(n_cls - 1);
    }
    d->n_classes = (uint32_t)n_cls + 1;
    const uint32_t cap = max_states ? max_states : default_cap(d->n_classes);
    *cap_used = cap;

    Closer cl(nfa);
    std::map<std::pair<std::vector<int>, bool>, uint32_t> ids;
    std::vector<std::pair<std::vector<int>, bool>> sets;  // by state number; [0] is the accepting state
    sets.emplace_back(std::vector<int>{}, false);
    d->trans.assign(d->n_classes, 0);  // the accepting state's row: absorbing
    bool ok = true;
    auto number_of = [&](std::vector<int> set, bool matched, bool initial) -> uint32_t {
        if (matched) return search::kAccept;
        if (initial) {  // being at the start only matters to a set that holds a `^`, or a `$` that may hide one (`$^`)
            initial = false;
            for (int st : set) initial = initial || nfa.st[st].kind == NState::AssertStart || nfa.st[st].kind == NState::AssertEnd;
        }
        auto key = std::make_pair(std::move(set), initial);
        auto it = ids.find(key);
        if (it != ids.end()) return it->second;
        if (sets.size() >= cap) {
            ok = false;
            return search::kAccept;
        }
        const uint32_t id = (uint32_t)sets.size();
        ids.emplace(key, id);
        sets.push_back(std::move(key));
        d->trans.resize((size_t)(id + 1) * d->n_classes, 0);
        return id;
    };
    bool matched = false;
    std::vector<int> s0 = cl.close({nfa.start}, true, false, &matched);
    d->init = number_of(std::move(s0), matched, true);
    uint32_t restart = 0;
    bool restart_known = false;
    for (uint32_t id = 1; ok && id < sets.size(); ++id) {
        const std::vector<int> set = sets[id].first;  // (a copy: sets grows below)
        const bool initial = sets[id].second;
        for (int c = 0; c < n_cls && ok; ++c) {
            const std::vector<int> core = cl.step(set, rep[c]);
            uint32_t to;
            if (core.size() == 1 && restart_known) {  // no range took the byte: only the re-entered start state
                to = restart;
            } else {
                std::vector<int> t = cl.close(core, false, false, &matched);
                to = number_of(std::move(t), matched, false);
                if (core.size() == 1 && ok) restart = to, restart_known = true;
            }
            d->trans[(size_t)id * d->n_classes + c] = (uint16_t)to;
        }
        (void)cl.close(set, initial, true, &matched);  // the end of the text: `$` holds, `^` only in the initial state
        d->trans[(size_t)id * d->n_classes + n_cls] = (uint16_t)(matched ? search::kAccept : id);
    }
    d->n_states = (uint32_t)sets.size();
    return ok;
}

}  // namespace

std::string check_syntax(const std::string &pattern) {
    try {
        (void)parse_pattern(pattern);
    } catch (const SyntaxError &e) {
        return syntax_message(pattern, e);
    }
    return "";
}

Compiled compile(const std::vector<std::string> &patterns, uint32_t max_states) {
    if (max_states == 1 || max_states > 65535) throw Error("regex state cap " + std::to_string(max_states) + " (2 to 65535)");
    if (!max_states) max_states = cap_from_env();
    std::vector<NodeP> trees;
    for (const std::string &p : patterns) {
        try {
            trees.push_back(parse_pattern(p));
        } catch (const SyntaxError &e) {
            throw Error(syntax_message(p, e));
        }
    }
    Compiled out;
    auto build = [&](size_t first, size_t n, Dfa *d, uint32_t *cap) {
        std::vector<const Node *> part;
        for (size_t i = first; i < first + n; ++i) part.push_back(trees[i].get());
        const Nfa nfa = build_nfa(part);
        d->first_pattern = (uint32_t)first;
        d->n_patterns = (uint32_t)n;
        return determinise(nfa, max_states, d, cap);
    };
    // greedy in list order: a group takes patterns while their union stays under the cap (tried in growing, then
    // shrinking steps: a group ends where the next pattern alone no longer fits)
    for (size_t k = 0; k < trees.size();) {
        Dfa best;
        uint32_t cap = 0;
        if (!build(k, 1, &best, &cap))
            throw Error("regex too large: \"" + patterns[k] + "\" needs more than " + std::to_string(cap) + " DFA states");
        if (out.groups.empty()) out.max_states = cap;
        size_t size = 1, step = 1;
        bool growing = true;
        while (k + size < trees.size()) {
            const size_t want = std::min(size + step, trees.size() - k);
            Dfa d;
            if (build(k, want, &d, &cap)) {
                best = std::move(d);
                size = want;
                if (growing) step *= 2;
            } else {
                if (step == 1) break;
                growing = false;
                step /= 2;
            }
        }
        out.groups.push_back(std::move(best));
        k += size;
    }
    return out;
}

bool nfa_match(const std::vector<std::string> &patterns, std::string_view value) {
    std::vector<NodeP> trees;
    std::vector<const Node *> part;
    for (const std::string &p : patterns) {
        try {
            trees.push_back(parse_pattern(p));
        } catch (const SyntaxError &e) {
            throw Error(syntax_message(p, e));
        }
        part.push_back(trees.back().get());
    }
    const Nfa nfa = build_nfa(part);
    Closer cl(nfa);
    bool matched = false;
    std::vector<int> cur = cl.close({nfa.start}, true, false, &matched);
    if (matched) return true;
    for (size_t i = 0; i < value.size(); ++i) {
        cur = cl.close(cl.step(cur, (uint8_t)value[i]), false, false, &matched);
        if (matched) return true;
    }
    (void)cl.close(cur, value.empty(), true, &matched);
    return matched;
}

bool dfa_match(const Compiled &c, std::string_view value) {
    for (const Dfa &g : c.groups) {
        const search::Dfa d{g.cls, g.trans.data(), g.n_states, g.n_classes, g.init};
        if (search::dfa_match(d, reinterpret_cast<const uint8_t *>(value.data()), value.size())) return true;
    }
    return false;
}

}  // namespace gffx::regex
