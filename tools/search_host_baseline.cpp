// search_host_baseline.cpp -- the yardstick of tools/search_bench.py: step 1 of the reference's `gffx search`
// (commands/search.rs:89-111) RESTATED for one host core -- NOT the Rust binary, which cannot be built here.
//   exact: the wanted strings in a hash set, every `.atn` value looked up (search.rs:105-110);
//   regex: every value against every pattern until one matches (search.rs:99-103: values x patterns matcher calls), each
//          pattern its own DFA of this project's compiler (host/regex_dfa.cpp) walked by device/search_core.hpp's loop.
// LIMIT > 0 takes only the first LIMIT values (the regex pass over millions of values x 1 K patterns runs for minutes);
// the caller scales the time by values / values_used and says so.
//   search_host_baseline ATN PATTERNS exact|regex [LIMIT]    -> one JSON line
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <string_view>
#include <unordered_set>
#include <vector>

#include "../gffx_amd/csrc/device/search_core.hpp"
#include "../gffx_amd/csrc/host/regex_dfa.hpp"
#include "../gffx_amd/csrc/host/text.hpp"

using namespace gffx;
using Clock = std::chrono::steady_clock;

static double ms_since(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }

static std::vector<std::string_view> lines(std::string_view d) {
    std::vector<std::string_view> out;
    for (size_t a = 0; a < d.size();) {
        size_t nl = d.find('\n', a);
        if (nl == std::string_view::npos) nl = d.size();
        const std::string_view l = trim_unicode_ws(d.substr(a, nl - a));
        if (!l.empty()) out.push_back(l);
        a = nl + 1;
    }
    return out;
}

int main(int argc, char **argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: search_host_baseline ATN PATTERNS exact|regex [LIMIT]\n");
        return 2;
    }
    try {
        const bool regex_mode = std::string(argv[3]) == "regex";
        const size_t limit = argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 0;
        auto t = Clock::now();
        const MappedFile atn(argv[1]), pf(argv[2]);
        std::vector<std::string_view> values;
        for (std::string_view l : lines(atn.view()))  // (core.rs:59-68, without its error cases)
            if (l[0] != '#') values.push_back(l);
        const std::vector<std::string_view> patterns = lines(pf.view());
        const double load_ms = ms_since(t);
        const size_t used = limit && limit < values.size() ? limit : values.size();
        size_t matched = 0;
        double compile_ms = 0, match_ms = 0;
        if (regex_mode) {
            t = Clock::now();
            std::vector<regex::Compiled> res;
            for (std::string_view p : patterns) res.push_back(regex::compile({std::string(p)}, 65535));
            compile_ms = ms_since(t);
            t = Clock::now();
            for (size_t i = 0; i < used; ++i)
                for (const regex::Compiled &c : res)
                    if (regex::dfa_match(c, values[i])) {
                        ++matched;
                        break;
                    }
            match_ms = ms_since(t);
        } else {
            t = Clock::now();
            const std::unordered_set<std::string_view> wanted(patterns.begin(), patterns.end());
            compile_ms = ms_since(t);
            t = Clock::now();
            for (size_t i = 0; i < used; ++i) matched += wanted.count(values[i]);
            match_ms = ms_since(t);
        }
        std::printf("{\"values\": %zu, \"values_used\": %zu, \"patterns\": %zu, \"load_ms\": %.3f, \"compile_ms\": %.3f, \"match_ms\": %.3f, \"matched\": %zu}\n",
                    values.size(), used, patterns.size(), load_ms, compile_ms, match_ms, matched);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "Error: %s\n", e.what());
        return 1;
    }
    return 0;
}
