// extract_host_baseline.cpp -- a ONE-CORE host run of the steps of `gffx extract`, for tools/extract_bench.py: a RESTATEMENT OF
// THE REFERENCE ALGORITHM, NOT THE RUST BINARY (the reference cannot be built here).  std::unordered_map build over the `.fts`
// names (fts.rs:16-22) and lookup of the requested names (fts.rs:41-93), the array chase (prt.rs:54-72, with the product's
// bound), and write_gff_output_filtered's scan of the hit blocks with memchr / memmem (common.rs:289-465) against per-root
// sets of ID strings.  Prints one JSON object with the wall-clock milliseconds of each step.
//   extract_host_baseline GFF NAMES    (the GFF has been indexed: GFF.fts, GFF.prt, GFF.gof are read)
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace {
std::string slurp(const std::string &path) {
    std::string s;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path.c_str());
        std::exit(2);
    }
    char buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
    std::fclose(f);
    return s;
}
std::vector<std::string_view> lines_of(const std::string &s) {
    std::vector<std::string_view> out;
    size_t a = 0;
    while (a < s.size()) {
        size_t e = s.find('\n', a);
        if (e == std::string::npos) e = s.size();
        if (e > a) out.emplace_back(s.data() + a, e - a);
        a = e + 1;
    }
    return out;
}
double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}
uint64_t le64(const char *p) {
    uint64_t v;
    std::memcpy(&v, p, 8);
    return v;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: extract_host_baseline GFF NAMES\n");
        return 2;
    }
    const std::string gff_path = argv[1];
    const std::string fts = slurp(gff_path + ".fts"), prt_raw = slurp(gff_path + ".prt"), gof = slurp(gff_path + ".gof"), names_raw = slurp(argv[2]);
    const std::string gff = slurp(gff_path);
    const std::vector<std::string_view> ids = lines_of(fts), names = lines_of(names_raw);
    std::vector<uint32_t> prt(prt_raw.size() / 4);
    std::memcpy(prt.data(), prt_raw.data(), prt.size() * 4);
    const uint32_t n = (uint32_t)prt.size();

    auto t = std::chrono::steady_clock::now();
    std::unordered_map<std::string, uint32_t> fwd;
    fwd.reserve(ids.size());
    for (uint32_t i = 0; i < ids.size(); ++i) fwd[std::string(ids[i])] = i;
    const double build_ms = ms_since(t);

    t = std::chrono::steady_clock::now();
    std::vector<uint32_t> fids;
    size_t missing = 0;
    for (std::string_view nm : names) {
        const auto it = fwd.find(std::string(nm));
        if (it == fwd.end()) ++missing;
        else fids.push_back(it->second);
    }
    const double lookup_ms = ms_since(t);

    t = std::chrono::steady_clock::now();
    std::vector<uint32_t> roots(fids.size());
    for (size_t i = 0; i < fids.size(); ++i) {
        uint32_t cur = fids[i], r = UINT32_MAX;
        for (uint32_t steps = 0; steps < n && cur < n; ++steps) {
            const uint32_t p = prt[cur];
            if (p == cur) {
                r = cur;
                break;
            }
            if (p >= n) break;
            cur = p;
        }
        roots[i] = r;
    }
    const double chase_ms = ms_since(t);

    t = std::chrono::steady_clock::now();
    std::unordered_map<uint32_t, std::unordered_set<std::string>> per_root;
    for (size_t i = 0; i < fids.size(); ++i)
        if (roots[i] != UINT32_MAX && fids[i] < ids.size()) per_root[roots[i]].insert(std::string(ids[fids[i]]));
    std::unordered_map<uint32_t, std::pair<uint64_t, uint64_t>> block;
    for (size_t o = 0; o + 24 <= gof.size(); o += 24) {
        uint32_t fid;
        std::memcpy(&fid, gof.data() + o, 4);
        block[fid] = {le64(gof.data() + o + 8), le64(gof.data() + o + 16)};
    }
    uint64_t kept_lines = 0, kept_bytes = 0, scanned = 0;
    for (const auto &[root, keep] : per_root) {
        const auto it = block.find(root);
        if (it == block.end()) continue;
        const uint64_t s = it->second.first, e = std::min<uint64_t>(it->second.second, gff.size());
        for (uint64_t pos = s; pos < e;) {
            const void *nl = std::memchr(gff.data() + pos, '\n', e - pos);
            const uint64_t next = nl ? (uint64_t)((const char *)nl - gff.data()) + 1 : e;
            uint64_t end = next;
            if (end > pos && gff[end - 1] == '\n') --end;
            if (end > pos && gff[end - 1] == '\r') --end;
            scanned += next - pos;
            if (gff[pos] != '#') {
                const char *p = gff.data() + pos, *z = gff.data() + end;
                int tabs = 0;
                while (tabs < 8 && p < z) {
                    const void *tb = std::memchr(p, '\t', z - p);
                    if (!tb) break;
                    p = (const char *)tb + 1;
                    ++tabs;
                }
                if (tabs == 8) {
                    const void *k = memmem(p, z - p, "ID=", 3);
                    if (k) {
                        const char *v = (const char *)k + 3;
                        const void *semi = std::memchr(v, ';', z - v);
                        const char *ve = semi ? (const char *)semi : z;
                        if (keep.count(std::string(v, ve - v))) {
                            ++kept_lines;
                            kept_bytes += next - pos;
                        }
                    }
                }
            }
            pos = next;
        }
    }
    const double filter_ms = ms_since(t);
    std::printf("{\"table_names\": %zu, \"names\": %zu, \"missing\": %zu, \"roots\": %zu, \"scanned_bytes\": %llu, \"kept_lines\": %llu, "
                "\"kept_bytes\": %llu, \"map_build_ms\": %.3f, \"map_lookup_ms\": %.3f, \"chase_ms\": %.3f, \"filter_ms\": %.3f}\n",
                ids.size(), names.size(), missing, per_root.size(), (unsigned long long)scanned, (unsigned long long)kept_lines,
                (unsigned long long)kept_bytes, build_ms, lookup_ms, chase_ms, filter_ms);
    return 0;
}
