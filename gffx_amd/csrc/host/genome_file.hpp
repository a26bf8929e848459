// genome_file.hpp -- the -g file of `gffx enrich` and `gffx meta`: the lengths of the seqids.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "gffx.hpp"

namespace gffx::commands {

// -g: `name<TAB>length` per line, further columns ignored (a .fai works); empty lines and lines that begin with '#' are
// skipped, so are names the index does not know; of a name given twice the last line counts.  Every seqid of the index
// must be there.
inline std::vector<uint32_t> read_genome(const std::string &path, const std::vector<std::string> &num_to_seqid, const std::unordered_map<std::string, uint32_t> &seqid_to_num) {
    const MappedFile file = map_file_or(path, "Cannot open genome file: \"" + path + "\"");
    const std::string_view text = file.view();
    std::vector<uint32_t> len(num_to_seqid.size(), 0);
    std::vector<bool> seen(num_to_seqid.size(), false);
    size_t line_no = 0;
    for (size_t at = 0; at < text.size();) {
        size_t nl = text.find('\n', at);
        if (nl == std::string_view::npos) nl = text.size();
        std::string_view line = text.substr(at, nl - at);
        at = nl + 1;
        ++line_no;
        if (!line.empty() && line.back() == '\r') line.remove_suffix(1);
        if (line.empty() || line[0] == '#') continue;
        const size_t tab = line.find('\t');
        const auto bad = [&](const char *what) { return Error("genome file " + path + ", line " + std::to_string(line_no) + ": " + what); };
        if (tab == std::string_view::npos || tab == 0) throw bad("expected name<TAB>length");
        size_t num_end = tab + 1;
        while (num_end < line.size() && line[num_end] != '\t') ++num_end;
        const std::string_view num = line.substr(tab + 1, num_end - tab - 1);
        if (num.empty() || num.size() > 10) throw bad("the length is not a number below 2^32");
        uint64_t v = 0;
        for (const char ch : num) {
            if (ch < '0' || ch > '9') throw bad("the length is not a number below 2^32");
            v = v * 10 + static_cast<uint64_t>(ch - '0');
        }
        if (v > 0xFFFFFFFFull) throw bad("the length is not a number below 2^32");
        const auto it = seqid_to_num.find(std::string(line.substr(0, tab)));
        if (it == seqid_to_num.end() || it->second >= len.size()) continue;
        len[it->second] = static_cast<uint32_t>(v), seen[it->second] = true;
    }
    for (size_t c = 0; c < len.size(); ++c)
        if (!seen[c]) throw Error("genome file " + path + " has no length for seqid '" + num_to_seqid[c] + "'");
    return len;
}

}  // namespace gffx::commands
