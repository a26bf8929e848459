// feature_rows.hpp -- what `gffx meta` needs of a feature's line beyond layer_rows.hpp's columns: the strand (column 7) and the
// ID (column 9).  The line table has neither, and its format stays as it is: for the few chosen lines they are read from the
// mapped text, at the line's start.  Plain C++17 on a string_view (tools/meta_check.cpp builds it under the sanitizers).
#pragma once
#include <cstdint>
#include <string_view>

namespace gffx::commands::feature_rows {

struct StrandId {
    bool minus = false;     // column 7 is "-"; "+", ".", "?" and anything else is plus
    bool stranded = false;  // column 7 is "+" or "-"
    // the value of the first attribute of column 9 whose key is ID ("ID=" at the column's start or right behind a ';', so that
    // geneID= or Parent_ID= are not taken for it), up to ';' or the line's end; "." if there is none or it is empty
    std::string_view id = ".";
};

// the line that begins at text[line_start] (it ends at '\n' or the text's end; a '\r' before that is not part of it)
inline StrandId read_strand_id(std::string_view text, uint64_t line_start) {
    StrandId r;
    if (line_start >= text.size()) return r;
    size_t nl = text.find('\n', line_start);
    if (nl == std::string_view::npos) nl = text.size();
    std::string_view line = text.substr(line_start, nl - line_start);
    if (!line.empty() && line.back() == '\r') line.remove_suffix(1);
    size_t at = 0;
    for (int col = 1; col <= 9; ++col) {
        size_t tab = line.find('\t', at);
        if (tab == std::string_view::npos) tab = line.size();
        const std::string_view field = line.substr(at, tab - at);
        if (col == 7) {
            r.minus = field == "-";
            r.stranded = r.minus || field == "+";
        } else if (col == 9) {
            size_t k = field.find("ID=");
            while (k != std::string_view::npos && k > 0 && field[k - 1] != ';') k = field.find("ID=", k + 1);
            if (k != std::string_view::npos) {
                size_t end = field.find(';', k + 3);
                if (end == std::string_view::npos) end = field.size();
                if (end > k + 3) r.id = field.substr(k + 3, end - k - 3);
            }
        }
        if (tab == line.size()) break;
        at = tab + 1;
    }
    return r;
}

}  // namespace gffx::commands::feature_rows
