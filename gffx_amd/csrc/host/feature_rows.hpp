// feature_rows.hpp -- what `gffx meta` needs of a feature's line beyond layer_rows.hpp's columns: the strand (column 7) and the
// ID (column 9).  The line table has neither, and its format stays as it is: for the few chosen lines they are read from the
// mapped text, at the line's start.  `gffx seq` reads the phase (column 8) and the Parent attribute the same way.  Plain C++17
// on a string_view (tools/meta_check.cpp and tools/seq_check.cpp build it under the sanitizers).
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

// What `gffx seq` needs of a line on top of that: column 7 as it prints it, the phase (column 8) and the Parent attribute.
struct SeqFields {
    StrandId si;
    char strand = '.';  // '+', '-', or '.' when column 7 is neither
    char phase = '.';   // column 8 when it is one character, else '.'
    // the value of the first attribute of column 9 whose key is Parent ("Parent=" at the column's start or right behind a ';',
    // as ID= is found), up to ';' or the line's end; empty if there is none
    std::string_view parent;
};

inline SeqFields read_seq_fields(std::string_view text, uint64_t line_start) {
    SeqFields r;
    r.si = read_strand_id(text, line_start);
    r.strand = r.si.minus ? '-' : r.si.stranded ? '+' : '.';
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
        if (col == 8 && field.size() == 1) r.phase = field[0];
        if (col == 9) {
            size_t k = field.find("Parent=");
            while (k != std::string_view::npos && k > 0 && field[k - 1] != ';') k = field.find("Parent=", k + 1);
            if (k != std::string_view::npos) {
                size_t end = field.find(';', k + 7);
                if (end == std::string_view::npos) end = field.size();
                r.parent = field.substr(k + 7, end - k - 7);
            }
        }
        if (tab == line.size()) break;
        at = tab + 1;
    }
    return r;
}

// fn(name) for every name of a Parent value, in order: the value split at ',', empty names dropped
template <typename F>
void for_each_parent(std::string_view value, F &&fn) {
    for (size_t at = 0; at <= value.size();) {
        size_t c = value.find(',', at);
        if (c == std::string_view::npos) c = value.size();
        if (c > at) fn(value.substr(at, c - at));
        at = c + 1;
    }
}

}  // namespace gffx::commands::feature_rows
