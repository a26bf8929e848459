// regex_dfa.hpp -- the regex subset of `gffx search -r`, compiled on the host: parser -> Thompson NFA over bytes -> subset
// construction -> byte classes -> flat tables that device/search_core.hpp's match loop walks (host and device alike).
//
// THE RULE OF THE SUBSET: whatever is accepted means exactly what the reference's `Regex::is_match` on a &str means
// (commands/search.rs:93-103: the `regex` crate's defaults, an unanchored search, Unicode scalars as the unit); everything
// else is refused with `unsupported regex syntax at byte N of "<pattern>": <what>`.  Nothing is accepted with another meaning.
//   accepted: literal scalars (a non-ASCII one is its UTF-8 sequence and ONE atom for a quantifier); `.` (any scalar but
//     '\n'); [...] and [^...] of ASCII singles and ranges (a leading ']', a leading or trailing '-' and a non-leading '^' are
//     literal; a negated class also takes every non-ASCII scalar); * + ? {m} {m,} {m,n} (counts <= 255) and their lazy forms
//     (is_match cannot tell them apart); | with empty alternates; ( ) and (?: ); ^ and $ as start / end of the text; the
//     escapes \\ \. \+ \* \? \( \) \| \[ \] \{ \} \^ \$ \-.
//   refused: every other escape (\d \w \s \b are Unicode-aware in the reference), inline flags and named groups, non-ASCII
//     members or an unescaped '[' inside a class, && -- ~~ inside a class, a malformed '{', a quantifier directly after a
//     quantifier or an anchor, or with nothing before it; groups nested more than 100 deep (the parser recurses per level).
//
// All patterns of a run are ONE alternation (the reference only asks `any`).  State 0 is the accepting state and absorbing;
// end of text is a symbol of its own, the last column of the table.  The determinisation has a state cap (default: the
// table, states x classes x 2 bytes, stays at or under 64 KiB; GFFX_SEARCH_DFA_STATES or max_states override it, 2 to
// 65535); when the union exceeds it the patterns are split, in list order, into groups with one DFA each, whose results
// are ORed; a single pattern over the cap is `regex too large`.
#pragma once
#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

namespace gffx::regex {

struct Dfa {
    uint32_t n_states = 0, n_classes = 0;  // n_classes counts the end-of-text class, the last column
    uint32_t init = 0;
    uint32_t first_pattern = 0, n_patterns = 0;  // the patterns [first_pattern, first_pattern + n_patterns) of the list
    uint8_t cls[256] = {};                       // byte -> column
    std::vector<uint16_t> trans;                 // n_states x n_classes
};

struct Compiled {
    std::vector<Dfa> groups;
    uint32_t max_states = 0;  // the cap that was in force for the first group
};

// throws gffx::Error with the messages above
Compiled compile(const std::vector<std::string> &patterns, uint32_t max_states = 0);
// the parser alone: "" when the pattern is accepted, else the message
std::string check_syntax(const std::string &pattern);
// the union of the patterns run as an NFA on the bytes, no tables: what the DFA is checked against
bool nfa_match(const std::vector<std::string> &patterns, std::string_view value);
bool dfa_match(const Compiled &c, std::string_view value);

}  // namespace gffx::regex
