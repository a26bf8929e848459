// table_output.hpp -- the output of the commands that write a table (`gffx closest`, `gffx annotate`): a file, or stdout when
// no path is given; every short write and a failing close is an Error that names the target.
#pragma once
#include <cstdio>
#include <optional>
#include <string>

#include "gffx.hpp"

namespace gffx::commands {

struct Output {
    FILE *f = stdout;
    std::string path;
    explicit Output(const std::optional<std::string> &p) {
        if (!p) return;
        path = *p;
        f = std::fopen(path.c_str(), "wb");
        if (!f) throw Error("Cannot create output file: \"" + path + "\"");
    }
    void write(const std::string &s) {
        if (!s.empty() && std::fwrite(s.data(), 1, s.size(), f) != s.size()) throw Error("Cannot write " + (path.empty() ? std::string("stdout") : path));
    }
    void close() {
        const bool own = f != stdout;
        const int rc = own ? std::fclose(f) : std::fflush(f);
        f = stdout;
        if (rc != 0) throw Error("Cannot write " + (path.empty() ? std::string("stdout") : path));
    }
    ~Output() {
        if (f != stdout) std::fclose(f);
    }
};

}  // namespace gffx::commands
