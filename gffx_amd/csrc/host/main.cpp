// main.cpp -- `gffx` command line for the intersect path: `gffx index` (prerequisite),
// `gffx intersect`, `gffx extract`, `gffx search`, `gffx depth` (BED source), `gffx closest`, `gffx annotate`, `gffx enrich` and `gffx meta` (additions) (reference: main.rs:11-39, commands/depth.rs:34-72, commands/extract.rs:16-35, commands/search.rs:18-51, commands/index.rs:11-23, commands/intersect.rs:32-70,
// utils/common.rs:17-52).  Flag names, short flags, defaults and groups follow the reference's
// clap derive; usage errors exit 2 like clap, run-time errors print `Error: <msg>` and exit 1.
#include <unistd.h>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>

#include <thread>

#include "gffx.hpp"

namespace gffx {

namespace {

struct UsageError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

struct OptSpec {
    char short_name;  // 0 = none
    const char *long_name;
    bool takes_value;
};

// clap-style scan: -x VALUE, -xVALUE, -x=VALUE, --long VALUE, --long=VALUE, bundled -ev
std::map<std::string, std::vector<std::string>> parse_opts(int argc, char **argv, int first,
                                                           const std::vector<OptSpec> &specs) {
    std::map<std::string, std::vector<std::string>> got;
    auto find_long = [&](const std::string &n) -> const OptSpec * {
        for (const auto &s : specs)
            if (n == s.long_name) return &s;
        return nullptr;
    };
    auto find_short = [&](char c) -> const OptSpec * {
        for (const auto &s : specs)
            if (s.short_name && s.short_name == c) return &s;
        return nullptr;
    };
    for (int i = first; i < argc; ++i) {
        const std::string a = argv[i];
        if (a.rfind("--", 0) == 0 && a.size() > 2) {
            const size_t eq = a.find('=');
            const std::string name = a.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
            const OptSpec *s = find_long(name);
            if (!s) throw UsageError("unexpected argument '--" + name + "' found");
            if (s->takes_value) {
                if (eq != std::string::npos) {
                    got[s->long_name].push_back(a.substr(eq + 1));
                } else {
                    if (i + 1 >= argc) throw UsageError("a value is required for '--" + name + "' but none was supplied");
                    got[s->long_name].push_back(argv[++i]);
                }
            } else {
                if (eq != std::string::npos) throw UsageError("unexpected value for '--" + name + "'");
                got[s->long_name].push_back("");
            }
        } else if (a.size() >= 2 && a[0] == '-' && a != "--") {
            for (size_t k = 1; k < a.size(); ++k) {
                const OptSpec *s = find_short(a[k]);
                if (!s) throw UsageError(std::string("unexpected argument '-") + a[k] + "' found");
                if (s->takes_value) {
                    std::string v = a.substr(k + 1);
                    if (!v.empty() && v[0] == '=') v.erase(0, 1);
                    if (v.empty()) {
                        if (i + 1 >= argc)
                            throw UsageError(std::string("a value is required for '-") + a[k] + "' but none was supplied");
                        v = argv[++i];
                    }
                    got[s->long_name].push_back(v);
                    break;
                }
                got[s->long_name].push_back("");
            }
        } else {
            throw UsageError("unexpected argument '" + a + "' found");
        }
    }
    for (const auto &[name, vals] : got)
        if (vals.size() > 1)
            throw UsageError("the argument '--" + name + "' cannot be used multiple times");
    return got;
}

const char *kTopUsage =
    "Usage: gffx <COMMAND>\n\nCommands:\n"
    "  index      Build index for GFF file\n"
    "  intersect  Extract models by a region or regions from a BED file (MI355X engine)\n"
    "  extract    Extract models by feature IDs (MI355X engine)\n"
    "  search     Search features by attribute values (MI355X engine)\n"
    "  depth      Compute coverage depth across genomic features from a BED, BAM or SAM file (MI355X engine)\n"
    "  coverage   Compute coverage breadth across genomic features from a BED, BAM or SAM file (MI355X engine)\n"
    "  closest    Report the nearest root features of a region or of the regions of a BED file (MI355X engine)\n"
    "  annotate   Count the bases of a region or of the regions of a BED file by feature class (MI355X engine)\n"
    "  enrich     Test the regions of a BED file against feature classes by permutation (MI355X engine)\n"
    "  meta       Sum the depth of a BED, BAM or SAM file around features, along their strand (MI355X engine)\n"
    "  help       Print this message\n";

const char *kIntersectUsage =
    "Usage: gffx intersect [OPTIONS] --input <FILE> <--region <REGION>|--bed <BED>>\n\nOptions:\n"
    "  -i, --input <FILE>       Input GFF file path\n"
    "  -o, --output <FILE>      Output file (stdout if not provided)\n"
    "  -e, --entire_group       Return the entire feature group for each match\n"
    "  -T, --types <TYPES>      Comma-separated feature types to retain (e.g. exon,gene)\n"
    "  -t, --threads <NUM>      Number of threads for parallel processing [default: 12]\n"
    "  -v, --verbose            Enable verbose output\n"
    "  -r, --region <REGION>    Single region in format \"chr:start-end\"\n"
    "  -b, --bed <BED>          BED file containing regions\n"
    "  -c, --contained          Only return features fully contained within regions\n"
    "  -C, --contains-region    Only return features that fully contain the regions\n"
    "  -O, --overlap            Return any overlapping features (default)\n"
    "  -I, --invert             Invert the selection (exclude matching features)\n"
    "      --device <N>         HIP device to run on [default: 0]\n"
    "      --gpus <N>           Shard the BED regions by chromosome bucket over N devices [default: 1]\n"
    "      --stats-json <FILE>  Write the run's stage timers and counts as one JSON object\n";

const char *kExtractUsage =
    "Usage: gffx extract [OPTIONS] --input <FILE> <--feature-file <FEATURE_FILE>|--feature-id <FEATURE_ID>>\n\nOptions:\n"
    "  -i, --input <FILE>                 Input GFF file path\n"
    "  -o, --output <FILE>                Output file (stdout if not provided)\n"
    "  -e, --entire_group                 Return the entire feature group for each match\n"
    "  -T, --types <TYPES>                Comma-separated feature types to retain (e.g. exon,gene)\n"
    "  -t, --threads <NUM>                Number of threads for parallel processing [default: 12]\n"
    "  -v, --verbose                      Enable verbose output\n"
    "  -f, --feature-id <FEATURE_ID>      A single feature ID\n"
    "  -F, --feature-file <FEATURE_FILE>  File with one feature ID per line\n"
    "      --device <N>                   HIP device to run on [default: 0]\n"
    "      --stats-json <FILE>            Write the run's stage timers and counts as one JSON object\n";

const char *kSearchUsage =
    "Usage: gffx search [OPTIONS] --input <FILE> <--attr-list <ATTR_LIST>|--attr <ATTR>>\n\nOptions:\n"
    "  -i, --input <FILE>           Input GFF file path\n"
    "  -o, --output <FILE>          Output file (stdout if not provided)\n"
    "  -e, --entire_group           Return the entire feature group for each match\n"
    "  -T, --types <TYPES>          Comma-separated feature types to retain (e.g. exon,gene)\n"
    "  -t, --threads <NUM>          Number of threads for parallel processing [default: 12]\n"
    "  -v, --verbose                Enable verbose output\n"
    "  -A, --attr-list <ATTR_LIST>  Attribute list file (one per line)\n"
    "  -a, --attr <ATTR>            Single attribute value to search\n"
    "  -r, --regex                  Enable regex mode for attribute matching (a subset of the syntax: see DESIGN.md)\n"
    "      --device <N>             HIP device to run on [default: 0]\n"
    "      --stats-json <FILE>      Write the run's stage timers and counts as one JSON object\n";

const char *kDepthUsage =
    "Usage: gffx depth [OPTIONS] --input <FILE> --source <SOURCE>\n\nOptions:\n"
    "  -i, --input <FILE>           Input GFF file path\n"
    "  -s, --source <SOURCE>        Input source (BED, BAM or SAM; CRAM is not supported)\n"
    "  -o, --output <FILE>          Output file (stdout if not provided)\n"
    "      --bin-shift <BIN_SHIFT>  Bin width parameter (2^k bp) [default: 12]\n"
    "  -t, --threads <THREADS>      Number of threads for parallel processing [default: 12]\n"
    "  -v, --verbose                Enable verbose output\n"
    "      --device <N>             HIP device to run on [default: 0]\n"
    "      --gpus <N>               Spread the BED, BAM or SAM rows over N devices [default: 1]\n";

const char *kCoverageUsage =
    "Usage: gffx coverage [OPTIONS] --input <FILE> --source <SOURCE>\n\nOptions:\n"
    "  -i, --input <FILE>       Input GFF file path\n"
    "  -s, --source <SOURCE>    Input source (BED, BAM or SAM; CRAM is not supported)\n"
    "  -o, --output <FILE>      Output file (stdout if not provided)\n"
    "  -t, --threads <NUM>      Number of threads for parallel processing [default: 12]\n"
    "  -v, --verbose            Enable verbose output\n"
    "      --device <N>         HIP device to run on [default: 0]\n"
    "      --gpus <N>           Spread the BED, BAM or SAM rows over N devices [default: 1]\n"
    "      --mean-depth         Add the columns bases, length and mean_depth (per-base depth of the feature's lines)\n"
    "      --thresholds <T1,T2,...>  Add the columns bases_ge<T> and fraction_ge<T> for one to eight depths T >= 1: the bases of\n"
    "                           the feature's lines at depth >= T among ALL rows of the seqid (so bases_ge1 can exceed breadth,\n"
    "                           which counts only rows that hit the feature's root) and their share of the lines' bases\n"
    "      --bedgraph <FILE>    Write the per-base depth of the source rows as a bedGraph (seqid, start, end, depth; depth > 0)\n"
    "      --stats-json <FILE>  Write the run's stage timers and counts as one JSON object\n";

const char *kClosestUsage =
    "Usage: gffx closest [OPTIONS] --input <FILE> <--region <REGION>|--bed <BED>>\n\nOptions:\n"
    "  -i, --input <FILE>       Input GFF file path\n"
    "  -o, --output <FILE>      Output file (stdout if not provided)\n"
    "  -r, --region <REGION>    Single region in format \"chr:start-end\"\n"
    "  -b, --bed <BED>          BED file containing regions (plain or bgzipped, as for intersect)\n"
    "      --ignore-overlaps    Do not report features that overlap the region: the nearest ones beside it\n"
    "      --side <SIDE>        Which features count beside the overlapping ones: both, left (ending at or before the\n"
    "                           region's start) or right (starting at or after its end) [default: both]\n"
    "  -t, --threads <NUM>      Number of threads for parallel processing [default: 12]\n"
    "  -v, --verbose            Enable verbose output\n"
    "      --device <N>         HIP device to run on [default: 0]\n"
    "      --stats-json <FILE>  Write the run's stage timers and counts as one JSON object\n\n"
    "Output: a header line, then one line per nearest root feature, in the order of the regions:\n"
    "  chr, start, end (as parsed), id, feature_start, feature_end (0-based, half-open), distance (0: overlap;\n"
    "  negative: the feature lies left of the region; adjacent intervals are 1 apart).  All features at the smallest\n"
    "  distance are reported; a region with none prints one line with '.' in the last four columns.\n";

const char *kAnnotateUsage =
    "Usage: gffx annotate [OPTIONS] --input <FILE> --types <T1,T2,...> <--region <REGION>|--bed <BED>>\n\nOptions:\n"
    "  -i, --input <FILE>       Input GFF file path\n"
    "  -o, --output <FILE>      Output file (stdout if not provided)\n"
    "  -r, --region <REGION>    Single region in format \"chr:start-end\"\n"
    "  -b, --bed <BED>          BED file containing regions (plain or bgzipped, as for closest)\n"
    "  -T, --types <T1,T2,...>  One to 32 feature types (column 3) in priority order, no name twice: a base belongs to the\n"
    "                           first type with a line that covers it, e.g. CDS,five_prime_UTR,three_prime_UTR,exon,gene\n"
    "      --summary <FILE>     Write one line per type and one for 'none': name, regions of that class, bases over all regions\n"
    "  -t, --threads <NUM>      Number of threads for parallel processing [default: 12]\n"
    "  -v, --verbose            Enable verbose output\n"
    "      --device <N>         HIP device to run on [default: 0]\n"
    "      --stats-json <FILE>  Write the run's stage timers and counts as one JSON object\n\n"
    "Output: a header line '#chr start end class <T1> ... none', then one line per region, in the order of the regions:\n"
    "  chr, start, end (as parsed), the first type with at least one base in the region ('.' for none), and the region's\n"
    "  bases per type and outside all of them; the counts add up to end - start.  Strand is ignored.\n";

const char *kEnrichUsage =
    "Usage: gffx enrich [OPTIONS] --input <FILE> --bed <BED> --types <T1,T2,...> --permutations <N>\n\nOptions:\n"
    "  -i, --input <FILE>       Input GFF file path\n"
    "  -o, --output <FILE>      Output file (stdout if not provided)\n"
    "  -b, --bed <BED>          BED file containing regions (plain or bgzipped, as for annotate)\n"
    "  -T, --types <T1,T2,...>  One to 32 feature types in priority order, as for annotate\n"
    "  -n, --permutations <N>   Number of permutations, 1 to 1048576: every region is moved to a random place on its own\n"
    "                           seqid N times\n"
    "      --seed <S>           Seed of the random numbers, 64 bits [default: 0]; the same seed gives the same output\n"
    "  -g, --genome <FILE>      Lengths of the seqids, 'name<TAB>length' per line (a .fai works: further columns are ignored).\n"
    "                           Without it a seqid's length is the largest end of its lines in the GFF file, which understates\n"
    "                           the real chromosome: -g is the right choice\n"
    "      --perms <FILE>       Write the raw totals, one line per row (0: observed, 1 .. N: the permutations): the row, the\n"
    "                           bases per type and outside all, the regions per class\n"
    "  -t, --threads <NUM>      Number of threads for parallel processing [default: 12]\n"
    "  -v, --verbose            Enable verbose output\n"
    "      --device <N>         HIP device to run on [default: 0]\n"
    "      --stats-json <FILE>  Write the run's stage timers and counts as one JSON object\n\n"
    "Output: a header line, then per type and for 'none' one line for 'bases' and one for 'regions':\n"
    "  class, quantity, observed, mean, sd, z, fold (observed / mean), n_ge and n_le (permutations with a value >= / <= the\n"
    "  observed one), p_ge = (n_ge + 1) / (N + 1) and p_le.  A region wider than its seqid stays where it is (a warning says\n"
    "  how many).  Regions may overlap each other after placement.\n";

const char *kMetaUsage =
    "Usage: gffx meta [OPTIONS] --input <FILE> --source <SOURCE>\n\nOptions:\n"
    "  -i, --input <FILE>       Input GFF file path\n"
    "  -s, --source <SOURCE>    Input source (BED, plain or bgzipped, BAM or SAM), as for coverage\n"
    "  -o, --output <FILE>      Output file (stdout if not provided)\n"
    "  -T, --types <T1,T2,...>  Feature types (column 3) whose lines are the features [default: gene]\n"
    "      --anchor <ANCHOR>    Point mode: columns around the feature's tss (its 5' end), tes (its 3' end) or center\n"
    "                           [default: tss]\n"
    "      --scale <M>          Scaled mode instead: every feature's body becomes M columns, whatever its length\n"
    "  -u, --upstream <UP>      Bases before the anchor or the body, a multiple of BIN [default: 2000]\n"
    "  -d, --downstream <DOWN>  Bases behind the anchor or the body, a multiple of BIN [default: 2000]\n"
    "  -w, --bin <BIN>          Bases per column outside the body [default: 10]\n"
    "  -g, --genome <FILE>      Lengths of the seqids, 'name<TAB>length' per line (a .fai works), as for enrich: columns are\n"
    "                           cut at a seqid's end.  Without it they are cut at 0 only\n"
    "      --matrix <FILE>      Write one line per feature: chr, start, end, id, strand and its bases per column\n"
    "  -t, --threads <NUM>      Number of threads for parallel processing [default: 12]\n"
    "  -v, --verbose            Enable verbose output\n"
    "      --device <N>         HIP device to run on [default: 0]\n"
    "      --gpus <N>           Spread the source rows over N devices [default: 1]\n"
    "      --stats-json <FILE>  Write the run's stage timers and counts as one JSON object\n\n"
    "Output: a header line, then one line per column, in the direction of transcription (a feature on '-' is mirrored):\n"
    "  column, part (point, up, body, down), from and to (offsets from the anchor, the 5' end or the 3' end; body columns\n"
    "  count from 0 to M), features with bases in the column, bases (summed depth), length, mean_depth = bases / length.\n"
    "  A strand other than '+' or '-' counts as '+' (a warning says how many).\n";

const char *kIndexUsage =
    "Usage: gffx index [OPTIONS] --input <INPUT>\n\nOptions:\n"
    "  -i, --input <INPUT>\n"
    "  -a, --attribute <ATTRIBUTE>    [default: gene_name]\n"
    "  -s, --skip-types <SKIP_TYPES>  [default: remark,note,comment,region,gap,assembly_gap,contig,scaffold,source]\n"
    "  -v, --verbose\n"
    "  -g, --gpu                      Build the side-cars on the HIP device (same bytes; no CPU fallback)\n"
    "      --device <N>               HIP device of --gpu [default: 0]\n";

size_t parse_size(const std::string &v, const char *flag) {
    const auto x = parse_u32_rust(v);
    if (!x) throw UsageError(std::string("invalid value '") + v + "' for '" + flag + "'");
    return *x;
}

int run_intersect_cli(int argc, char **argv) {
    static const std::vector<OptSpec> specs = {
        {'i', "input", true},   {'o', "output", true},     {'e', "entire_group", false}, {'T', "types", true},
        {'t', "threads", true}, {'v', "verbose", false},   {'r', "region", true},        {'b', "bed", true},
        {'c', "contained", false}, {'C', "contains-region", false}, {'O', "overlap", false},
        {'I', "invert", false}, {0, "device", true},       {0, "gpus", true},           {0, "stats-json", true},
        {'h', "help", false}};
    const auto o = parse_opts(argc, argv, 2, specs);
    if (o.count("help")) {
        std::fputs(kIntersectUsage, stdout);
        return 0;
    }
    commands::intersect::IntersectArgs a;
    if (!o.count("input")) throw UsageError("the following required arguments were not provided:\n  --input <FILE>");
    a.common.input = o.at("input")[0];
    if (o.count("output")) a.common.output = o.at("output")[0];
    a.common.entire_group = o.count("entire_group") > 0;
    if (o.count("types")) a.common.types = o.at("types")[0];
    if (o.count("threads")) a.common.threads = parse_size(o.at("threads")[0], "--threads <NUM>");
    a.common.verbose = o.count("verbose") > 0;
    if (o.count("region")) a.region = o.at("region")[0];
    if (o.count("bed")) a.bed = o.at("bed")[0];
    // ArgGroup "regions": required, exactly one (intersect.rs:37-39)
    if (a.region && a.bed)
        throw UsageError("the argument '--region <REGION>' cannot be used with '--bed <BED>'");
    if (!a.region && !a.bed)
        throw UsageError("the following required arguments were not provided:\n  <--region <REGION>|--bed <BED>>");
    a.contained = o.count("contained") > 0;
    a.contains_region = o.count("contains-region") > 0;
    a.overlap = o.count("overlap") > 0;
    if (a.contained + a.contains_region + a.overlap > 1)  // ArgGroup "mode" (intersect.rs:40-42)
        throw UsageError("the arguments '--contained', '--contains-region' and '--overlap' cannot be used together");
    a.invert = o.count("invert") > 0;
    if (o.count("device")) a.device = static_cast<int>(parse_size(o.at("device")[0], "--device <N>"));
    if (o.count("gpus")) a.gpus = static_cast<int>(std::max<size_t>(1, std::min<size_t>(64, parse_size(o.at("gpus")[0], "--gpus <N>"))));
    if (o.count("stats-json")) g_run_stats.path = o.at("stats-json")[0];
    commands::intersect::run(a);
    return 0;
}

int run_extract_cli(int argc, char **argv) {
    static const std::vector<OptSpec> specs = {
        {'i', "input", true},   {'o', "output", true},   {'e', "entire_group", false}, {'T', "types", true},
        {'t', "threads", true}, {'v', "verbose", false}, {'f', "feature-id", true},    {'F', "feature-file", true},
        {0, "device", true},    {0, "stats-json", true}, {'h', "help", false}};
    const auto o = parse_opts(argc, argv, 2, specs);
    if (o.count("help")) {
        std::fputs(kExtractUsage, stdout);
        return 0;
    }
    commands::extract::ExtractArgs a;
    if (!o.count("input")) throw UsageError("the following required arguments were not provided:\n  --input <FILE>");
    a.common.input = o.at("input")[0];
    if (o.count("output")) a.common.output = o.at("output")[0];
    a.common.entire_group = o.count("entire_group") > 0;
    if (o.count("types")) a.common.types = o.at("types")[0];
    if (o.count("threads")) a.common.threads = parse_size(o.at("threads")[0], "--threads <NUM>");
    a.common.verbose = o.count("verbose") > 0;
    if (o.count("feature-id")) a.feature_id = o.at("feature-id")[0];
    if (o.count("feature-file")) a.feature_file = o.at("feature-file")[0];
    // ArgGroup "feature": required, exactly one (extract.rs:21-25)
    if (a.feature_id && a.feature_file)
        throw UsageError("the argument '--feature-id <FEATURE_ID>' cannot be used with '--feature-file <FEATURE_FILE>'");
    if (!a.feature_id && !a.feature_file)
        throw UsageError("the following required arguments were not provided:\n  <--feature-file <FEATURE_FILE>|--feature-id <FEATURE_ID>>");
    if (o.count("device")) a.device = static_cast<int>(parse_size(o.at("device")[0], "--device <N>"));
    if (o.count("stats-json")) g_run_stats.path = o.at("stats-json")[0];
    commands::extract::run_extract(a);
    return 0;
}

int run_search_cli(int argc, char **argv) {
    static const std::vector<OptSpec> specs = {
        {'i', "input", true},   {'o', "output", true},   {'e', "entire_group", false}, {'T', "types", true},
        {'t', "threads", true}, {'v', "verbose", false}, {'A', "attr-list", true},     {'a', "attr", true},
        {'r', "regex", false},  {0, "device", true},     {0, "stats-json", true},      {'h', "help", false}};
    const auto o = parse_opts(argc, argv, 2, specs);
    if (o.count("help")) {
        std::fputs(kSearchUsage, stdout);
        return 0;
    }
    commands::search::SearchArgs a;
    if (!o.count("input")) throw UsageError("the following required arguments were not provided:\n  --input <FILE>");
    a.common.input = o.at("input")[0];
    if (o.count("output")) a.common.output = o.at("output")[0];
    a.common.entire_group = o.count("entire_group") > 0;
    if (o.count("types")) a.common.types = o.at("types")[0];
    if (o.count("threads")) a.common.threads = parse_size(o.at("threads")[0], "--threads <NUM>");
    a.common.verbose = o.count("verbose") > 0;
    if (o.count("attr-list")) a.attr_list = o.at("attr-list")[0];
    if (o.count("attr")) a.attr = o.at("attr")[0];
    a.regex = o.count("regex") > 0;
    // ArgGroup "attr_input": required, exactly one (search.rs:19-24)
    if (a.attr_list && a.attr) throw UsageError("the argument '--attr-list <ATTR_LIST>' cannot be used with '--attr <ATTR>'");
    if (!a.attr_list && !a.attr)
        throw UsageError("the following required arguments were not provided:\n  <--attr-list <ATTR_LIST>|--attr <ATTR>>");
    if (o.count("device")) a.device = static_cast<int>(parse_size(o.at("device")[0], "--device <N>"));
    if (o.count("stats-json")) g_run_stats.path = o.at("stats-json")[0];
    commands::search::run_search(a);
    return 0;
}

int run_depth_cli(int argc, char **argv) {
    static const std::vector<OptSpec> specs = {{'i', "input", true},   {'s', "source", true},   {'o', "output", true},
                                               {0, "bin-shift", true}, {'t', "threads", true},  {'v', "verbose", false},
                                               {0, "device", true},    {0, "gpus", true},       {0, "stats-json", true}, {'h', "help", false}};
    const auto o = parse_opts(argc, argv, 2, specs);
    if (o.count("help")) {
        std::fputs(kDepthUsage, stdout);
        return 0;
    }
    commands::depth::DepthArgs a;
    if (!o.count("input") || !o.count("source"))
        throw UsageError(std::string("the following required arguments were not provided:") +
                         (o.count("input") ? "" : "\n  --input <FILE>") + (o.count("source") ? "" : "\n  --source <SOURCE>"));
    a.input = o.at("input")[0];
    a.source = o.at("source")[0];
    if (o.count("output")) a.output = o.at("output")[0];
    if (o.count("bin-shift")) a.bin_shift = static_cast<uint32_t>(parse_size(o.at("bin-shift")[0], "--bin-shift <BIN_SHIFT>"));
    if (o.count("threads")) a.threads = parse_size(o.at("threads")[0], "--threads <THREADS>");
    a.verbose = o.count("verbose") > 0;
    if (o.count("device")) a.device = static_cast<int>(parse_size(o.at("device")[0], "--device <N>"));
    if (o.count("gpus")) a.gpus = static_cast<int>(std::max<size_t>(1, std::min<size_t>(64, parse_size(o.at("gpus")[0], "--gpus <N>"))));
    if (o.count("stats-json")) g_run_stats.path = o.at("stats-json")[0];
    commands::depth::run(a);
    return 0;
}

// --thresholds T1,T2,...: one to eight integers in 1 .. 4294967295, no duplicates
std::vector<uint32_t> parse_thresholds(const std::string &v) {
    const char *flag = "'--thresholds <T1,T2,...>'";
    std::vector<uint32_t> out;
    size_t at = 0;
    while (true) {
        const size_t comma = v.find(',', at);
        const std::string item = v.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
        const bool digits = !item.empty() && item.size() <= 10 && item.find_first_not_of("0123456789") == std::string::npos;
        const unsigned long long x = digits ? std::strtoull(item.c_str(), nullptr, 10) : 0ull;
        if (!digits || x == 0 || x > 0xFFFFFFFFull)
            throw Error("invalid value '" + v + "' for " + flag + ": '" + item + "' is not an integer in 1 .. 4294967295");
        if (std::find(out.begin(), out.end(), static_cast<uint32_t>(x)) != out.end())
            throw Error("invalid value '" + v + "' for " + flag + ": " + item + " is given twice");
        out.push_back(static_cast<uint32_t>(x));
        if (out.size() > 8) throw Error("invalid value '" + v + "' for " + flag + ": more than eight thresholds");
        if (comma == std::string::npos) break;
        at = comma + 1;
    }
    return out;
}

int run_coverage_cli(int argc, char **argv) {
    static const std::vector<OptSpec> specs = {{'i', "input", true},   {'s', "source", true},   {'o', "output", true},
                                               {'t', "threads", true}, {'v', "verbose", false}, {0, "device", true},
                                               {0, "gpus", true},      {0, "stats-json", true}, {0, "mean-depth", false},
                                               {0, "thresholds", true}, {0, "bedgraph", true},  {'h', "help", false}};
    const auto o = parse_opts(argc, argv, 2, specs);
    if (o.count("help")) {
        std::fputs(kCoverageUsage, stdout);
        return 0;
    }
    commands::coverage::CoverageArgs a;
    if (!o.count("input") || !o.count("source"))
        throw UsageError(std::string("the following required arguments were not provided:") +
                         (o.count("input") ? "" : "\n  --input <FILE>") + (o.count("source") ? "" : "\n  --source <SOURCE>"));
    a.input = o.at("input")[0];
    a.source = o.at("source")[0];
    if (o.count("output")) a.output = o.at("output")[0];
    if (o.count("threads")) a.threads = parse_size(o.at("threads")[0], "--threads <NUM>");
    a.verbose = o.count("verbose") > 0;
    if (o.count("device")) a.device = static_cast<int>(parse_size(o.at("device")[0], "--device <N>"));
    if (o.count("gpus")) a.gpus = static_cast<int>(std::max<size_t>(1, std::min<size_t>(64, parse_size(o.at("gpus")[0], "--gpus <N>"))));
    if (o.count("stats-json")) g_run_stats.path = o.at("stats-json")[0];
    a.mean_depth = o.count("mean-depth") > 0;
    if (o.count("thresholds")) a.thresholds = parse_thresholds(o.at("thresholds")[0]);
    if (o.count("bedgraph")) a.bedgraph = o.at("bedgraph")[0];
    commands::coverage::run(a);
    return 0;
}

int run_closest_cli(int argc, char **argv) {
    static const std::vector<OptSpec> specs = {{'i', "input", true},   {'o', "output", true},          {'r', "region", true}, {'b', "bed", true},
                                               {0, "ignore-overlaps", false}, {0, "side", true},       {'t', "threads", true}, {'v', "verbose", false},
                                               {0, "device", true},    {0, "stats-json", true},        {'h', "help", false}};
    const auto o = parse_opts(argc, argv, 2, specs);
    if (o.count("help")) {
        std::fputs(kClosestUsage, stdout);
        return 0;
    }
    commands::closest::ClosestArgs a;
    if (!o.count("input")) throw UsageError("the following required arguments were not provided:\n  --input <FILE>");
    a.common.input = o.at("input")[0];
    if (o.count("output")) a.common.output = o.at("output")[0];
    if (o.count("threads")) a.common.threads = parse_size(o.at("threads")[0], "--threads <NUM>");
    a.common.verbose = o.count("verbose") > 0;
    if (o.count("region")) a.region = o.at("region")[0];
    if (o.count("bed")) a.bed = o.at("bed")[0];
    if (a.region && a.bed) throw UsageError("the argument '--region <REGION>' cannot be used with '--bed <BED>'");
    if (!a.region && !a.bed) throw UsageError("the following required arguments were not provided:\n  <--region <REGION>|--bed <BED>>");
    a.ignore_overlaps = o.count("ignore-overlaps") > 0;
    if (o.count("side")) {
        const std::string &v = o.at("side")[0];
        if (v == "both")
            a.side = commands::closest::Side::Both;
        else if (v == "left")
            a.side = commands::closest::Side::Left;
        else if (v == "right")
            a.side = commands::closest::Side::Right;
        else
            throw UsageError("invalid value '" + v + "' for '--side <SIDE>'\n  [possible values: both, left, right]");
    }
    if (o.count("device")) a.device = static_cast<int>(parse_size(o.at("device")[0], "--device <N>"));
    if (o.count("stats-json")) g_run_stats.path = o.at("stats-json")[0];
    commands::closest::run(a);
    return 0;
}

// -T: one to 32 names, none empty, none twice
std::vector<std::string> parse_layers(const std::string &v) {
    std::vector<std::string> layers;
    for (size_t at = 0;;) {
        const size_t c = v.find(',', at);
        const std::string name = v.substr(at, c == std::string::npos ? std::string::npos : c - at);
        if (name.empty()) throw UsageError("invalid value '" + v + "' for '--types <T1,T2,...>': an empty type name");
        if (std::find(layers.begin(), layers.end(), name) != layers.end())
            throw UsageError("invalid value '" + v + "' for '--types <T1,T2,...>': '" + name + "' is given twice");
        layers.push_back(name);
        if (c == std::string::npos) break;
        at = c + 1;
    }
    if (layers.size() > 32) throw UsageError("invalid value '" + v + "' for '--types <T1,T2,...>': more than 32 types");
    return layers;
}

int run_annotate_cli(int argc, char **argv) {
    static const std::vector<OptSpec> specs = {{'i', "input", true},   {'o', "output", true},  {'r', "region", true}, {'b', "bed", true},
                                               {'T', "types", true},   {0, "summary", true},   {'t', "threads", true}, {'v', "verbose", false},
                                               {0, "device", true},    {0, "stats-json", true}, {'h', "help", false}};
    const auto o = parse_opts(argc, argv, 2, specs);
    if (o.count("help")) {
        std::fputs(kAnnotateUsage, stdout);
        return 0;
    }
    commands::annotate::AnnotateArgs a;
    if (!o.count("input")) throw UsageError("the following required arguments were not provided:\n  --input <FILE>");
    a.common.input = o.at("input")[0];
    if (o.count("output")) a.common.output = o.at("output")[0];
    if (o.count("threads")) a.common.threads = parse_size(o.at("threads")[0], "--threads <NUM>");
    a.common.verbose = o.count("verbose") > 0;
    if (o.count("region")) a.region = o.at("region")[0];
    if (o.count("bed")) a.bed = o.at("bed")[0];
    if (a.region && a.bed) throw UsageError("the argument '--region <REGION>' cannot be used with '--bed <BED>'");
    if (!a.region && !a.bed) throw UsageError("the following required arguments were not provided:\n  <--region <REGION>|--bed <BED>>");
    if (!o.count("types")) throw UsageError("the following required arguments were not provided:\n  --types <T1,T2,...>");
    a.layers = parse_layers(o.at("types")[0]);
    if (o.count("summary")) a.summary = o.at("summary")[0];
    if (o.count("device")) a.device = static_cast<int>(parse_size(o.at("device")[0], "--device <N>"));
    if (o.count("stats-json")) g_run_stats.path = o.at("stats-json")[0];
    commands::annotate::run(a);
    return 0;
}

int run_enrich_cli(int argc, char **argv) {
    static const std::vector<OptSpec> specs = {{'i', "input", true},   {'o', "output", true},       {'b', "bed", true},     {'T', "types", true},
                                               {'n', "permutations", true}, {0, "seed", true},      {'g', "genome", true},  {0, "perms", true},
                                               {'t', "threads", true}, {'v', "verbose", false},     {0, "device", true},    {0, "stats-json", true},
                                               {'h', "help", false}};
    const auto o = parse_opts(argc, argv, 2, specs);
    if (o.count("help")) {
        std::fputs(kEnrichUsage, stdout);
        return 0;
    }
    commands::enrich::EnrichArgs a;
    std::string missing;
    for (const char *name : {"input", "bed", "types", "permutations"})
        if (!o.count(name))
            missing += std::string("\n  --") + name + (std::string(name) == "input" ? " <FILE>" : std::string(name) == "bed" ? " <BED>" : std::string(name) == "types" ? " <T1,T2,...>" : " <N>");
    if (!missing.empty()) throw UsageError("the following required arguments were not provided:" + missing);
    a.common.input = o.at("input")[0];
    if (o.count("output")) a.common.output = o.at("output")[0];
    if (o.count("threads")) a.common.threads = parse_size(o.at("threads")[0], "--threads <NUM>");
    a.common.verbose = o.count("verbose") > 0;
    a.bed = o.at("bed")[0];
    a.layers = parse_layers(o.at("types")[0]);
    {
        const std::string &v = o.at("permutations")[0];
        const size_t n = parse_size(v, "--permutations <N>");
        if (n < 1 || n > (1u << 20)) throw UsageError("invalid value '" + v + "' for '--permutations <N>': 1 to 1048576 are possible");
        a.n_perm = static_cast<uint32_t>(n);
    }
    if (o.count("seed")) {
        const std::string &v = o.at("seed")[0];
        char *end = nullptr;
        errno = 0;
        const unsigned long long s = std::strtoull(v.c_str(), &end, 10);
        if (v.empty() || v[0] < '0' || v[0] > '9' || *end || errno == ERANGE) throw UsageError("invalid value '" + v + "' for '--seed <S>': a number below 2^64 is expected");
        a.seed = s;
    }
    if (o.count("genome")) a.genome = o.at("genome")[0];
    if (o.count("perms")) a.perms = o.at("perms")[0];
    if (o.count("device")) a.device = static_cast<int>(parse_size(o.at("device")[0], "--device <N>"));
    if (o.count("stats-json")) g_run_stats.path = o.at("stats-json")[0];
    commands::enrich::run(a);
    return 0;
}

int run_meta_cli(int argc, char **argv) {
    static const std::vector<OptSpec> specs = {{'i', "input", true},    {'s', "source", true},     {'o', "output", true},  {'T', "types", true},
                                               {0, "anchor", true},     {0, "scale", true},        {'u', "upstream", true}, {'d', "downstream", true},
                                               {'w', "bin", true},      {'g', "genome", true},     {0, "matrix", true},    {'t', "threads", true},
                                               {'v', "verbose", false}, {0, "device", true},       {0, "gpus", true},      {0, "stats-json", true},
                                               {'h', "help", false}};
    const auto o = parse_opts(argc, argv, 2, specs);
    if (o.count("help")) {
        std::fputs(kMetaUsage, stdout);
        return 0;
    }
    commands::meta::MetaArgs a;
    if (!o.count("input") || !o.count("source"))
        throw UsageError(std::string("the following required arguments were not provided:") + (o.count("input") ? "" : "\n  --input <FILE>") +
                         (o.count("source") ? "" : "\n  --source <SOURCE>"));
    a.common.input = o.at("input")[0];
    a.source = o.at("source")[0];
    if (o.count("output")) a.common.output = o.at("output")[0];
    if (o.count("threads")) a.common.threads = parse_size(o.at("threads")[0], "--threads <NUM>");
    a.common.verbose = o.count("verbose") > 0;
    if (o.count("types")) a.types = parse_layers(o.at("types")[0]);
    if (o.count("anchor") && o.count("scale")) throw UsageError("the argument '--anchor <ANCHOR>' cannot be used with '--scale <M>'");
    gffx_hip_meta_layout &y = a.layout;
    if (o.count("anchor")) {
        const std::string &v = o.at("anchor")[0];
        if (v == "tss")
            y.anchor = 0;
        else if (v == "tes")
            y.anchor = 1;
        else if (v == "center")
            y.anchor = 2;
        else
            throw UsageError("invalid value '" + v + "' for '--anchor <ANCHOR>'\n  [possible values: tss, tes, center]");
    }
    if (o.count("upstream")) y.up = static_cast<uint32_t>(parse_size(o.at("upstream")[0], "--upstream <UP>"));
    if (o.count("downstream")) y.down = static_cast<uint32_t>(parse_size(o.at("downstream")[0], "--downstream <DOWN>"));
    if (o.count("bin")) y.bin = static_cast<uint32_t>(parse_size(o.at("bin")[0], "--bin <BIN>"));
    if (o.count("scale")) {
        y.mode = 1;
        y.body_bins = static_cast<uint32_t>(parse_size(o.at("scale")[0], "--scale <M>"));
        if (y.body_bins == 0) throw UsageError("invalid value '0' for '--scale <M>': at least one body column is needed");
    }
    if (y.bin == 0) throw UsageError("invalid value '0' for '--bin <BIN>': a column has at least one base");
    if (y.up % y.bin) throw UsageError("invalid value '" + std::to_string(y.up) + "' for '--upstream <UP>': not a multiple of --bin " + std::to_string(y.bin));
    if (y.down % y.bin) throw UsageError("invalid value '" + std::to_string(y.down) + "' for '--downstream <DOWN>': not a multiple of --bin " + std::to_string(y.bin));
    if (y.mode == 0 && static_cast<uint64_t>(y.up) + y.down == 0) throw UsageError("--upstream and --downstream are both 0: there is no column");
    if (gffx_hip_pileup_meta_columns(&y) > gffx_hip_pileup_meta_max_columns())
        throw UsageError(std::to_string(gffx_hip_pileup_meta_columns(&y)) + " columns exceed the limit of " + std::to_string(gffx_hip_pileup_meta_max_columns()) +
                         ": choose a larger --bin or a smaller --scale");
    if (o.count("genome")) a.genome = o.at("genome")[0];
    if (o.count("matrix")) a.matrix = o.at("matrix")[0];
    if (o.count("device")) a.device = static_cast<int>(parse_size(o.at("device")[0], "--device <N>"));
    if (o.count("gpus")) a.gpus = static_cast<int>(std::max<size_t>(1, std::min<size_t>(64, parse_size(o.at("gpus")[0], "--gpus <N>"))));
    if (o.count("stats-json")) g_run_stats.path = o.at("stats-json")[0];
    commands::meta::run(a);
    return 0;
}

int run_index_cli(int argc, char **argv) {
    static const std::vector<OptSpec> specs = {{'i', "input", true},
                                               {'a', "attribute", true},
                                               {'s', "skip-types", true},
                                               {'v', "verbose", false},
                                               {'g', "gpu", false},
                                               {0, "device", true},
                                               {'h', "help", false}};
    const auto o = parse_opts(argc, argv, 2, specs);
    if (o.count("help")) {
        std::fputs(kIndexUsage, stdout);
        return 0;
    }
    if (!o.count("input")) throw UsageError("the following required arguments were not provided:\n  --input <INPUT>");
    const std::string input = o.at("input")[0];
    const std::string attr = o.count("attribute") ? o.at("attribute")[0] : "gene_name";  // commands/index.rs:15
    const std::string skip = o.count("skip-types")
                                 ? o.at("skip-types")[0]
                                 : "remark,note,comment,region,gap,assembly_gap,contig,scaffold,source";  // :18
    const bool verbose = o.count("verbose") > 0;
    if (verbose) std::printf("Indexing: %s\n", input.c_str());  // commands/index.rs:26-28
    // addition: --gpu builds the same eight files from arrays made on the device (GFFX_INDEX_CHUNK_BYTES: the text per pass)
    if (o.count("gpu"))
        build_index_device(input, attr, skip, o.count("device") ? static_cast<int>(parse_size(o.at("device")[0], "--device <N>")) : 0, verbose);
    else
        build_index(input, attr, skip, verbose);
    // addition: the all-line SoA image `<gff>.lsoa` for depth / coverage (block_table.cpp); GFFX_LINE_TABLE=off skips it
    const char *lt = std::getenv("GFFX_LINE_TABLE");
    if (!(lt && std::string(lt) == "off")) {
        const index_loader::GofMap gof = index_loader::load_gof(input);
        const MappedFile text(input);
        unsigned hw = std::thread::hardware_concurrency();
        // Both images are optional accelerators (the commands fall back to the text walk without them): a failure to write one
        // -- a full or read-only directory, a quota -- is a warning, the partial file is removed, and the index the reference
        // defines (the eight side-cars above) stands.
        try {
            const auto t = commands::depth::build_block_table(gof, text.view(), std::min(hw ? hw : 1u, 12u));
            commands::depth::write_block_table(append_suffix(input, ".lsoa"), t, text.size(), index_loader::line_table_key(input, gof));
            if (verbose) std::printf("Line table image: %zu lines in %zu blocks.\n", t.line_start.size(), t.block_line_off.size() - 1);
        } catch (const Error &e) {
            std::fprintf(stderr, "[WARN] line table image %s not written: %s\n", append_suffix(input, ".lsoa").c_str(), e.what());
            std::remove(append_suffix(input, ".lsoa").c_str());
        }
        // ... and the all-line table `<gff>.lall` of intersect's per-line mode (line_index.cpp)
        try {
            const auto all = commands::intersect::build_all_lines(text.view(), std::min(hw ? hw : 1u, 12u));
            commands::intersect::write_all_lines(append_suffix(input, ".lall"), all, text.size(), index_loader::line_table_key(input, gof));
            if (verbose) std::printf("All-line table: %zu lines, %zu seqid names, %zu types.\n", all.ls.size(), all.seq_names.size(), all.type_names.size());
        } catch (const Error &e) {
            std::fprintf(stderr, "[WARN] all-line table %s not written: %s\n", append_suffix(input, ".lall").c_str(), e.what());
            std::remove(append_suffix(input, ".lall").c_str());
        }
    } else {
        std::remove(append_suffix(input, ".lsoa").c_str());  // an image of an earlier index run would be stale
        std::remove(append_suffix(input, ".lall").c_str());
    }
    if (verbose) std::printf("Index created successfully.\n");
    return 0;
}

}  // namespace

int cli_main(int argc, char **argv) {
    const char *usage = kTopUsage;
    try {
        if (argc < 2) throw UsageError("a subcommand is required");
        const std::string cmd = argv[1];
        if (cmd == "help" || cmd == "--help" || cmd == "-h") {
            std::fputs(kTopUsage, stdout);
            return 0;
        }
        if (cmd == "intersect") {
            usage = kIntersectUsage;
            return run_intersect_cli(argc, argv);
        }
        if (cmd == "index") {
            usage = kIndexUsage;
            return run_index_cli(argc, argv);
        }
        if (cmd == "extract") {
            usage = kExtractUsage;
            return run_extract_cli(argc, argv);
        }
        if (cmd == "search") {
            usage = kSearchUsage;
            return run_search_cli(argc, argv);
        }
        if (cmd == "depth") {
            usage = kDepthUsage;
            return run_depth_cli(argc, argv);
        }
        if (cmd == "coverage") {
            usage = kCoverageUsage;
            return run_coverage_cli(argc, argv);
        }
        if (cmd == "closest") {
            usage = kClosestUsage;
            return run_closest_cli(argc, argv);
        }
        if (cmd == "annotate") {
            usage = kAnnotateUsage;
            return run_annotate_cli(argc, argv);
        }
        if (cmd == "enrich") {
            usage = kEnrichUsage;
            return run_enrich_cli(argc, argv);
        }
        if (cmd == "meta") {
            usage = kMetaUsage;
            return run_meta_cli(argc, argv);
        }
        throw UsageError("unrecognized subcommand '" + cmd + "' (this build carries the intersect, extract, search, depth, coverage, closest, annotate, enrich and meta paths only)");
    } catch (const UsageError &e) {
        std::fprintf(stderr, "error: %s\n\n%s\nFor more information, try '--help'.\n", e.what(), usage);
        return 2;
    } catch (const Error &e) {
        std::fprintf(stderr, "Error: %s\n", e.what());
        return 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "Error: %s\n", e.what());
        return 1;
    }
}

}  // namespace gffx

#ifndef GFFX_NO_MAIN
// The process ends the ordinary way: destructors, atexit handlers, HIP runtime shutdown.  GFFX_EXIT=fast (opt-in, for
// throughput runs on multi-GB inputs) skips that teardown once cli_main has closed and checked every output it wrote --
// unmapping a 2.4 GB BED file, freeing the region stores and shutting HIP down cost ~0.1 s of a 0.9 s run there, and the
// kernel reclaims all of it faster when the process simply ends.  Never under a preloaded tool (a profiler flushes its
// trace from an exit handler).
int main(int argc, char **argv) {
    const int rc = gffx::cli_main(argc, argv);
    const char *how = std::getenv("GFFX_EXIT");
    if (!(how && std::string(how) == "fast")) return rc;
    const char *preload = std::getenv("LD_PRELOAD");
    if ((preload && *preload) || std::getenv("ROCP_TOOL_LIBRARIES") || std::getenv("ROCPROFILER_REGISTER_ROOT") || std::getenv("HSA_TOOLS_LIB"))
        return rc;
    std::fflush(stdout);
    std::fflush(stderr);
    _exit(rc);
}
#endif
