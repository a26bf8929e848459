// main.cpp -- `gffx` command line for the intersect path: `gffx index` (prerequisite),
// `gffx intersect`, `gffx extract`, `gffx search`, `gffx depth` (BED source), `gffx closest`, `gffx annotate`, `gffx enrich`, `gffx meta`, `gffx seq` and `gffx effect` (additions) (reference: main.rs:11-39, commands/depth.rs:34-72, commands/extract.rs:16-35, commands/search.rs:18-51, commands/index.rs:11-23, commands/intersect.rs:32-70,
// utils/common.rs:17-52).  Flag names, short flags, defaults and groups follow the reference's
// clap derive; usage errors exit 2 like clap, run-time errors print `Error: <msg>` and exit 1.
#include <unistd.h>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

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
    "  seq        Write the sequences of features, or of their parents spliced, from a FASTA file (MI355X engine)\n"
    "  effect     Classify single-base substitutions against the transcripts they hit (MI355X engine)\n"
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

const char *kSeqUsage =
    "Usage: gffx seq [OPTIONS] --input <FILE> --fasta <FILE>\n\nOptions:\n"
    "  -i, --input <FILE>       Input GFF file path\n"
    "  -f, --fasta <FILE>       The genome as plain FASTA (lines of any lengths; a compressed file is refused)\n"
    "  -o, --output <FILE>      Output file (stdout if not provided)\n"
    "  -T, --types <T1,T2,...>  Feature types (column 3) whose lines give the segments [default: exon]\n"
    "  -j, --join               One record per Parent instead of one per line: its segments in order of start, joined\n"
    "      --translate          Amino acids instead of bases: NCBI table 1 from the phase (column 8) of the first segment,\n"
    "                           stops as '*', a codon with a letter outside ACGTU as 'X' (e.g. -j --translate -T CDS)\n"
    "  -w, --width <W>          Sequence characters per line; 0: one line per record [default: 60]\n"
    "  -t, --threads <NUM>      Number of threads for parallel processing [default: 12]\n"
    "  -v, --verbose            Enable verbose output\n"
    "      --device <N>         HIP device to run on [default: 0]\n"
    "      --stats-json <FILE>  Write the run's stage timers and counts as one JSON object\n\n"
    "Output: FASTA.  Without -j one record per line of the types, in file order: '>ID seqid:start-end(strand)' ('.' for a\n"
    "  line without ID).  With -j one record per name in the lines' Parent attributes, in order of first appearance:\n"
    "  '>name seqid:start-end(strand) segments=k'.  A feature on '-' is reverse-complemented (IUPAC codes, case kept).  A record\n"
    "  with a member on a seqid the FASTA file lacks, beyond its sequence's end, or (-j) on another seqid or strand than its\n"
    "  first member is left out (warnings say how many).\n";

const char *kEffectUsage =
    "Usage: gffx effect [OPTIONS] --input <FILE> --fasta <FILE> --variants <FILE>\n\nOptions:\n"
    "  -i, --input <FILE>       Input GFF file path\n"
    "  -f, --fasta <FILE>       The genome as plain FASTA (lines of any lengths; a compressed file is refused)\n"
    "  -V, --variants <FILE>    The variants as plain text, CHROM POS ID REF ALT per line as in VCF ('#' lines are skipped; a\n"
    "                           compressed file is refused).  ALT is split at ','; only single-base alleles are taken\n"
    "  -o, --output <FILE>      Output file (stdout if not provided)\n"
    "      --cds-type <TYPE>    Feature type (column 3) whose lines give a transcript's coding segments [default: CDS]\n"
    "      --exon-type <TYPE>   Feature type whose lines give its exons [default: exon]\n"
    "      --summary <FILE>     Write 'class<TAB>alleles<TAB>pairs' for every class\n"
    "  -t, --threads <NUM>      Number of threads for parallel processing [default: 12]\n"
    "  -v, --verbose            Enable verbose output\n"
    "      --device <N>         HIP device to run on [default: 0]\n"
    "      --stats-json <FILE>  Write the run's stage timers and counts as one JSON object\n\n"
    "Output: one TAB-separated line per allele and transcript whose span contains it, the alleles in file order, an allele's\n"
    "  transcripts in order of first appearance: chrom pos ref alt transcript strand class cds_pos codons aa_pos aa ref_match.\n"
    "  A transcript is a name in the Parent attributes of the CDS and exon lines.  Classes: partial_codon, coding_unknown,\n"
    "  stop_retained, synonymous, stop_gained, stop_lost, start_lost, missense, noncoding_exon, 5_prime_UTR, 3_prime_UTR, intron,\n"
    "  splice_donor, splice_acceptor (the two bases next to an exon) and intergenic (no transcript: one line with '.').  The\n"
    "  codon is read from the genome, never from REF; ref_match says whether REF is the genome's base.  A transcript with a\n"
    "  member on a seqid the FASTA file lacks, beyond its sequence's end, or on another seqid or strand than its first member is\n"
    "  left out (warnings say how many).\n";

// what `gffx effect` prints for help and usage errors once --indels is among its arguments (without it: kEffectUsage, unchanged)
const char *kEffectIndelsUsage =
    "Usage: gffx effect --indels [OPTIONS] --input <FILE> --fasta <FILE> --variants <FILE>\n\nOptions:\n"
    "  -i, --input <FILE>       Input GFF file path\n"
    "  -f, --fasta <FILE>       The genome as plain FASTA (lines of any lengths; a compressed file is refused)\n"
    "  -V, --variants <FILE>    The variants as plain text, CHROM POS ID REF ALT per line as in VCF ('#' lines are skipped; a\n"
    "                           compressed file is refused).  ALT is split at ','\n"
    "      --indels             Take insertions, deletions and multi-base substitutions as well: REF and an ALT piece of 1 to\n"
    "                           65535 bases of ACGTN each\n"
    "  -o, --output <FILE>      Output file (stdout if not provided)\n"
    "      --cds-type <TYPE>    Feature type (column 3) whose lines give a transcript's coding segments [default: CDS]\n"
    "      --exon-type <TYPE>   Feature type whose lines give its exons [default: exon]\n"
    "      --summary <FILE>     Write 'class<TAB>alleles<TAB>pairs' for every class\n"
    "  -t, --threads <NUM>      Number of threads for parallel processing [default: 12]\n"
    "  -v, --verbose            Enable verbose output\n"
    "      --device <N>         HIP device to run on [default: 0]\n"
    "      --stats-json <FILE>  Write the run's stage timers and counts as one JSON object\n\n"
    "Output: one TAB-separated line per allele and transcript whose span it meets, the alleles in file order, an allele's\n"
    "  transcripts in order of first appearance: chrom pos ref alt transcript strand class cds_pos codons aa_pos aa ref_match;\n"
    "  pos, ref and alt are the file's own.  REF and the piece are trimmed (case folded; the common prefix first, then the common\n"
    "  suffix); the genome is not consulted, so nothing is left-aligned.  One base against one base is a single-base substitution\n"
    "  and gets the lines of the command without --indels.  Every other allele covers its reference bases, an insertion the two\n"
    "  bases around it, and takes the first of: unclassified_model (rows of the transcript overlap), transcript_ablation (the\n"
    "  whole span is deleted), splice_donor or splice_acceptor (a deletion meets the two bases next to an exon, an insertion lies\n"
    "  inside them), then in coding sequence partial_codon, start_lost, frameshift, coding_unknown, stop_retained, synonymous,\n"
    "  stop_gained, stop_lost, inframe_insertion, inframe_deletion or missense, then noncoding_exon, 5_prime_UTR or 3_prime_UTR,\n"
    "  then intron; intergenic without a transcript.  For these alleles cds_pos and aa_pos are where the change begins in the\n"
    "  transcribed coding sequence; codons and aa print '.': the residues an in-frame change replaces are not reported.\n"
    "  ref_match says whether the trimmed REF is the genome's.  Left out, each kind under a warning of its own: '*', '.', symbolic\n"
    "  and breakend pieces and any other byte; a REF or piece longer than 65535 bytes; a piece equal to REF; an insertion in front\n"
    "  of a sequence's first base.  --summary has 20 lines.\n";

const char *kIndexUsage =
    "Usage: gffx index [OPTIONS] --input <INPUT>\n\nOptions:\n"
    "  -i, --input <INPUT>\n"
    "  -a, --attribute <ATTRIBUTE>    [default: gene_name]\n"
    "  -s, --skip-types <SKIP_TYPES>  [default: remark,note,comment,region,gap,assembly_gap,contig,scaffold,source]\n"
    "  -v, --verbose\n"
    "  -g, --gpu                      Build the side-cars on the HIP device (same bytes; no CPU fallback)\n"
    "      --device <N>               HIP device of --gpu [default: 0]\n";

// What the scan found on a command's line, with the checks and conversions the commands share.  A `label` is the option as
// the help text prints it ("--threads <NUM>"): the messages quote it.
class Opts {
  public:
    Opts(int argc, char **argv, const std::vector<OptSpec> &specs) : got_(parse_opts(argc, argv, 2, specs)) {}
    bool has(const char *name) const { return got_.count(name) > 0; }
    const std::string &str(const char *name) const { return got_.at(name)[0]; }
    std::optional<std::string> opt(const char *name) const { return has(name) ? std::optional<std::string>(str(name)) : std::nullopt; }
    // a number as the reference's u32 / usize options take it; `fallback` without the option
    size_t size(const char *name, const char *label, size_t fallback) const {
        if (!has(name)) return fallback;
        const auto x = parse_u32_rust(str(name));
        if (!x) throw UsageError("invalid value '" + str(name) + "' for '" + label + "'");
        return *x;
    }
    using Labelled = std::pair<const char *, const char *>;  // {name, label}
    // all of them, or the message that lists the missing ones in this order
    void require(std::initializer_list<Labelled> wanted) const {
        std::string missing;
        for (const auto &[name, label] : wanted)
            if (!has(name)) missing += std::string("\n  ") + label;
        if (!missing.empty()) throw UsageError("the following required arguments were not provided:" + missing);
    }
    void conflict(const Labelled &a, const Labelled &b) const {
        if (has(a.first) && has(b.first)) throw UsageError(std::string("the argument '") + a.second + "' cannot be used with '" + b.second + "'");
    }
    // a required group of two options
    void exactly_one(const char *a, const char *label_a, const char *b, const char *label_b) const {
        conflict({a, label_a}, {b, label_b});
        if (!has(a) && !has(b)) require({{a, (std::string("<") + label_a + "|" + label_b + ">").c_str()}});
    }
    // the place of the option's value among `values`; 0 without the option
    int choice(const char *name, const char *label, std::initializer_list<const char *> values) const {
        if (!has(name)) return 0;
        std::string all;
        int k = 0;
        for (const char *v : values) {
            if (str(name) == v) return k;
            all += (k++ ? ", " : "") + std::string(v);
        }
        throw UsageError("invalid value '" + str(name) + "' for '" + label + "'\n  [possible values: " + all + "]");
    }
    // ---- the blocks every command repeats
    void common(std::string &input, std::optional<std::string> &output, size_t &threads, bool &verbose, const char *threads_label = "--threads <NUM>") const {
        input = str("input");
        output = opt("output");
        threads = size("threads", threads_label, threads);
        verbose = has("verbose");
    }
    void common(CommonArgs &c) const { common(c.input, c.output, c.threads, c.verbose); }
    void group_filters(CommonArgs &c) const {  // -e and -T of intersect, extract and search
        c.entire_group = has("entire_group");
        c.types = opt("types");
    }
    int device() const { return static_cast<int>(size("device", "--device <N>", 0)); }
    int gpus() const { return static_cast<int>(std::max<size_t>(1, std::min<size_t>(64, size("gpus", "--gpus <N>", 1)))); }
    void stats_json() const {
        if (has("stats-json")) g_run_stats.path = str("stats-json");
    }

  private:
    std::map<std::string, std::vector<std::string>> got_;
};

constexpr const char *kInput = "--input <FILE>", *kSource = "--source <SOURCE>", *kRegion = "--region <REGION>", *kBed = "--bed <BED>",
                     *kTypes = "--types <T1,T2,...>";

void run_intersect_cli(const Opts &o) {
    commands::intersect::IntersectArgs a;
    o.require({{"input", kInput}});
    o.common(a.common);
    o.group_filters(a.common);
    o.exactly_one("region", kRegion, "bed", kBed);  // ArgGroup "regions": required, exactly one (intersect.rs:37-39)
    a.region = o.opt("region");
    a.bed = o.opt("bed");
    a.contained = o.has("contained");
    a.contains_region = o.has("contains-region");
    a.overlap = o.has("overlap");
    if (a.contained + a.contains_region + a.overlap > 1)  // ArgGroup "mode" (intersect.rs:40-42)
        throw UsageError("the arguments '--contained', '--contains-region' and '--overlap' cannot be used together");
    a.invert = o.has("invert");
    a.device = o.device();
    a.gpus = o.gpus();
    o.stats_json();
    commands::intersect::run(a);
}

void run_extract_cli(const Opts &o) {
    commands::extract::ExtractArgs a;
    o.require({{"input", kInput}});
    o.common(a.common);
    o.group_filters(a.common);
    // ArgGroup "feature": required, exactly one (extract.rs:21-25); clap names the pair one way round in the conflict and
    // the other way round in the usage
    o.conflict({"feature-id", "--feature-id <FEATURE_ID>"}, {"feature-file", "--feature-file <FEATURE_FILE>"});
    o.exactly_one("feature-file", "--feature-file <FEATURE_FILE>", "feature-id", "--feature-id <FEATURE_ID>");
    a.feature_id = o.opt("feature-id");
    a.feature_file = o.opt("feature-file");
    a.device = o.device();
    o.stats_json();
    commands::extract::run_extract(a);
}

void run_search_cli(const Opts &o) {
    commands::search::SearchArgs a;
    o.require({{"input", kInput}});
    o.common(a.common);
    o.group_filters(a.common);
    o.exactly_one("attr-list", "--attr-list <ATTR_LIST>", "attr", "--attr <ATTR>");  // ArgGroup "attr_input" (search.rs:19-24)
    a.attr_list = o.opt("attr-list");
    a.attr = o.opt("attr");
    a.regex = o.has("regex");
    a.device = o.device();
    o.stats_json();
    commands::search::run_search(a);
}

void run_depth_cli(const Opts &o) {
    commands::depth::DepthArgs a;
    o.require({{"input", kInput}, {"source", kSource}});
    a.source = o.str("source");
    a.bin_shift = static_cast<uint32_t>(o.size("bin-shift", "--bin-shift <BIN_SHIFT>", a.bin_shift));
    o.common(a.input, a.output, a.threads, a.verbose, "--threads <THREADS>");
    a.device = o.device();
    a.gpus = o.gpus();
    o.stats_json();
    commands::depth::run(a);
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

void run_coverage_cli(const Opts &o) {
    commands::coverage::CoverageArgs a;
    o.require({{"input", kInput}, {"source", kSource}});
    a.source = o.str("source");
    o.common(a.input, a.output, a.threads, a.verbose);
    a.device = o.device();
    a.gpus = o.gpus();
    o.stats_json();
    a.mean_depth = o.has("mean-depth");
    if (o.has("thresholds")) a.thresholds = parse_thresholds(o.str("thresholds"));
    a.bedgraph = o.opt("bedgraph");
    commands::coverage::run(a);
}

void run_closest_cli(const Opts &o) {
    commands::closest::ClosestArgs a;
    o.require({{"input", kInput}});
    o.common(a.common);
    o.exactly_one("region", kRegion, "bed", kBed);
    a.region = o.opt("region");
    a.bed = o.opt("bed");
    a.ignore_overlaps = o.has("ignore-overlaps");
    const commands::closest::Side sides[] = {commands::closest::Side::Both, commands::closest::Side::Left, commands::closest::Side::Right};
    a.side = sides[o.choice("side", "--side <SIDE>", {"both", "left", "right"})];
    a.device = o.device();
    o.stats_json();
    commands::closest::run(a);
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

void run_annotate_cli(const Opts &o) {
    commands::annotate::AnnotateArgs a;
    o.require({{"input", kInput}});
    o.common(a.common);
    o.exactly_one("region", kRegion, "bed", kBed);
    a.region = o.opt("region");
    a.bed = o.opt("bed");
    o.require({{"types", kTypes}});
    a.layers = parse_layers(o.str("types"));
    a.summary = o.opt("summary");
    a.device = o.device();
    o.stats_json();
    commands::annotate::run(a);
}

void run_enrich_cli(const Opts &o) {
    commands::enrich::EnrichArgs a;
    o.require({{"input", kInput}, {"bed", kBed}, {"types", kTypes}, {"permutations", "--permutations <N>"}});
    o.common(a.common);
    a.bed = o.str("bed");
    a.layers = parse_layers(o.str("types"));
    const size_t n = o.size("permutations", "--permutations <N>", 0);
    if (n < 1 || n > (1u << 20)) throw UsageError("invalid value '" + o.str("permutations") + "' for '--permutations <N>': 1 to 1048576 are possible");
    a.n_perm = static_cast<uint32_t>(n);
    if (o.has("seed")) {
        const std::string &v = o.str("seed");
        char *end = nullptr;
        errno = 0;
        const unsigned long long s = std::strtoull(v.c_str(), &end, 10);
        if (v.empty() || v[0] < '0' || v[0] > '9' || *end || errno == ERANGE) throw UsageError("invalid value '" + v + "' for '--seed <S>': a number below 2^64 is expected");
        a.seed = s;
    }
    a.genome = o.opt("genome");
    a.perms = o.opt("perms");
    a.device = o.device();
    o.stats_json();
    commands::enrich::run(a);
}

void run_meta_cli(const Opts &o) {
    commands::meta::MetaArgs a;
    o.require({{"input", kInput}, {"source", kSource}});
    a.source = o.str("source");
    o.common(a.common);
    if (o.has("types")) a.types = parse_layers(o.str("types"));
    o.conflict({"anchor", "--anchor <ANCHOR>"}, {"scale", "--scale <M>"});
    gffx_hip_meta_layout &y = a.layout;
    y.anchor = static_cast<uint32_t>(o.choice("anchor", "--anchor <ANCHOR>", {"tss", "tes", "center"}));
    y.up = static_cast<uint32_t>(o.size("upstream", "--upstream <UP>", y.up));
    y.down = static_cast<uint32_t>(o.size("downstream", "--downstream <DOWN>", y.down));
    y.bin = static_cast<uint32_t>(o.size("bin", "--bin <BIN>", y.bin));
    if (o.has("scale")) {
        y.mode = 1;
        y.body_bins = static_cast<uint32_t>(o.size("scale", "--scale <M>", 0));
        if (y.body_bins == 0) throw UsageError("invalid value '0' for '--scale <M>': at least one body column is needed");
    }
    if (y.bin == 0) throw UsageError("invalid value '0' for '--bin <BIN>': a column has at least one base");
    if (y.up % y.bin) throw UsageError("invalid value '" + std::to_string(y.up) + "' for '--upstream <UP>': not a multiple of --bin " + std::to_string(y.bin));
    if (y.down % y.bin) throw UsageError("invalid value '" + std::to_string(y.down) + "' for '--downstream <DOWN>': not a multiple of --bin " + std::to_string(y.bin));
    if (y.mode == 0 && static_cast<uint64_t>(y.up) + y.down == 0) throw UsageError("--upstream and --downstream are both 0: there is no column");
    if (gffx_hip_pileup_meta_columns(&y) > gffx_hip_pileup_meta_max_columns())
        throw UsageError(std::to_string(gffx_hip_pileup_meta_columns(&y)) + " columns exceed the limit of " + std::to_string(gffx_hip_pileup_meta_max_columns()) +
                         ": choose a larger --bin or a smaller --scale");
    a.genome = o.opt("genome");
    a.matrix = o.opt("matrix");
    a.device = o.device();
    a.gpus = o.gpus();
    o.stats_json();
    commands::meta::run(a);
}

void run_seq_cli(const Opts &o) {
    commands::seq::SeqArgs a;
    o.require({{"input", kInput}, {"fasta", "--fasta <FILE>"}});
    o.common(a.common);
    a.fasta = o.str("fasta");
    if (o.has("types")) a.types = parse_layers(o.str("types"));
    a.join = o.has("join");
    a.translate = o.has("translate");
    a.width = static_cast<uint32_t>(o.size("width", "--width <W>", a.width));
    a.device = o.device();
    o.stats_json();
    commands::seq::run(a);
}

void run_effect_cli(const Opts &o) {
    commands::effect::EffectArgs a;
    o.require({{"input", kInput}, {"fasta", "--fasta <FILE>"}, {"variants", "--variants <FILE>"}});
    o.common(a.common);
    a.fasta = o.str("fasta");
    a.variants = o.str("variants");
    if (o.has("cds-type")) a.cds_type = o.str("cds-type");
    if (o.has("exon-type")) a.exon_type = o.str("exon-type");
    if (a.cds_type.empty() || a.exon_type.empty()) throw UsageError("'--cds-type <TYPE>' and '--exon-type <TYPE>' take a type name");
    if (a.cds_type == a.exon_type) throw UsageError("the argument '--cds-type <TYPE>' names the type of '--exon-type <TYPE>': '" + a.cds_type + "'");
    a.summary = o.opt("summary");
    a.indels = o.has("indels");
    a.device = o.device();
    o.stats_json();
    commands::effect::run(a);
}

void run_index_cli(const Opts &o) {
    o.require({{"input", "--input <INPUT>"}});
    const std::string &input = o.str("input");
    const std::string attr = o.has("attribute") ? o.str("attribute") : "gene_name";  // commands/index.rs:15
    const std::string skip = o.has("skip-types") ? o.str("skip-types") : "remark,note,comment,region,gap,assembly_gap,contig,scaffold,source";  // :18
    const bool verbose = o.has("verbose");
    if (verbose) std::printf("Indexing: %s\n", input.c_str());  // commands/index.rs:26-28
    // addition: --gpu builds the same eight files from arrays made on the device (GFFX_INDEX_CHUNK_BYTES: the text per pass);
    // --device is read with it only
    if (o.has("gpu"))
        build_index_device(input, attr, skip, o.device(), verbose);
    else
        build_index(input, attr, skip, verbose);
    write_line_images(input, verbose);
    if (verbose) std::printf("Index created successfully.\n");
}

// The subcommands in the order of the top-level help; every one also takes -h / --help.
struct Command {
    const char *name, *usage;
    void (*run)(const Opts &);
    std::vector<OptSpec> specs;
};
const std::vector<Command> &commands_table() {
    static const std::vector<Command> table = {
        {"index", kIndexUsage, run_index_cli,
         {{'i', "input", true}, {'a', "attribute", true}, {'s', "skip-types", true}, {'v', "verbose", false}, {'g', "gpu", false}, {0, "device", true}}},
        {"intersect", kIntersectUsage, run_intersect_cli,
         {{'i', "input", true}, {'o', "output", true}, {'e', "entire_group", false}, {'T', "types", true}, {'t', "threads", true}, {'v', "verbose", false},
          {'r', "region", true}, {'b', "bed", true}, {'c', "contained", false}, {'C', "contains-region", false}, {'O', "overlap", false}, {'I', "invert", false},
          {0, "device", true}, {0, "gpus", true}, {0, "stats-json", true}}},
        {"extract", kExtractUsage, run_extract_cli,
         {{'i', "input", true}, {'o', "output", true}, {'e', "entire_group", false}, {'T', "types", true}, {'t', "threads", true}, {'v', "verbose", false},
          {'f', "feature-id", true}, {'F', "feature-file", true}, {0, "device", true}, {0, "stats-json", true}}},
        {"search", kSearchUsage, run_search_cli,
         {{'i', "input", true}, {'o', "output", true}, {'e', "entire_group", false}, {'T', "types", true}, {'t', "threads", true}, {'v', "verbose", false},
          {'A', "attr-list", true}, {'a', "attr", true}, {'r', "regex", false}, {0, "device", true}, {0, "stats-json", true}}},
        {"depth", kDepthUsage, run_depth_cli,
         {{'i', "input", true}, {'s', "source", true}, {'o', "output", true}, {0, "bin-shift", true}, {'t', "threads", true}, {'v', "verbose", false},
          {0, "device", true}, {0, "gpus", true}, {0, "stats-json", true}}},
        {"coverage", kCoverageUsage, run_coverage_cli,
         {{'i', "input", true}, {'s', "source", true}, {'o', "output", true}, {'t', "threads", true}, {'v', "verbose", false}, {0, "device", true},
          {0, "gpus", true}, {0, "stats-json", true}, {0, "mean-depth", false}, {0, "thresholds", true}, {0, "bedgraph", true}}},
        {"closest", kClosestUsage, run_closest_cli,
         {{'i', "input", true}, {'o', "output", true}, {'r', "region", true}, {'b', "bed", true}, {0, "ignore-overlaps", false}, {0, "side", true},
          {'t', "threads", true}, {'v', "verbose", false}, {0, "device", true}, {0, "stats-json", true}}},
        {"annotate", kAnnotateUsage, run_annotate_cli,
         {{'i', "input", true}, {'o', "output", true}, {'r', "region", true}, {'b', "bed", true}, {'T', "types", true}, {0, "summary", true},
          {'t', "threads", true}, {'v', "verbose", false}, {0, "device", true}, {0, "stats-json", true}}},
        {"enrich", kEnrichUsage, run_enrich_cli,
         {{'i', "input", true}, {'o', "output", true}, {'b', "bed", true}, {'T', "types", true}, {'n', "permutations", true}, {0, "seed", true},
          {'g', "genome", true}, {0, "perms", true}, {'t', "threads", true}, {'v', "verbose", false}, {0, "device", true}, {0, "stats-json", true}}},
        {"meta", kMetaUsage, run_meta_cli,
         {{'i', "input", true}, {'s', "source", true}, {'o', "output", true}, {'T', "types", true}, {0, "anchor", true}, {0, "scale", true},
          {'u', "upstream", true}, {'d', "downstream", true}, {'w', "bin", true}, {'g', "genome", true}, {0, "matrix", true}, {'t', "threads", true},
          {'v', "verbose", false}, {0, "device", true}, {0, "gpus", true}, {0, "stats-json", true}}},
        {"seq", kSeqUsage, run_seq_cli,
         {{'i', "input", true}, {'f', "fasta", true}, {'o', "output", true}, {'T', "types", true}, {'j', "join", false}, {0, "translate", false},
          {'w', "width", true}, {'t', "threads", true}, {'v', "verbose", false}, {0, "device", true}, {0, "stats-json", true}}},
        {"effect", kEffectUsage, run_effect_cli,
         {{'i', "input", true}, {'f', "fasta", true}, {'V', "variants", true}, {'o', "output", true}, {0, "cds-type", true}, {0, "exon-type", true},
          {0, "summary", true}, {0, "indels", false}, {'t', "threads", true}, {'v', "verbose", false}, {0, "device", true}, {0, "stats-json", true}}},
    };
    return table;
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
        for (const Command &c : commands_table()) {
            if (cmd != c.name) continue;
            usage = c.usage;
            if (cmd == "effect")
                for (int k = 2; k < argc && std::strcmp(argv[k], "--") != 0; ++k)
                    if (std::strcmp(argv[k], "--indels") == 0) usage = kEffectIndelsUsage;
            std::vector<OptSpec> specs = c.specs;
            specs.push_back({'h', "help", false});
            const Opts o(argc, argv, specs);
            if (o.has("help"))
                std::fputs(usage, stdout);
            else
                c.run(o);
            return 0;
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
