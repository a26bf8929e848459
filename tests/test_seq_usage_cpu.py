"""`gffx seq` on the command line, byte for byte: its help text, its usage errors (status 2: `error: <msg>`, a blank line, the
help text, the closing hint), its line in the top-level help.  Usage errors are raised before any file or device is opened, so
no GPU is needed; a gzip-compressed FASTA and a missing one are run-time errors (status 1)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
VALID = ["-i", "x.gff", "-f", "genome.fa"]
MISSING = "the following required arguments were not provided:"

HELP = (b"Usage: gffx seq [OPTIONS] --input <FILE> --fasta <FILE>\n\nOptions:\n"
        b"  -i, --input <FILE>       Input GFF file path\n"
        b"  -f, --fasta <FILE>       The genome as plain FASTA (lines of any lengths; a compressed file is refused)\n"
        b"  -o, --output <FILE>      Output file (stdout if not provided)\n"
        b"  -T, --types <T1,T2,...>  Feature types (column 3) whose lines give the segments [default: exon]\n"
        b"  -j, --join               One record per Parent instead of one per line: its segments in order of start, joined\n"
        b"      --translate          Amino acids instead of bases: NCBI table 1 from the phase (column 8) of the first segment,\n"
        b"                           stops as '*', a codon with a letter outside ACGTU as 'X' (e.g. -j --translate -T CDS)\n"
        b"  -w, --width <W>          Sequence characters per line; 0: one line per record [default: 60]\n"
        b"  -t, --threads <NUM>      Number of threads for parallel processing [default: 12]\n"
        b"  -v, --verbose            Enable verbose output\n"
        b"      --device <N>         HIP device to run on [default: 0]\n"
        b"      --stats-json <FILE>  Write the run's stage timers and counts as one JSON object\n\n"
        b"Output: FASTA.  Without -j one record per line of the types, in file order: '>ID seqid:start-end(strand)' ('.' for a\n"
        b"  line without ID).  With -j one record per name in the lines' Parent attributes, in order of first appearance:\n"
        b"  '>name seqid:start-end(strand) segments=k'.  A feature on '-' is reverse-complemented (IUPAC codes, case kept).  A record\n"
        b"  with a member on a seqid the FASTA file lacks, beyond its sequence's end, or (-j) on another seqid or strand than its\n"
        b"  first member is left out (warnings say how many).\n")


def _usage_error(args, msg):
    r = subprocess.run([GFFX, "seq"] + list(args), capture_output=True)
    want = b"error: " + msg.encode() + b"\n\n" + HELP + b"\nFor more information, try '--help'.\n"
    assert (r.returncode, r.stdout, r.stderr) == (2, b"", want), args


def test_the_help_text_and_the_top_level_line():
    for flag in ("--help", "-h"):
        r = subprocess.run([GFFX, "seq", flag], capture_output=True)
        assert (r.returncode, r.stdout, r.stderr) == (0, HELP, b"")
    r = subprocess.run([GFFX, "seq"] + VALID + ["--width", "x", "--help"], capture_output=True)  # --help wins over the checks after the scan
    assert (r.returncode, r.stdout, r.stderr) == (0, HELP, b"")
    top = subprocess.run([GFFX, "help"], capture_output=True)
    assert top.returncode == 0 and b"\n  seq        Write the sequences of features, or of their parents spliced, from a FASTA file (MI355X engine)\n" in top.stdout
    assert top.stdout.index(b"\n  meta ") < top.stdout.index(b"\n  seq ") < top.stdout.index(b"\n  help ")


@pytest.mark.parametrize("args,msg", [
    ([], MISSING + "\n  --input <FILE>\n  --fasta <FILE>"),
    (["-f", "genome.fa"], MISSING + "\n  --input <FILE>"),
    (["-i", "x.gff"], MISSING + "\n  --fasta <FILE>"),
    (VALID + ["-T", "exon,,CDS"], "invalid value 'exon,,CDS' for '--types <T1,T2,...>': an empty type name"),
    (VALID + ["-T", ""], "invalid value '' for '--types <T1,T2,...>': an empty type name"),
    (VALID + ["-T", "exon,CDS,exon"], "invalid value 'exon,CDS,exon' for '--types <T1,T2,...>': 'exon' is given twice"),
    (VALID + ["-T", ",".join("t%d" % i for i in range(33))], "invalid value '" + ",".join("t%d" % i for i in range(33)) + "' for '--types <T1,T2,...>': more than 32 types"),
    (VALID + ["-w", "sixty"], "invalid value 'sixty' for '--width <W>'"),
    (VALID + ["-w", "-1"], "invalid value '-1' for '--width <W>'"),
    (VALID + ["-w", "4294967296"], "invalid value '4294967296' for '--width <W>'"),
    (VALID + ["--width"], "a value is required for '--width' but none was supplied"),
    (VALID + ["-t", "many"], "invalid value 'many' for '--threads <NUM>'"),
    (VALID + ["--device", "x"], "invalid value 'x' for '--device <N>'"),
    (VALID + ["--gpus", "2"], "unexpected argument '--gpus' found"),
    (VALID + ["--join=yes"], "unexpected value for '--join'"),
    (VALID + ["-j", "-j"], "the argument '--join' cannot be used multiple times"),
    (VALID + ["-f", "other.fa"], "the argument '--fasta' cannot be used multiple times"),
    (VALID + ["extra"], "unexpected argument 'extra' found"),
    (VALID + ["-x"], "unexpected argument '-x' found"),
])
def test_usage_errors(args, msg):
    _usage_error(args, msg)


def test_the_limits_pass_the_usage_checks(tmp_path):
    # the run then fails on the missing index, not on the usage
    for ok in (["-w", "0"], ["-w", "4294967295"], ["-jv", "--translate", "-T", "CDS"], ["-T", ",".join("t%d" % i for i in range(32))]):
        r = subprocess.run([GFFX, "seq", "-i", str(tmp_path / "none.gff"), "-f", str(tmp_path / "none.fa")] + ok, capture_output=True)
        assert r.returncode == 1 and r.stderr.startswith(b"Error: ") and r.stdout == b"", r.stderr
