"""`gffx effect` on the command line, byte for byte: its help text, its usage errors (status 2: `error: <msg>`, a blank line, the
help text, the closing hint), its line in the top-level help.  Usage errors are raised before any file or device is opened; the
errors of the variants file (status 1, `line <n>: <reason>`, n counted over the whole file) and the refusal of a compressed one
come before the first device call, so no GPU is needed for them either."""
import gzip
import os
import subprocess

import pytest

import _effect_definition as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
VALID = ["-i", "x.gff", "-f", "genome.fa", "-V", "calls.vcf"]
MISSING = "the following required arguments were not provided:"

HELP = (b"Usage: gffx effect [OPTIONS] --input <FILE> --fasta <FILE> --variants <FILE>\n\nOptions:\n"
        b"  -i, --input <FILE>       Input GFF file path\n"
        b"  -f, --fasta <FILE>       The genome as plain FASTA (lines of any lengths; a compressed file is refused)\n"
        b"  -V, --variants <FILE>    The variants as plain text, CHROM POS ID REF ALT per line as in VCF ('#' lines are skipped; a\n"
        b"                           compressed file is refused).  ALT is split at ','; only single-base alleles are taken\n"
        b"  -o, --output <FILE>      Output file (stdout if not provided)\n"
        b"      --cds-type <TYPE>    Feature type (column 3) whose lines give a transcript's coding segments [default: CDS]\n"
        b"      --exon-type <TYPE>   Feature type whose lines give its exons [default: exon]\n"
        b"      --summary <FILE>     Write 'class<TAB>alleles<TAB>pairs' for every class\n"
        b"  -t, --threads <NUM>      Number of threads for parallel processing [default: 12]\n"
        b"  -v, --verbose            Enable verbose output\n"
        b"      --device <N>         HIP device to run on [default: 0]\n"
        b"      --stats-json <FILE>  Write the run's stage timers and counts as one JSON object\n\n"
        b"Output: one TAB-separated line per allele and transcript whose span contains it, the alleles in file order, an allele's\n"
        b"  transcripts in order of first appearance: chrom pos ref alt transcript strand class cds_pos codons aa_pos aa ref_match.\n"
        b"  A transcript is a name in the Parent attributes of the CDS and exon lines.  Classes: partial_codon, coding_unknown,\n"
        b"  stop_retained, synonymous, stop_gained, stop_lost, start_lost, missense, noncoding_exon, 5_prime_UTR, 3_prime_UTR, intron,\n"
        b"  splice_donor, splice_acceptor (the two bases next to an exon) and intergenic (no transcript: one line with '.').  The\n"
        b"  codon is read from the genome, never from REF; ref_match says whether REF is the genome's base.  A transcript with a\n"
        b"  member on a seqid the FASTA file lacks, beyond its sequence's end, or on another seqid or strand than its first member is\n"
        b"  left out (warnings say how many).\n")


def _usage_error(args, msg):
    r = subprocess.run([GFFX, "effect"] + list(args), capture_output=True)
    want = b"error: " + msg.encode() + b"\n\n" + HELP + b"\nFor more information, try '--help'.\n"
    assert (r.returncode, r.stdout, r.stderr) == (2, b"", want), args


def test_the_help_text_and_the_top_level_line():
    for flag in ("--help", "-h"):
        r = subprocess.run([GFFX, "effect", flag], capture_output=True)
        assert (r.returncode, r.stdout, r.stderr) == (0, HELP, b"")
    r = subprocess.run([GFFX, "effect"] + VALID + ["--device", "x", "--help"], capture_output=True)  # --help wins over the checks after the scan
    assert (r.returncode, r.stdout, r.stderr) == (0, HELP, b"")
    top = subprocess.run([GFFX, "help"], capture_output=True)
    assert top.returncode == 0 and b"\n  effect     Classify single-base substitutions against the transcripts they hit (MI355X engine)\n" in top.stdout
    assert top.stdout.index(b"\n  seq ") < top.stdout.index(b"\n  effect ") < top.stdout.index(b"\n  help ")
    assert all(c.encode() in HELP for c in D.CLASSES)


@pytest.mark.parametrize("args,msg", [
    ([], MISSING + "\n  --input <FILE>\n  --fasta <FILE>\n  --variants <FILE>"),
    (["-f", "genome.fa", "-V", "calls.vcf"], MISSING + "\n  --input <FILE>"),
    (["-i", "x.gff", "-V", "calls.vcf"], MISSING + "\n  --fasta <FILE>"),
    (["-i", "x.gff", "-f", "genome.fa"], MISSING + "\n  --variants <FILE>"),
    (["-i", "x.gff", "-f", "genome.fa", "-v", "calls.vcf"], "unexpected argument 'calls.vcf' found"),  # -v is --verbose here as everywhere
    (VALID + ["--cds-type", ""], "'--cds-type <TYPE>' and '--exon-type <TYPE>' take a type name"),
    (VALID + ["--exon-type", "CDS"], "the argument '--cds-type <TYPE>' names the type of '--exon-type <TYPE>': 'CDS'"),
    (VALID + ["--cds-type", "exon"], "the argument '--cds-type <TYPE>' names the type of '--exon-type <TYPE>': 'exon'"),
    (VALID + ["--summary"], "a value is required for '--summary' but none was supplied"),
    (VALID + ["-t", "many"], "invalid value 'many' for '--threads <NUM>'"),
    (VALID + ["--device", "x"], "invalid value 'x' for '--device <N>'"),
    (VALID + ["--gpus", "2"], "unexpected argument '--gpus' found"),
    (VALID + ["-V", "other.vcf"], "the argument '--variants' cannot be used multiple times"),
    (VALID + ["extra"], "unexpected argument 'extra' found"),
    (VALID + ["-T", "CDS"], "unexpected argument '-T' found"),
])
def test_usage_errors(args, msg):
    _usage_error(args, msg)


def test_valid_options_pass_the_usage_checks(tmp_path):
    # the run then fails on the missing index, not on the usage
    base = ["-i", str(tmp_path / "none.gff"), "-f", str(tmp_path / "none.fa")]
    for ok in (["-V", "x.vcf", "--cds-type", "cds", "--exon-type", "Exon"], ["-V", "x.vcf", "-v", "--summary", str(tmp_path / "s.tsv")], ["--variants=x.vcf", "-t", "1"]):
        r = subprocess.run([GFFX, "effect"] + base + ok, capture_output=True)
        assert r.returncode == 1 and r.stderr.startswith(b"Error: ") and r.stdout == b"", r.stderr


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    d = tmp_path_factory.mktemp("effect_usage")
    gff, fa = str(d / "h.gff"), str(d / "h.fa")
    open(gff, "wb").write(D.HAND_GFF)
    open(fa, "wb").write(D.HAND_FASTA)
    r = subprocess.run([GFFX, "index", "-i", gff], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return dict(dir=d, gff=gff, fa=fa)


GOOD = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n\nchrA\t5\t.\tA\tC\r\n"


@pytest.mark.parametrize("name,text,line,what", [
    ("four_fields", GOOD + b"chrA\t7\t.\tA\n", 5, b"fewer than 5 TAB-separated fields"),
    ("pos_0", GOOD + b"chrA\t7\t.\tA\tG\nchrA\t0\t.\tA\tG\n", 6, b"POS is not a number in 1 .. 4294967295"),
    ("pos_2_32", b"chrA\t4294967296\t.\tA\tG\n" + GOOD, 1, b"POS is not a number in 1 .. 4294967295"),
    ("pos_1x", GOOD * 3 + b"chrA\t1x\t.\tA\tG", 13, b"POS is not a number in 1 .. 4294967295"),
    ("the_first_of_two", GOOD + b"chrA\t1x\t.\tA\tG\nchrA\t7\n", 5, b"POS is not a number"),
])
def test_the_errors_of_the_variants_file(hand, name, text, line, what):
    path = str(hand["dir"] / (name + ".vcf"))
    open(path, "wb").write(text)
    for threads in ("1", "4"):
        r = subprocess.run([GFFX, "effect", "-i", hand["gff"], "-f", hand["fa"], "-V", path, "-t", threads], capture_output=True, timeout=120)
        assert r.returncode == 1 and r.stdout == b"", r.stderr
        last = r.stderr.rstrip(b"\n").split(b"\n")[-1]
        assert last.startswith(b"Error: variants file " + path.encode() + b", line %d: " % line + what), r.stderr


def test_refused_files(hand):
    d = hand["dir"]
    gz = str(d / "calls.vcf.gz")
    open(gz, "wb").write(gzip.compress(D.HAND_VCF))
    r = subprocess.run([GFFX, "effect", "-i", hand["gff"], "-f", hand["fa"], "-V", gz], capture_output=True, timeout=120)
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.endswith(b"Error: compressed variants file is not read: decompress \"" + gz.encode() + b"\" first\n")
    fgz = str(d / "h.fa.gz")
    open(fgz, "wb").write(gzip.compress(D.HAND_FASTA))
    vcf = str(d / "ok.vcf")
    open(vcf, "wb").write(D.HAND_VCF)
    r = subprocess.run([GFFX, "effect", "-i", hand["gff"], "-f", fgz, "-V", vcf], capture_output=True, timeout=120)
    assert r.returncode == 1 and r.stderr.endswith(b"Error: compressed FASTA is not read: decompress \"" + fgz.encode() + b"\" first\n")
    r = subprocess.run([GFFX, "effect", "-i", hand["gff"], "-f", hand["fa"], "-V", str(d / "missing.vcf")], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"Error: Cannot open variants file" in r.stderr
