"""The command line's usage errors, byte for byte: for each of the ten subcommands the exit status (2) and the whole of
stderr -- `error: <msg>`, a blank line, the subcommand's help text, the closing hint.  The messages are written out here;
the help text is what `gffx <cmd> --help` prints.  Usage errors are raised before any file or device is opened, so the
paths given are never touched and no GPU is needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")

COMMANDS = ["index", "intersect", "extract", "search", "depth", "coverage", "closest", "annotate", "enrich", "meta"]
# arguments that pass the command line's checks (the files are never opened before them)
VALID = {
    "index": ["-i", "x.gff"],
    "intersect": ["-i", "x.gff", "-r", "chr1:1-2"],
    "extract": ["-i", "x.gff", "-f", "gene1"],
    "search": ["-i", "x.gff", "-a", "abc"],
    "depth": ["-i", "x.gff", "-s", "y.bed"],
    "coverage": ["-i", "x.gff", "-s", "y.bed"],
    "closest": ["-i", "x.gff", "-r", "chr1:1-2"],
    "annotate": ["-i", "x.gff", "-r", "chr1:1-2", "-T", "gene"],
    "enrich": ["-i", "x.gff", "-b", "y.bed", "-T", "gene", "-n", "5"],
    "meta": ["-i", "x.gff", "-s", "y.bed"],
}
MISSING = "the following required arguments were not provided:"
REGION_GROUP = "<--region <REGION>|--bed <BED>>"
FEATURE_GROUP = "<--feature-file <FEATURE_FILE>|--feature-id <FEATURE_ID>>"
ATTR_GROUP = "<--attr-list <ATTR_LIST>|--attr <ATTR>>"

_help_cache = {}


def _help(cmd):
    """stdout of `gffx <cmd> --help` (of `gffx --help` for cmd None)"""
    if cmd not in _help_cache:
        r = subprocess.run([GFFX, "--help"] if cmd is None else [GFFX, cmd, "--help"], capture_output=True)
        assert r.returncode == 0 and r.stderr == b"" and r.stdout.startswith(b"Usage: gffx ")
        _help_cache[cmd] = r.stdout
    return _help_cache[cmd]


def _usage_error(cmd, args, msg):
    r = subprocess.run([GFFX] + ([] if cmd is None else [cmd]) + list(args), capture_output=True)
    want = b"error: " + msg.encode() + b"\n\n" + _help(cmd) + b"\nFor more information, try '--help'.\n"
    assert (r.returncode, r.stdout, r.stderr) == (2, b"", want), (cmd, args)


def _without(args, *flags):
    """args without the given flags and their values"""
    out, skip = [], False
    for a in args:
        if skip:
            skip = False
        elif a in flags:
            skip = True
        else:
            out.append(a)
    return out


# ---- required options: one at a time, then all at once (the order of the list) ------------------------------------------
REQUIRED = [
    ("index", [], MISSING + "\n  --input <INPUT>"),
    ("intersect", ["-r", "chr1:1-2"], MISSING + "\n  --input <FILE>"),
    ("intersect", ["-i", "x.gff"], MISSING + "\n  " + REGION_GROUP),
    ("intersect", [], MISSING + "\n  --input <FILE>"),
    ("extract", ["-f", "gene1"], MISSING + "\n  --input <FILE>"),
    ("extract", ["-i", "x.gff"], MISSING + "\n  " + FEATURE_GROUP),
    ("extract", [], MISSING + "\n  --input <FILE>"),
    ("search", ["-a", "abc"], MISSING + "\n  --input <FILE>"),
    ("search", ["-i", "x.gff"], MISSING + "\n  " + ATTR_GROUP),
    ("search", [], MISSING + "\n  --input <FILE>"),
    ("depth", ["-s", "y.bed"], MISSING + "\n  --input <FILE>"),
    ("depth", ["-i", "x.gff"], MISSING + "\n  --source <SOURCE>"),
    ("depth", [], MISSING + "\n  --input <FILE>\n  --source <SOURCE>"),
    ("coverage", ["-s", "y.bed"], MISSING + "\n  --input <FILE>"),
    ("coverage", ["-i", "x.gff"], MISSING + "\n  --source <SOURCE>"),
    ("coverage", [], MISSING + "\n  --input <FILE>\n  --source <SOURCE>"),
    ("closest", ["-r", "chr1:1-2"], MISSING + "\n  --input <FILE>"),
    ("closest", ["-i", "x.gff"], MISSING + "\n  " + REGION_GROUP),
    ("closest", [], MISSING + "\n  --input <FILE>"),
    ("annotate", ["-r", "chr1:1-2", "-T", "gene"], MISSING + "\n  --input <FILE>"),
    ("annotate", ["-i", "x.gff", "-T", "gene"], MISSING + "\n  " + REGION_GROUP),
    ("annotate", ["-i", "x.gff", "-r", "chr1:1-2"], MISSING + "\n  --types <T1,T2,...>"),
    ("annotate", ["-i", "x.gff"], MISSING + "\n  " + REGION_GROUP),
    ("annotate", [], MISSING + "\n  --input <FILE>"),
    ("enrich", ["-b", "y.bed", "-T", "gene", "-n", "5"], MISSING + "\n  --input <FILE>"),
    ("enrich", ["-i", "x.gff", "-T", "gene", "-n", "5"], MISSING + "\n  --bed <BED>"),
    ("enrich", ["-i", "x.gff", "-b", "y.bed", "-n", "5"], MISSING + "\n  --types <T1,T2,...>"),
    ("enrich", ["-i", "x.gff", "-b", "y.bed", "-T", "gene"], MISSING + "\n  --permutations <N>"),
    ("enrich", ["-T", "gene"], MISSING + "\n  --input <FILE>\n  --bed <BED>\n  --permutations <N>"),
    ("enrich", [], MISSING + "\n  --input <FILE>\n  --bed <BED>\n  --types <T1,T2,...>\n  --permutations <N>"),
    ("meta", ["-s", "y.bed"], MISSING + "\n  --input <FILE>"),
    ("meta", ["-i", "x.gff"], MISSING + "\n  --source <SOURCE>"),
    ("meta", [], MISSING + "\n  --input <FILE>\n  --source <SOURCE>"),
]


@pytest.mark.parametrize("cmd,args,msg", REQUIRED, ids=lambda v: v if isinstance(v, str) and "\n" not in v else None)
def test_required_options(cmd, args, msg):
    _usage_error(cmd, args, msg)


# ---- exclusive groups: both members -------------------------------------------------------------------------------------
EXCLUSIVE = [
    ("intersect", ["-i", "x.gff", "-r", "chr1:1-2", "-b", "y.bed"], "the argument '--region <REGION>' cannot be used with '--bed <BED>'"),
    ("closest", ["-i", "x.gff", "-r", "chr1:1-2", "-b", "y.bed"], "the argument '--region <REGION>' cannot be used with '--bed <BED>'"),
    ("annotate", ["-i", "x.gff", "-T", "gene", "-b", "y.bed", "-r", "chr1:1-2"], "the argument '--region <REGION>' cannot be used with '--bed <BED>'"),
    ("extract", ["-i", "x.gff", "-F", "ids.txt", "-f", "gene1"],
     "the argument '--feature-id <FEATURE_ID>' cannot be used with '--feature-file <FEATURE_FILE>'"),
    ("search", ["-i", "x.gff", "-a", "abc", "-A", "list.txt"], "the argument '--attr-list <ATTR_LIST>' cannot be used with '--attr <ATTR>'"),
    ("meta", ["-i", "x.gff", "-s", "y.bed", "--anchor", "tes", "--scale", "5"], "the argument '--anchor <ANCHOR>' cannot be used with '--scale <M>'"),
    ("intersect", ["-i", "x.gff", "-r", "chr1:1-2", "-c", "-C"], "the arguments '--contained', '--contains-region' and '--overlap' cannot be used together"),
    ("intersect", ["-i", "x.gff", "-r", "chr1:1-2", "-O", "-c"], "the arguments '--contained', '--contains-region' and '--overlap' cannot be used together"),
]


@pytest.mark.parametrize("cmd,args,msg", EXCLUSIVE)
def test_exclusive_groups(cmd, args, msg):
    _usage_error(cmd, args, msg)


# ---- what the scan of the line itself refuses, the same for every command -----------------------------------------------
@pytest.mark.parametrize("cmd", COMMANDS)
def test_scan_errors(cmd):
    ok = VALID[cmd]
    _usage_error(cmd, ok + ["--bogus"], "unexpected argument '--bogus' found")
    _usage_error(cmd, ok + ["--bogus=1"], "unexpected argument '--bogus' found")
    _usage_error(cmd, ok + ["-Z"], "unexpected argument '-Z' found")
    _usage_error(cmd, ["-vZ"] + ok, "unexpected argument '-Z' found")
    _usage_error(cmd, ok + ["stray"], "unexpected argument 'stray' found")
    _usage_error(cmd, ok + ["--"], "unexpected argument '--' found")
    _usage_error(cmd, _without(ok, "-i") + ["--input"], "a value is required for '--input' but none was supplied")
    _usage_error(cmd, _without(ok, "-i") + ["-i"], "a value is required for '-i' but none was supplied")
    _usage_error(cmd, _without(ok, "-i") + ["-vi"], "a value is required for '-i' but none was supplied")
    _usage_error(cmd, ok + ["--verbose=1"], "unexpected value for '--verbose'")
    _usage_error(cmd, ok + ["-i", "z.gff"], "the argument '--input' cannot be used multiple times")
    _usage_error(cmd, ok + ["--input=z.gff"], "the argument '--input' cannot be used multiple times")
    _usage_error(cmd, ok + ["-v", "--verbose"], "the argument '--verbose' cannot be used multiple times")
    _usage_error(cmd, ok + ["-vv"], "the argument '--verbose' cannot be used multiple times")


# ---- numbers ------------------------------------------------------------------------------------------------------------
THREADS_LABEL = {c: "--threads <NUM>" for c in COMMANDS if c != "index"}
THREADS_LABEL["depth"] = "--threads <THREADS>"


@pytest.mark.parametrize("cmd", sorted(THREADS_LABEL))
def test_threads_must_be_a_number(cmd):
    for bad in ("x", "-1", "", "4294967296", "1.5"):
        _usage_error(cmd, VALID[cmd] + ["--threads", bad], "invalid value '%s' for '%s'" % (bad, THREADS_LABEL[cmd]))
    _usage_error(cmd, VALID[cmd] + ["-tx"], "invalid value 'x' for '%s'" % THREADS_LABEL[cmd])


@pytest.mark.parametrize("cmd", COMMANDS)
def test_device_must_be_a_number(cmd):
    ok = VALID[cmd] + (["--gpu"] if cmd == "index" else [])  # (index reads --device only with --gpu, below)
    for bad in ("x", "-1", ""):
        _usage_error(cmd, ok + ["--device", bad], "invalid value '%s' for '--device <N>'" % bad)
    _usage_error(cmd, ok + ["--device=x"], "invalid value 'x' for '--device <N>'")


@pytest.mark.parametrize("cmd", ["intersect", "depth", "coverage", "meta"])
def test_gpus_must_be_a_number(cmd):
    for bad in ("x", "-1", ""):
        _usage_error(cmd, VALID[cmd] + ["--gpus", bad], "invalid value '%s' for '--gpus <N>'" % bad)


def test_commands_without_gpus_refuse_the_option():
    for cmd in ("index", "extract", "search", "closest", "annotate", "enrich"):
        _usage_error(cmd, VALID[cmd] + ["--gpus", "2"], "unexpected argument '--gpus' found")


def test_index_reads_device_only_with_gpu(tmp_path):
    r = subprocess.run([GFFX, "index", "-i", str(tmp_path / "missing.gff"), "--device", "x"], capture_output=True)
    assert r.returncode == 1 and r.stderr.startswith(b"Error: ") and r.stdout == b""


def test_more_numbers():
    _usage_error("depth", VALID["depth"] + ["--bin-shift", "x"], "invalid value 'x' for '--bin-shift <BIN_SHIFT>'")
    for flag, label in (("--upstream", "--upstream <UP>"), ("--downstream", "--downstream <DOWN>"), ("--bin", "--bin <BIN>"), ("--scale", "--scale <M>")):
        _usage_error("meta", VALID["meta"] + [flag, "x"], "invalid value 'x' for '%s'" % label)
    _usage_error("enrich", _without(VALID["enrich"], "-n") + ["-n", "x"], "invalid value 'x' for '--permutations <N>'")


# ---- particular commands ------------------------------------------------------------------------------------------------
def test_choices():
    _usage_error("closest", VALID["closest"] + ["--side", "x"], "invalid value 'x' for '--side <SIDE>'\n  [possible values: both, left, right]")
    _usage_error("closest", VALID["closest"] + ["--side", "Left"], "invalid value 'Left' for '--side <SIDE>'\n  [possible values: both, left, right]")
    _usage_error("meta", VALID["meta"] + ["--anchor", "x"], "invalid value 'x' for '--anchor <ANCHOR>'\n  [possible values: tss, tes, center]")


def test_meta_layout():
    ok = VALID["meta"]
    _usage_error("meta", ok + ["--scale", "0"], "invalid value '0' for '--scale <M>': at least one body column is needed")
    _usage_error("meta", ok + ["--bin", "0"], "invalid value '0' for '--bin <BIN>': a column has at least one base")
    _usage_error("meta", ok + ["-u", "15", "-w", "10"], "invalid value '15' for '--upstream <UP>': not a multiple of --bin 10")
    _usage_error("meta", ok + ["-d", "15", "-w", "10"], "invalid value '15' for '--downstream <DOWN>': not a multiple of --bin 10")
    _usage_error("meta", ok + ["-u", "0", "-d", "0"], "--upstream and --downstream are both 0: there is no column")
    # 4000 / 1 + 97 = 4097 columns, one over; the same line with -d 96 passes the command line (and fails later, on the files)
    _usage_error("meta", ok + ["-u", "4000", "-d", "97", "-w", "1"], "4097 columns exceed the limit of 4096: choose a larger --bin or a smaller --scale")
    _usage_error("meta", ok + ["--scale", "4000000000"], "4000000400 columns exceed the limit of 4096: choose a larger --bin or a smaller --scale")
    r = subprocess.run([GFFX, "meta", "-i", "/nonexistent/x.gff", "-s", "y.bed", "-u", "4000", "-d", "96", "-w", "1"], capture_output=True)
    assert r.returncode == 1 and r.stderr.startswith(b"Error: ")


def test_enrich_numbers():
    base = _without(VALID["enrich"], "-n")
    _usage_error("enrich", base + ["-n", "0"], "invalid value '0' for '--permutations <N>': 1 to 1048576 are possible")
    _usage_error("enrich", base + ["-n", "1048577"], "invalid value '1048577' for '--permutations <N>': 1 to 1048576 are possible")
    for bad in ("x", "-1", "", " 7", "7x", "18446744073709551616"):
        _usage_error("enrich", VALID["enrich"] + ["--seed", bad], "invalid value '%s' for '--seed <S>': a number below 2^64 is expected" % bad)


@pytest.mark.parametrize("cmd", ["annotate", "enrich", "meta"])
def test_type_lists(cmd):
    base = _without(VALID[cmd], "-T")
    label = "'--types <T1,T2,...>'"
    _usage_error(cmd, base + ["-T", "a,,b"], "invalid value 'a,,b' for %s: an empty type name" % label)
    _usage_error(cmd, base + ["-T", ""], "invalid value '' for %s: an empty type name" % label)
    _usage_error(cmd, base + ["-T", "a,"], "invalid value 'a,' for %s: an empty type name" % label)
    _usage_error(cmd, base + ["-T", "a,a"], "invalid value 'a,a' for %s: 'a' is given twice" % label)
    names = ",".join("t%d" % i for i in range(33))
    _usage_error(cmd, base + ["-T", names], "invalid value '%s' for %s: more than 32 types" % (names, label))


def test_top_level():
    _usage_error(None, [], "a subcommand is required")
    _usage_error(None, ["frobnicate"], "unrecognized subcommand 'frobnicate' (this build carries the intersect, extract, search, depth, coverage, "
                 "closest, annotate, enrich and meta paths only)")
    _usage_error(None, ["--bogus"], "unrecognized subcommand '--bogus' (this build carries the intersect, extract, search, depth, coverage, "
                 "closest, annotate, enrich and meta paths only)")
    top = _help(None)
    for word in ("help", "--help", "-h"):
        r = subprocess.run([GFFX, word], capture_output=True)
        assert (r.returncode, r.stdout, r.stderr) == (0, top, b"")
    for cmd in COMMANDS:
        assert (b"\n  %-10s " % cmd.encode()) in top
        assert _help(cmd).startswith(b"Usage: gffx " + cmd.encode() + b" ")
        r = subprocess.run([GFFX, cmd, "-h"], capture_output=True)
        assert (r.returncode, r.stdout, r.stderr) == (0, _help(cmd), b"")
        # --help wins over everything the checks after the scan would refuse, not over the scan itself
        r = subprocess.run([GFFX, cmd, "--threads" if cmd != "index" else "--device", "x", "--help"], capture_output=True)
        assert (r.returncode, r.stdout, r.stderr) == (0, _help(cmd), b"")
        _usage_error(cmd, ["--help", "--bogus"], "unexpected argument '--bogus' found")


# ---- two mistakes on one line: which one is reported ---------------------------------------------------------------------
TWO_MISTAKES = [
    ("index", ["--bogus"], "unexpected argument '--bogus' found"),                                       # scan before required
    ("intersect", ["-r", "chr1:1-2", "-b", "y.bed"], MISSING + "\n  --input <FILE>"),                  # required before the group
    ("intersect", ["-i", "x.gff", "-t", "x", "-c", "-C"], "invalid value 'x' for '--threads <NUM>'"),  # threads before the groups
    ("intersect", ["-i", "x.gff", "-r", "chr1:1-2", "-c", "-C", "--device", "x"],
     "the arguments '--contained', '--contains-region' and '--overlap' cannot be used together"),
    ("intersect", ["-i", "x.gff", "-r", "chr1:1-2", "--gpus", "x", "--device", "y"], "invalid value 'y' for '--device <N>'"),
    ("extract", ["-i", "x.gff", "-f", "a", "-F", "b", "--device", "x"],
     "the argument '--feature-id <FEATURE_ID>' cannot be used with '--feature-file <FEATURE_FILE>'"),
    ("extract", ["-i", "x.gff", "-t", "x"], "invalid value 'x' for '--threads <NUM>'"),
    ("search", ["-i", "x.gff", "-a", "a", "-A", "b", "--device", "x"], "the argument '--attr-list <ATTR_LIST>' cannot be used with '--attr <ATTR>'"),
    ("search", ["-i", "x.gff", "-t", "x"], "invalid value 'x' for '--threads <NUM>'"),
    ("depth", ["-i", "x.gff", "--threads", "x"], MISSING + "\n  --source <SOURCE>"),
    ("depth", VALID["depth"] + ["--device", "x", "--threads", "y", "--bin-shift", "z"], "invalid value 'z' for '--bin-shift <BIN_SHIFT>'"),
    ("depth", VALID["depth"] + ["--device", "x", "--threads", "y"], "invalid value 'y' for '--threads <THREADS>'"),
    ("depth", VALID["depth"] + ["--gpus", "x", "--device", "y"], "invalid value 'y' for '--device <N>'"),
    ("coverage", VALID["coverage"] + ["--gpus", "x", "--device", "y"], "invalid value 'y' for '--device <N>'"),
    ("coverage", VALID["coverage"] + ["--thresholds", "0", "--gpus", "x"], "invalid value 'x' for '--gpus <N>'"),
    ("closest", ["-i", "x.gff", "--side", "x"], MISSING + "\n  " + REGION_GROUP),
    ("closest", ["-i", "x.gff", "-t", "x"], "invalid value 'x' for '--threads <NUM>'"),
    ("closest", VALID["closest"] + ["--device", "x", "--side", "y"], "invalid value 'y' for '--side <SIDE>'\n  [possible values: both, left, right]"),
    ("annotate", ["-i", "x.gff", "-T", "a,,b"], MISSING + "\n  " + REGION_GROUP),
    ("annotate", ["-i", "x.gff", "-r", "chr1:1-2", "-T", "a,,b", "--device", "x"], "invalid value 'a,,b' for '--types <T1,T2,...>': an empty type name"),
    ("annotate", ["-i", "x.gff", "-t", "x"], "invalid value 'x' for '--threads <NUM>'"),
    ("enrich", ["-i", "x.gff", "-b", "y.bed", "-T", "a,a", "-n", "0"], "invalid value 'a,a' for '--types <T1,T2,...>': 'a' is given twice"),
    ("enrich", ["-i", "x.gff", "-b", "y.bed", "-T", "a", "-n", "0", "-t", "x"], "invalid value 'x' for '--threads <NUM>'"),
    ("enrich", ["-i", "x.gff", "-b", "y.bed", "-T", "a", "-n", "0", "--seed", "x"], "invalid value '0' for '--permutations <N>': 1 to 1048576 are possible"),
    ("enrich", VALID["enrich"] + ["--device", "x", "--seed", "y"], "invalid value 'y' for '--seed <S>': a number below 2^64 is expected"),
    ("meta", VALID["meta"] + ["--anchor", "x", "--scale", "0"], "the argument '--anchor <ANCHOR>' cannot be used with '--scale <M>'"),
    ("meta", VALID["meta"] + ["-T", "a,,b", "--threads", "x"], "invalid value 'x' for '--threads <NUM>'"),
    ("meta", VALID["meta"] + ["-T", "a,,b", "--anchor", "x"], "invalid value 'a,,b' for '--types <T1,T2,...>': an empty type name"),
    ("meta", VALID["meta"] + ["--anchor", "x", "-u", "y"], "invalid value 'x' for '--anchor <ANCHOR>'\n  [possible values: tss, tes, center]"),
    ("meta", VALID["meta"] + ["-u", "x", "-d", "y", "-w", "z"], "invalid value 'x' for '--upstream <UP>'"),
    ("meta", VALID["meta"] + ["-d", "y", "-w", "z"], "invalid value 'y' for '--downstream <DOWN>'"),
    ("meta", VALID["meta"] + ["-w", "z", "--scale", "0"], "invalid value 'z' for '--bin <BIN>'"),
    ("meta", VALID["meta"] + ["-w", "0", "--scale", "0"], "invalid value '0' for '--scale <M>': at least one body column is needed"),
    ("meta", VALID["meta"] + ["-w", "0", "-u", "0", "-d", "0"], "invalid value '0' for '--bin <BIN>': a column has at least one base"),
    ("meta", VALID["meta"] + ["-w", "10", "-u", "15", "-d", "15"], "invalid value '15' for '--upstream <UP>': not a multiple of --bin 10"),
    ("meta", VALID["meta"] + ["-u", "0", "-d", "0", "--device", "x"], "--upstream and --downstream are both 0: there is no column"),
    ("meta", VALID["meta"] + ["--scale", "5000", "--device", "x"], "5400 columns exceed the limit of 4096: choose a larger --bin or a smaller --scale"),
    ("meta", VALID["meta"] + ["--gpus", "x", "--device", "y"], "invalid value 'y' for '--device <N>'"),
]


@pytest.mark.parametrize("cmd,args,msg", TWO_MISTAKES)
def test_which_of_two_mistakes_is_reported(cmd, args, msg):
    _usage_error(cmd, args, msg)


# ---- coverage --thresholds: a run-time error (`Error:`, exit 1), raised before any file is opened ------------------------
@pytest.mark.parametrize("value,tail", [
    ("0", "'0' is not an integer in 1 .. 4294967295"),
    ("x", "'x' is not an integer in 1 .. 4294967295"),
    ("1,,2", "'' is not an integer in 1 .. 4294967295"),
    ("4294967296", "'4294967296' is not an integer in 1 .. 4294967295"),
    ("1,1", "1 is given twice"),
    ("1,2,3,4,5,6,7,8,9", "more than eight thresholds"),
])
def test_coverage_thresholds_errors(value, tail):
    r = subprocess.run([GFFX, "coverage"] + VALID["coverage"] + ["--thresholds", value], capture_output=True)
    want = b"Error: invalid value '" + value.encode() + b"' for '--thresholds <T1,T2,...>': " + tail.encode() + b"\n"
    assert (r.returncode, r.stdout, r.stderr) == (1, b"", want)
