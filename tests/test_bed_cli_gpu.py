"""`gffx intersect -b`, `gffx depth -s` and `gffx coverage -s` with the BED file read on the device: the output bytes, the
`Error:` line and the exit status are those of the host parser on the same text, whether the device route is taken by the knob
(GFFX_BED_DEVICE=1 on q.bed) or by the content (q.bed.gz / q.bed.bgz, bgzip-compressed), for every mode, with --gpus 2 and
with sub-batches of 200 bytes; plain gzip is refused by name; other extensions stay refused; the three device stages are in
--stats-json exactly when the device route ran."""
import gzip
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import _bed_cases as cases
from gffx_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
NAMES = [n for n, _ in synth.SMALL2]
KNOBS = ("GFFX_BED_DEVICE", "GFFX_BED_CHUNK_BYTES", "GFFX_CHUNK_BYTES", "GFFX_CHUNK_MB", "GFFX_DEPTH_BATCH_ROWS", "GFFX_COVERAGE_BATCH_ROWS")
STAGES = ["BED inflate (device)", "BED line scan (device)", "BED rows (device)"]
TIMEOUT = 120


def _bgzip(text, block=700):
    return b"".join(synth.bgzf_member(text[i:i + block]) for i in range(0, len(text), block)) + synth.BGZF_EOF


@pytest.fixture(scope="module")
def inp(tmp_path_factory):
    d = tmp_path_factory.mktemp("bed_cli")
    roots = synth.gencode_like_roots(300, seed=21, chroms=synth.SMALL2)
    gff = str(d / "s.gff")
    synth.write_gff3(gff, roots, seed=21, quirks=True)
    assert subprocess.run([GFFX, "index", "-i", gff], capture_output=True, timeout=TIMEOUT).returncode == 0
    rows = synth.synth_bed(400, seed=22, chroms=synth.SMALL2, width=(20, 40000), edge_frac=0.25, roots=roots)
    lines = [b"%s\t%d\t%d" % (NAMES[c].encode(), s, e) for c, s, e in rows.tolist()]
    table = [ln for ln, i, _ in cases.CASES if i[0] != "error"]  # the hand table's lines that no dialect calls an error
    assert len(table) >= 40
    for k, ln in enumerate(table):
        lines.insert((k * 7) % len(lines), ln)
    text = b"\n".join(lines)  # (the last line without newline)
    files = {}
    for tag, body in (("q", text), ("coord", text + b"\nchr1\t12\tx7\tname\n" + text[:300]), ("utf8", text + b"\nchr1\t1\t2\tn\xffme\n" + text[:300])):
        sub = d / tag
        sub.mkdir()
        open(str(sub / "q.bed"), "wb").write(body)
        for ext in (".gz", ".bgz"):
            open(str(sub / ("q.bed" + ext)), "wb").write(_bgzip(body))
        files[tag] = str(sub / "q.bed")
    return dict(dir=d, gff=gff, **files)


def _run(inp, cmd, source, route, tag, extra=(), knobs=None, stdout=False):
    """One CLI run.  route: host (q.bed), knob (q.bed, GFFX_BED_DEVICE=1), gz / bgz (the compressed twins).  Returns
    (exit status, the Error: lines of stderr, the output bytes or None when there is no output file, stats or None)."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs or {})
    if route == "knob":
        env["GFFX_BED_DEVICE"] = "1"
    path = source + {"host": "", "knob": "", "gz": ".gz", "bgz": ".bgz"}[route]
    out, sj = str(inp["dir"] / (tag + ".out")), str(inp["dir"] / (tag + ".json"))
    for p in (out, sj):
        if os.path.exists(p):
            os.remove(p)
    args = [GFFX, cmd, "-i", inp["gff"], "-b" if cmd == "intersect" else "-s", path, "-t", "4", "--stats-json", sj] + list(extra)
    r = subprocess.run(args + ([] if stdout else ["-o", out]), capture_output=True, env=env, timeout=TIMEOUT)
    errors = [ln for ln in r.stderr.splitlines() if ln.startswith(b"Error:")]
    body = r.stdout if stdout else (open(out, "rb").read() if os.path.exists(out) else None)
    return r.returncode, errors, body, json.load(open(sj)) if os.path.exists(sj) else None


def _all_routes_equal_the_host(inp, cmd, extra, tag, source="q"):
    """host once; then knob and gz, each plain, with --gpus 2 and with 200-byte sub-batches, side by side."""
    base = _run(inp, cmd, inp[source], "host", tag + "_host", extra)
    jobs = [(route, variant) for route in ("knob", "gz") for variant in ("plain", "gpus2", "chunk200")]

    def one(job):
        route, variant = job
        return _run(inp, cmd, inp[source], route, "%s_%s_%s" % (tag, route, variant),
                    list(extra) + (["--gpus", "2"] if variant == "gpus2" else []),
                    {"GFFX_BED_CHUNK_BYTES": "200"} if variant == "chunk200" else None)

    with ThreadPoolExecutor(max_workers=6) as pool:
        results = list(pool.map(one, jobs))
    for job, got in zip(jobs, results):
        assert got[:3] == base[:3], (cmd, extra, job, got[1], base[1])
        assert got[3] is None or [n for n, _ in got[3]["stages_ms"] if n in STAGES] == STAGES, job
    assert base[3] is None or not [n for n, _ in base[3]["stages_ms"] if n.startswith("BED ") and "(device)" in n]
    return base


MODES = [m + i + e + t for m in ("O", "c", "C") for i in ("", "I") for e in ("", "e") for t in ("", "T")]


def _flags(mode):
    return ["-" + mode[0]] + (["-I"] if "I" in mode else []) + (["-e"] if "e" in mode else []) + (["-T", "exon,CDS"] if "T" in mode else [])


@pytest.mark.parametrize("mode", MODES)
def test_intersect_bytes_equal_the_host_path(inp, mode):
    rc, errors, body, stats = _all_routes_equal_the_host(inp, "intersect", _flags(mode), "i_" + mode)
    assert rc == 0 and not errors and body is not None and stats is not None
    if mode in ("O", "Oe", "c"):
        assert len(body) > 0  # (the comparison is not one of empty files)


@pytest.mark.parametrize("cmd", ["depth", "coverage"])
def test_depth_and_coverage_bytes_equal_the_host_path(inp, cmd):
    rc, errors, body, stats = _all_routes_equal_the_host(inp, cmd, [], cmd)
    assert rc == 0 and not errors and body and stats is not None
    assert _run(inp, cmd, inp["q"], "bgz", cmd + "_bgz")[:3] == (rc, errors, body)


@pytest.mark.parametrize("cmd,extra", [("intersect", ["-O", "-e"]), ("intersect", ["-c"]), ("depth", []), ("coverage", [])])
def test_stdout_and_the_bgz_name(inp, cmd, extra):
    base = _run(inp, cmd, inp["q"], "host", "so_host", extra, stdout=True)
    assert base[0] == 0 and base[2]
    for route in ("knob", "gz", "bgz"):
        assert _run(inp, cmd, inp["q"], route, "so_" + route, extra, stdout=True)[:3] == base[:3], (cmd, route)


@pytest.mark.parametrize("source", ["coord", "utf8"])
@pytest.mark.parametrize("cmd,extra", [("intersect", ["-O", "-e"]), ("intersect", ["-c", "-T", "exon,CDS"]), ("depth", []), ("coverage", [])])
def test_a_bad_line_ends_every_route_as_it_ends_the_host_path(inp, cmd, extra, source):
    """The Error: line, the exit status and the state of the output file are the host run's, whatever they are: intersect
    fails on both files, depth and coverage skip the line."""
    rc, errors, body, _ = _all_routes_equal_the_host(inp, cmd, extra, "bad_%s_%s" % (cmd, source), source)
    if cmd == "intersect":
        assert rc == 1 and len(errors) == 1
        assert errors[0] == (b'Error: lexical parse error: invalid BED coordinate in "chr1\t12\tx7\tname"' if source == "coord"
                             else b"Error: invalid utf-8 sequence in BED line")
    else:
        assert rc == 0 and not errors and body


@pytest.mark.parametrize("cmd", ["intersect", "depth", "coverage"])
def test_plain_gzip_is_refused_by_name(inp, cmd):
    d = inp["dir"] / ("plain_gzip_" + cmd)
    d.mkdir()
    path = str(d / "q.bed")
    open(path + ".gz", "wb").write(gzip.compress(open(inp["q"], "rb").read()))
    rc, errors, body, _ = _run(inp, cmd, path, "gz", "gzip_" + cmd, ["-O"] if cmd == "intersect" else [])
    assert rc == 1 and len(errors) == 1 and b"bgzip" in errors[0] and b"not BGZF" in errors[0] and body is None


def test_other_extensions_stay_refused(inp):
    path = str(inp["dir"] / "q.txt")
    open(path, "wb").write(open(inp["q"], "rb").read())
    open(path + ".gz", "wb").write(_bgzip(open(inp["q"], "rb").read()))
    for cmd in ("depth", "coverage"):
        for p in (path, path + ".gz"):
            rc, errors, _, _ = _run(inp, cmd, p, "host", "txt_" + cmd)
            assert rc == 1 and len(errors) == 1 and errors[0].startswith(b"Error: Unsupported file type"), (cmd, p)


@pytest.mark.parametrize("cmd,extra", [("intersect", ["-O", "-e"]), ("depth", []), ("coverage", [])])
def test_stats_json_has_the_device_stages_only_on_the_device_route(inp, cmd, extra):
    for route in ("host", "knob", "gz"):
        rc, _, _, stats = _run(inp, cmd, inp["q"], route, "sj_" + route, extra)
        assert rc == 0
        names = [n for n, _ in stats["stages_ms"]]
        assert [n for n in names if n in STAGES] == (STAGES if route != "host" else []), (cmd, route, names)
        assert ("bed_rows_kept" in stats["counts"]) == (route != "host")
