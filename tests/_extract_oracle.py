"""TEST INFRASTRUCTURE ONLY -- pure-Python restatement of the reference's `gffx extract` (Baohua-Chen/GFFx v0.4.0, paths
relative to its src/): commands/extract.rs:37-162, index_loader/fts.rs:16-31, index_loader/prt.rs:54-72 and
utils/common.rs:289-465 (write_gff_output_filtered), on top of oracle.gffx_oracle_py.build_index.  It follows the source text
line by line and cites it; the reference cannot be built here, so parity is pinned by hand-derived answers
(tests/test_extract_oracle.py).  Two deliberate differences of the product are restated here too: the names that are not found
keep the order of their first appearance (the reference walks an FxHashSet), and the parent chase ends after n steps on a
cycle that no root closes (the reference never returns).
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence, Tuple

from oracle.gffx_oracle_py import MISSING, _WS, Built, build_index  # noqa: F401

NONE = 0xFFFFFFFF  # u32::MAX: a name that is not found, a fid without a valid root


def fts_index(ids: Sequence) -> Dict:
    """fts.rs:16-22: string -> fid, the lines inserted in order, so the LAST line of a string wins."""
    m = {}
    for i, s in enumerate(ids):
        m[s] = i
    return m


def resolve_root(prt: Sequence[int], start: int) -> int:
    """prt.rs:54-72, bounded: NONE when cur >= n, when a parent is >= n, or (the product's bound) after n steps."""
    n = len(prt)
    cur = start
    for _ in range(n):
        if cur >= n:  # :59-61
            return NONE
        p = prt[cur]  # :62
        if p == cur:  # :64-66
            return cur
        if p >= n:  # :67-69
            return NONE
        cur = p  # :70
    return NONE


def read_feature_file(data: bytes) -> List[str]:
    """extract.rs:61-75: BufRead::lines (cut at "\\n", a "\\r" before it dropped; invalid UTF-8 is an error), trim(), empty
    ones dropped; a set there, the order of first appearance here."""
    out, seen = [], set()
    parts = data.split(b"\n")
    if parts and parts[-1] == b"":
        parts.pop()
    for raw in parts:
        if raw.endswith(b"\r"):
            raw = raw[:-1]
        s = raw.decode("utf-8").strip(_WS)  # UnicodeDecodeError == the run fails
        if s and s not in seen:
            seen.add(s)
            out.append(s)
    return out


def split_types(types: Optional[str]) -> Optional[set]:
    """common.rs:306-311"""
    if types is None:
        return None
    return {t.strip(_WS) for t in types.split(",")} - {""}


def type_ok(line: bytes, allow: Optional[set]) -> bool:
    """common.rs:362-386"""
    if allow is None:
        return True
    parts = line.split(b"\t", 3)
    if len(parts) < 4:
        return False
    try:
        return parts[2].decode("utf-8") in allow
    except UnicodeDecodeError:
        return False


def attr_value(line: bytes, key: bytes = b"ID") -> Optional[bytes]:
    """common.rs:389-409: the attribute field is everything after the eighth TAB; the value follows the first `<key>=` in
    it and ends at the next ';' or at the end of the line."""
    parts = line.split(b"\t", 8)
    if len(parts) < 9:
        return None
    attr = parts[8]
    p = attr.find(key + b"=")
    if p < 0:
        return None
    v = attr[p + len(key) + 1:]
    semi = v.find(b";")
    return v if semi < 0 else v[:semi]


def keeps_line(line: bytes, keep: set, allow: Optional[set], key: bytes = b"ID") -> bool:
    """One line with its line ending (common.rs:418-431): keep = the ID strings of the block's root."""
    if line[:1] == b"#":
        return False
    body = line
    if body.endswith(b"\n"):  # :350-357
        body = body[:-1]
    if body.endswith(b"\r"):
        body = body[:-1]
    if not type_ok(body, allow):
        return False
    v = attr_value(body, key)
    if v is None:
        return False
    try:
        return v.decode("utf-8") in keep
    except UnicodeDecodeError:
        return False


def write_gff_output_filtered(gff: bytes, blocks: Iterable[Tuple[int, int, int]], per_root: Dict[int, set],
                              types: Optional[str], key: bytes = b"ID") -> bytes:
    """common.rs:289-465"""
    allow = split_types(types)
    file_len = len(gff)
    parts = []
    for root, start, end in blocks:
        keep = per_root.get(root)
        if not keep:  # :325-328
            continue
        s, e = start, min(end, file_len)
        if s >= e:  # :330-334
            continue
        out = bytearray()
        pos = s
        while pos < e:  # :342-359, :418-432
            nl = gff.find(b"\n", pos, e)
            nxt = nl + 1 if nl >= 0 else e
            line = gff[pos:nxt]
            if keeps_line(line, keep, allow, key):
                out += line
            pos = nxt
        if out:
            parts.append((start, bytes(out)))
    parts.sort(key=lambda p: p[0])  # :451
    return b"".join(p[1] for p in parts)


def write_gff_output(gff: bytes, blocks: Iterable[Tuple[int, int, int]]) -> bytes:
    """common.rs:188-287"""
    srt = sorted(((s, e) for _r, s, e in blocks if s != MISSING), key=lambda b: b[0])
    merged = []
    if srt:
        cs, ce = srt[0]
        for s, e in srt[1:]:
            if s <= ce:
                ce = max(ce, e)
            else:
                if cs < ce:
                    merged.append((cs, ce))
                cs, ce = s, e
        if cs < ce:
            merged.append((cs, ce))
    return b"".join(gff[s:e] for s, e in merged if s < e and e <= len(gff))


def extract_run(gff: bytes, B: Built, names: Sequence[str], entire_group: bool, types: Optional[str]):
    """extract.rs:37-162 for the deduplicated names (a -f ID as given, or read_feature_file's).  Returns (output bytes,
    the names that were not found, the invalid fids sorted)."""
    idx = fts_index(B.ids)
    fids, missing, seen = [], [], set()
    for nm in names:  # :84-90
        if nm in idx:
            if idx[nm] not in seen:
                seen.add(idx[nm])
                fids.append(idx[nm])
        else:
            missing.append(nm)
    roots_vec = [resolve_root(B.prt, f) for f in fids]  # :97
    invalid = sorted({f for f, r in zip(fids, roots_vec) if r == NONE})  # :100-105
    roots = sorted({r for r in roots_vec if r != NONE})  # :114-116
    gof_index = {}
    for fid, _seq, s, e in B.gof:
        gof_index[fid] = (s, e)  # gof.rs:32-37 later duplicates win
    blocks = [(r,) + gof_index.get(r, (MISSING, MISSING)) for r in roots]  # :119
    if (not entire_group) or (types is not None):  # :121
        per_root: Dict[int, set] = {}
        for f, r in zip(fids, roots_vec):  # :127-135
            if r != NONE and f < len(B.ids):
                per_root.setdefault(r, set()).add(B.ids[f])
        out = write_gff_output_filtered(gff, blocks, per_root, types)
    else:
        out = write_gff_output(gff, blocks)
    return out, missing, invalid


def rust_debug_list(names: Sequence[str]) -> str:
    """`{:?}` of a Vec<String> for names of printable characters without quotes or backslashes"""
    return "[" + ", ".join('"%s"' % n for n in names) + "]"
