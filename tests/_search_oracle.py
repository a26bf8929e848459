"""TEST INFRASTRUCTURE ONLY -- pure-Python restatement of the reference's `gffx search` (Baohua-Chen/GFFx v0.4.0, paths
relative to its src/): commands/search.rs:55-252, index_loader/core.rs:37-89 (load_atn), index_loader/a2f.rs:77-113 and, through
tests/_extract_oracle.py, prt.rs:54-72 and both writers of utils/common.rs.  It follows the source text line by line and cites
it; the reference cannot be built here, so parity is pinned by hand-derived answers (tests/test_search_oracle.py).  Python's
re.search is the regex oracle: within the subset the product accepts it agrees with the reference's Regex::is_match, given
values without "\\n" (load_atn cannot produce one).  The product's deliberate differences are restated too: the AID warnings
come in ascending aid order, and the parent chase ends after n steps.
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Sequence, Tuple

import _extract_oracle as xo
from _extract_oracle import MISSING, NONE, _WS, Built, build_index  # noqa: F401

BOM = "﻿"


def load_atn(data: bytes) -> Tuple[str, List[str]]:
    """core.rs:37-89"""
    values: List[str] = []
    attr_name: Optional[str] = None
    parts = data.split(b"\n")  # :73-83 (a trailing piece without "\n" is a line; an empty one is dropped by :47)
    for raw in parts:
        if not raw:  # :47-49
            continue
        try:
            line = raw.decode("utf-8").strip(_WS)  # :50-52
        except UnicodeDecodeError:
            raise ValueError("ATN contains invalid UTF-8")
        if attr_name is None and line.startswith(BOM):  # :55-57
            line = line[len(BOM):]
        if line.startswith("#attribute="):  # :59-64
            if attr_name is not None:
                raise ValueError("Multiple #attribute= headers found in .atn file")
            attr_name = line[len("#attribute="):]
        elif line and not line.startswith("#"):  # :65-68
            values.append(line)
    if attr_name is None:  # :85-86
        raise ValueError("Missing #attribute=... header in .atn file")
    return attr_name, values


def load_a2f(data: bytes) -> List[int]:
    """a2f.rs:77-113: word f = the aid of fid f; NONE = no attribute"""
    if len(data) % 4:
        raise ValueError("Corrupted A2F: length %d not aligned to u32" % len(data))
    return [int.from_bytes(data[i:i + 4], "little") for i in range(0, len(data), 4)]


def atn_bytes(attr_name: str, values: Sequence[str]) -> bytes:
    """what `gffx index` writes (index_builder/core.rs:209-239)"""
    return ("#attribute=%s\n" % attr_name + "".join(v + "\n" for v in values)).encode()


def read_attr_list(data: bytes) -> List[str]:
    """search.rs:76-82: BufRead::lines, trim(), empty ones dropped; duplicates stay"""
    parts = data.split(b"\n")
    if parts and parts[-1] == b"":
        parts.pop()
    out = []
    for raw in parts:
        if raw.endswith(b"\r"):
            raw = raw[:-1]
        s = raw.decode("utf-8").strip(_WS)
        if s:
            out.append(s)
    return out


def match_aids(values: Sequence[str], patterns: Sequence[str], regex: bool) -> List[int]:
    """search.rs:89-111: the aids whose value matches, ascending"""
    if regex:
        res = [re.compile(p) for p in patterns]
        return [i for i, v in enumerate(values) if any(r.search(v) for r in res)]
    wanted = set(patterns)
    return [i for i, v in enumerate(values) if v in wanted]


class Steps:
    """the state after steps 1-3 (search.rs:89-191)"""
    aids: List[int]
    no_fid_aids: List[int]  # "[WARN] AID n not found (no FIDs)."
    fids: List[int]
    invalid: List[int]
    roots: List[int]
    per_root: Dict[int, set]  # root -> the matched value strings some fid under it carries (:209-218)
    bail: Optional[str] = None


def steps(values: Sequence[str], a2f: Sequence[int], prt: Sequence[int], patterns: Sequence[str], regex: bool) -> Steps:
    S = Steps()
    S.aids = match_aids(values, patterns, regex)
    S.no_fid_aids, S.fids, S.invalid, S.roots, S.per_root = [], [], [], [], {}
    if not S.aids:  # :114-116
        S.bail = "None of the attributes matched."
        return S
    aid_to_fids: Dict[int, List[int]] = {}
    for f, a in enumerate(a2f):  # a2f.rs:96-104
        if a != NONE:
            aid_to_fids.setdefault(a, []).append(f)
    attr_to_fids: Dict[str, set] = {}
    for a in S.aids:  # :130-138 (per string there; the union is the same)
        if a in aid_to_fids:
            attr_to_fids.setdefault(values[a], set()).update(aid_to_fids[a])
        else:
            S.no_fid_aids.append(a)
    if not attr_to_fids:  # :140-142
        S.bail = "No feature IDs (FIDs) resolved from matched attributes."
        return S
    S.fids = sorted(set().union(*attr_to_fids.values()))  # :152-157
    root = {f: xo.resolve_root(prt, f) for f in S.fids}  # :164
    S.invalid = [f for f in S.fids if root[f] == NONE]  # :167-185
    S.roots = sorted({r for r in root.values() if r != NONE})  # :186-187
    if not S.roots:  # :189-191
        S.bail = "No valid root features resolved from matched attributes."
        return S
    for v, fs in attr_to_fids.items():  # :209-218
        for f in fs:
            if root[f] != NONE:
                S.per_root.setdefault(root[f], set()).add(v)
    return S


def search_run(gff: bytes, gof, attr_name: str, values: Sequence[str], a2f: Sequence[int], prt: Sequence[int], patterns: Sequence[str],
               regex: bool, entire_group: bool, types: Optional[str]):
    """search.rs:55-252.  gof: (fid, seq, start, end) records.  Returns (output bytes, Steps)."""
    S = steps(values, a2f, prt, patterns, regex)
    if S.bail:
        return b"", S
    gof_index = {}
    for fid, _seq, s, e in gof:
        gof_index[fid] = (s, e)  # gof.rs:32-37 later duplicates win
    blocks = [(r,) + gof_index.get(r, (MISSING, MISSING)) for r in S.roots]  # :196
    if (not entire_group) or (types is not None):  # :198
        out = xo.write_gff_output_filtered(gff, blocks, S.per_root, types, attr_name.encode())
    else:
        out = xo.write_gff_output(gff, blocks)
    return out, S


def warn_lines(S: Steps) -> List[bytes]:
    """the [WARN] lines of a run, in the product's order"""
    out = [b"[WARN] AID %d not found (no FIDs)." % a for a in S.no_fid_aids]
    if S.invalid:
        out.append(b"[WARN] %d FIDs have invalid parent chains (or out-of-range): [%s]" % (len(S.invalid), ", ".join(map(str, S.invalid)).encode()))
    return out
