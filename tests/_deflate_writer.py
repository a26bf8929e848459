"""A DEFLATE (RFC 1951) *writer* in plain Python for the BGZF tests (tests/test_deflate_streams_cpu.py, _gpu.py): it builds a
raw stream from an explicit description, so that a test can put into a member what zlib's encoder never emits -- 15-bit codes,
distance symbols 28 / 29, both spellings of length 258, code-length repeats that run across the border between the
literal/length and the distance lengths (libdeflate codes the two tables as one sequence), one-code and empty distance tables,
untrimmed HLIT / HDIST, empty blocks, stored blocks after bit-unaligned ones.

A stream is a list of blocks: stored(bytes), fixed(items), dynamic(litlen_lengths, dist_lengths, items, header_rle, trim).
items are literals (int 0..255) and matches (length, distance) or (258, distance, 284): length 258 spelled as symbol 284 with
extra bits 31 instead of symbol 285.  deflate(blocks) returns the raw stream and the bytes it stands for, played back by the
writer itself; features(blocks) counts what the description holds (no decoder is asked).  The base / extra tables are RFC 1951
§3.2.5, the same as length_base / dist_base in device/bgzf_core.hpp."""
import struct
import zlib
from collections import Counter

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0 if (s < 8 or s == 28) else (s - 4) >> 2 for s in range(29)]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0 if s < 4 else (s - 2) >> 1 for s in range(30)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
MAX_OUT = 65536      # output bytes of a BGZF member
MAX_MEMBER = 65536   # bytes of a BGZF member, header and footer included (BSIZE is 16 bits)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30


def stored(data):
    return {"type": "stored", "data": bytes(data)}


def fixed(items):
    return {"type": "fixed", "items": list(items)}


def dynamic(litlen_lengths, dist_lengths, items, header_rle="joined", trim=True, header_ops=None):
    """header_rle: how the code-length sequence is run-length coded -- "none", "table" (each table by itself, as zlib does) or
    "joined" (one sequence, so repeats may cross the border).  trim: drop trailing zero lengths (else HLIT / HDIST say
    len(litlen_lengths) - 257 / len(dist_lengths) - 1).  header_ops: the (symbol, extra) sequence itself, for invalid streams."""
    assert header_rle in ("none", "table", "joined")
    return {"type": "dynamic", "ll": list(litlen_lengths), "dl": list(dist_lengths), "items": list(items), "rle": header_rle,
            "trim": trim, "ops": header_ops}


def length_symbol(length, spelling=285):
    """(symbol, extra bits, extra value) of a match length 3..258."""
    if length == 258:
        return (285, 0, 0) if spelling == 285 else (284, 5, 31)
    s = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + s, LEN_EXTRA[s], length - LEN_BASE[s]


def dist_symbol(distance):
    s = max(i for i in range(30) if DIST_BASE[i] <= distance)
    return s, DIST_EXTRA[s], distance - DIST_BASE[s]


def canonical_codes(lengths):
    """RFC 1951 §3.2.2: {symbol: (code, length)} of the symbols with a non-zero length."""
    count = Counter(l for l in lengths if l)
    code, nxt = 0, {}
    for l in range(1, 16):
        code = (code + count.get(l - 1, 0)) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def kraft_left(lengths):
    """2^15 minus the code space the lengths take: 0 complete, > 0 incomplete, < 0 over-subscribed."""
    return (1 << 15) - sum(1 << (15 - l) for l in lengths if l)


def random_complete(n, max_len, rng):
    """The lengths of a random COMPLETE code of n symbols whose longest code is max_len bits (n > max_len, n <= 2^max_len):
    a chain down to max_len, then random leaves split until there are n."""
    assert max_len + 1 <= n <= (1 << max_len)
    leaves = list(range(1, max_len + 1)) + [max_len]
    while len(leaves) < n:
        open_ = [i for i, d in enumerate(leaves) if d < max_len]
        i = open_[int(rng.integers(0, len(open_)))]
        leaves[i] += 1
        leaves.append(leaves[i])
    return [leaves[i] for i in rng.permutation(n)]


def skewed():
    """1, 2, ..., 14, 15, 15: complete, and every length of the canonical walk is taken by one symbol."""
    return list(range(1, 16)) + [15]


def spread(code_lengths, symbols, alphabet):
    """A length list over `alphabet` symbols: code_lengths[i] for symbols[i], 0 elsewhere."""
    out = [0] * alphabet
    for l, s in zip(code_lengths, symbols):
        out[s] = l
    return out


def used_symbols(items, spelling_default=285):
    ll, dd = Counter({256: 1}), Counter()
    for it in items:
        if isinstance(it, int):
            ll[it] += 1
        else:
            ll[length_symbol(it[0], it[2] if len(it) > 2 else spelling_default)[0]] += 1
            dd[dist_symbol(it[1])[0]] += 1
    return ll, dd


def lengths_for(freq, alphabet, max_len, rng, by_frequency=False, skew=False):
    """Code lengths over `alphabet` symbols that give every symbol of freq a code: a random complete code (or the skewed one)
    over those symbols and as many random others as the longest code needs.  by_frequency: the short codes go to the frequent
    symbols (compress()); else at random."""
    syms = sorted(freq)
    need = 16 if skew else max(max_len + 1, 2)
    if skew:
        assert len(syms) <= 16
    if len(syms) < need:
        rest = [s for s in range(alphabet) if s not in freq]
        syms += [rest[i] for i in rng.permutation(len(rest))[:need - len(syms)]]
    ls = skewed() if skew else random_complete(len(syms), max_len, rng)
    if by_frequency:
        ls = sorted(ls)
        syms = sorted(syms, key=lambda s: -freq.get(s, 0))
    else:
        syms = [syms[i] for i in rng.permutation(len(syms))]
    return spread(ls, syms, alphabet)


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, k):  # k bits of v, least significant first (RFC 1951 §3.1.1: everything but Huffman codes)
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, c):  # a Huffman code, most significant bit first
        v, k = c
        self.put(int(format(v, "0%db" % k)[::-1], 2), k)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bit_pos(self):
        return len(self.out) * 8 + self.n


def _rle(seq):
    """Greedy run-length coding of a code-length sequence: [(symbol, extra value, lengths covered)]."""
    ops, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                ops.append((18, r - 11, r))
                run -= r
            if run >= 3:
                ops.append((17, run - 3, run))
                run = 0
        else:
            ops.append((v, 0, 1))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                ops.append((16, r - 3, r))
                run -= r
        ops += [(v, 0, 1)] * run
        i = j
    return ops


def _header_ops(b, nlen, ndist):
    ll, dl = b["ll"][:nlen], b["dl"][:ndist]
    if b["ops"] is not None:
        return [(s, x, {16: 3 + x, 17: 3 + x, 18: 11 + x}.get(s, 1)) for s, x in b["ops"]]
    if b["rle"] == "none":
        return [(v, 0, 1) for v in ll + dl]
    if b["rle"] == "table":
        return _rle(ll) + _rle(dl)
    return _rle(ll + dl)


def _cl_lengths(ops, seed):
    """A complete code for the code-length alphabet (at most 7 bits) over the symbols the ops use."""
    rng = np.random.default_rng(seed)
    freq = Counter(s for s, _, _ in ops)
    if len(freq) < 2:  # the code-length code may not be incomplete: a second symbol that nothing uses
        freq[next(s for s in (0, 8, 1) if s not in freq)] = 0
    if len(freq) == 2:
        return spread([1, 1], sorted(freq), 19)
    lo = (len(freq) - 1).bit_length()
    return lengths_for(freq, 19, int(rng.integers(lo, 8)), rng, by_frequency=True)


def _encode(blocks, check=True):
    """-> raw, data, Counter of features.  check=False writes what the description says even where it is not a valid stream
    (no playback guarantees then)."""
    w, data, feat = _Bits(), bytearray(), Counter()
    kinds = []
    for bi, b in enumerate(blocks):
        start_bits = w.bit_pos()
        w.put(1 if bi == len(blocks) - 1 else 0, 1)
        w.put({"stored": 0, "fixed": 1, "dynamic": 2}[b["type"]], 2)
        before = len(data)
        if b["type"] == "stored":
            if kinds and kinds[-1][0] != "stored" and start_bits % 8:
                feat["stored after a bit-unaligned Huffman block"] += 1
            w.align()
            n = len(b["data"])
            assert n <= 65535
            w.out += struct.pack("<HH", n, n ^ 0xFFFF) + b["data"]
            data += b["data"]
        else:
            if b["type"] == "fixed":
                ll, dl = FIXED_LL, FIXED_D
            else:
                ll, dl = b["ll"], b["dl"]
                if b["trim"]:
                    nlen = max([257] + [i + 1 for i, l in enumerate(ll) if l])
                    ndist = max([1] + [i + 1 for i, l in enumerate(dl) if l])
                else:
                    nlen, ndist = len(ll), len(dl)
                ops = _header_ops(b, nlen, ndist)
                cl = _cl_lengths(ops, bi * 1000003 + len(ops))
                ncode = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl[s]])
                if check:
                    assert 257 <= nlen <= 286 and 1 <= ndist <= 30 and len(ll) >= nlen and len(dl) >= ndist
                    assert sum(r for _, _, r in ops) == nlen + ndist
                    assert ll[256] and kraft_left(ll[:nlen]) == 0, "literal/length code must be complete"
                    used_d = [l for l in dl[:ndist] if l]
                    assert kraft_left(used_d) == 0 or used_d == [1] or not used_d, "distance code: complete, one code or none"
                w.put(nlen - 257, 5)
                w.put(ndist - 1, 5)
                w.put(ncode - 4, 4)
                for s in CL_ORDER[:ncode]:
                    w.put(cl[s], 3)
                clc = canonical_codes(cl)
                at = 0
                for s, x, r in ops:
                    w.code(clc[s])
                    if s >= 16:
                        w.put(x, {16: 2, 17: 3, 18: 7}[s])
                        if at < nlen < at + r:
                            feat["repeat %d across the table border" % s] += 1
                    at += r
                feat["HLIT = 29"] += nlen == 286
                feat["HDIST = 29"] += ndist == 30
                feat["single-code distance table"] += [l for l in dl[:ndist] if l] == [1]
                feat["block without distance codes"] += not any(dl[:ndist])
                ll, dl = ll[:nlen] + [0] * (288 - nlen), dl[:ndist] + [0] * (32 - ndist)
            lc, dc = canonical_codes(ll), canonical_codes(dl)
            for it in b["items"]:
                if isinstance(it, int):
                    w.code(lc[it])
                    data.append(it)
                    bits = lc[it][1]
                else:
                    length, dist = it[0], it[1]
                    s, xb, xv = length_symbol(length, it[2] if len(it) > 2 else 285)
                    ds, dxb, dxv = dist_symbol(dist)
                    w.code(lc[s])
                    w.put(xv, xb)
                    w.code(dc[ds])
                    w.put(dxv, dxb)
                    bits = lc[s][1]
                    if check:
                        assert 3 <= length <= 258 and 1 <= dist <= len(data) and dist <= 32768, (length, dist, len(data))
                    for _ in range(length):
                        data.append(data[-dist] if dist <= len(data) else 0)
                    feat["distance %d" % dist] += dist in (1, 16385, 24577, 32768)
                    feat["distance 1..3 with length >= 100"] += dist <= 3 and length >= 100
                    feat["length 258 as symbol %d" % s] += length == 258
                    feat["used distance code longer than 9 bits"] += dc[ds][1] > 9
                feat["used 15-bit literal/length code"] += bits == 15
                feat["used 10..14-bit literal/length code"] += 10 <= bits <= 14
            if 256 in lc:
                w.code(lc[256])
            else:
                assert not check
        kinds.append((b["type"], len(data) - before))
    for i in range(1, len(kinds) - 1):
        if kinds[i][1] == 0 and kinds[i - 1][1] and kinds[i + 1][1]:
            feat["empty %s block between non-empty blocks" % kinds[i][0]] += kinds[i][0] in ("stored", "fixed")
    feat["member of five or more blocks"] += len(blocks) >= 5 and len({k for k, _ in kinds}) >= 2
    w.align()
    if check:
        assert len(data) <= MAX_OUT and 18 + len(w.out) + 8 <= MAX_MEMBER, (len(data), len(w.out))
    return bytes(w.out), bytes(data), +feat


FEATURES = ["used 15-bit literal/length code", "used 10..14-bit literal/length code", "used distance code longer than 9 bits",
            "distance 32768", "distance 24577", "distance 16385", "distance 1", "length 258 as symbol 285",
            "length 258 as symbol 284", "repeat 16 across the table border", "repeat 17 across the table border",
            "repeat 18 across the table border", "single-code distance table", "block without distance codes", "HLIT = 29",
            "HDIST = 29", "empty stored block between non-empty blocks", "empty fixed block between non-empty blocks",
            "stored after a bit-unaligned Huffman block", "member of five or more blocks",
            "distance 1..3 with length >= 100"]


def deflate(blocks, check=True):
    raw, data, _ = _encode(blocks, check)
    return raw, data


def features(blocks):
    return _encode(blocks)[2]


def member(raw, data, before=b"", after=b"", ftext=False, mtime=0, xfl=0, os_=255):
    """A BGZF member around a raw stream.  before / after: whole extra subfields (SI1 SI2 SLEN data) around `BC`."""
    extra_len = len(before) + 6 + len(after)
    total = 12 + extra_len + len(raw) + 8
    assert total <= MAX_MEMBER and len(data) <= MAX_OUT, (total, len(data))
    return (struct.pack("<BBBBIBBH", 31, 139, 8, 4 | (1 if ftext else 0), mtime, xfl, os_, extra_len) + before + b"BC\x02\x00" +
            struct.pack("<H", total - 1) + after + raw + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def subfield(si, payload):
    return si + struct.pack("<H", len(payload)) + payload


# ---- directed cases ----------------------------------------------------------------------------------------------------
def _lits(data):
    return list(data)


def directed_cases():
    """{name: blocks}: each feature of FEATURES, on purpose."""
    rng = np.random.default_rng(11)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    cases = {}
    # the skewed code on both tables: every length 1..15 decoded, the 15-bit codes and distance symbols 28 / 29 used
    lsyms = [ord("a") + i for i in range(11)] + [256, 257, 270, 284, 285]  # 16 symbols: lengths 3, 23..26, 227..258, 258
    dsyms = [0, 1, 2, 5, 9, 12, 15, 18, 20, 22, 24, 25, 26, 27, 28, 29]
    items = [lsyms[i % 11] for i in range(60)]
    items += [(3, 1), (24, 2), (258, 3), (258, 1, 284), (258, 2), (230, 3)]
    items += [(3, d) for d in (32768, 24577, 16385, 16384, 32767, 24576)] + [(258, 32768), (258, 32768, 284), (25, 24577)]
    items += [(3, DIST_BASE[s]) for s in dsyms] + [lsyms[i] for i in range(11)]
    for name, rot in (("skewed", 0), ("skewed_rotated", 5)):  # rotated: other symbols get the long codes
        ll = spread(skewed(), lsyms[rot:] + lsyms[:rot], 286)
        dl = spread(skewed(), dsyms[rot:] + dsyms[:rot], 30)
        cases[name] = [stored(rnd(32768)), dynamic(ll, dl, items, "joined")]
    # a 9-bit code over some text, lengths 3, 4, 5, 195..226, 227..258
    ll = spread(random_complete(43, 9, rng), list(range(90, 126)) + [256, 257, 258, 259, 283, 284, 285], 286)
    text = bytes(rng.integers(90, 126, 300, dtype=np.uint8))
    # repeats across the border.  16: the last four literal/length lengths and the first four distance lengths are all 6
    ll16 = spread([1, 2, 3, 4, 6, 6, 6, 6], [100, 101, 102, 256, 282, 283, 284, 285], 286)
    dl16 = [6, 6, 6, 6, 4, 4, 4, 2, 2, 2] + [0] * 20
    it16 = [100, 101, 102, 100, (258, 1), (258, 2, 284), (163, 3), (200, 4), (227, 9), (258, 25), (194, 6)]
    cases["repeat16_border"] = [dynamic(ll16, dl16, it16, "joined", trim=False)]
    # 17: five zeros, two at the end of the literal/length lengths and three at the head of the distance lengths
    ll17 = spread(random_complete(40, 9, rng), list(range(90, 126)) + [256, 257, 258, 283], 286)
    dl17 = [0, 0, 0, 1, 1] + [0] * 25
    cases["repeat17_border"] = [dynamic(ll17, dl17, _lits(text) + [(3, 4), (4, 5), (195, 4), (226, 6)], "joined", trim=False)]
    # 18: 13 + 12 zeros, HLIT = 13 sent untrimmed; then the same with HLIT = 29
    ll18 = spread(random_complete(38, 9, rng), list(range(90, 126)) + [255, 256], 286)
    dl18 = [0] * 12 + [1, 1] + [0] * 16
    it18 = _lits(text[:100])
    cases["repeat18_border"] = [stored(rnd(200)), dynamic(ll18[:270], dl18, it18, "joined", trim=False)]
    cases["repeat18_border_hlit29"] = [stored(rnd(200)), dynamic(ll18, dl18, it18, "joined", trim=False)]
    # the same tables with the two other header codings
    cases["rle_per_table"] = [dynamic(ll16, dl16, it16, "table", trim=False)]
    cases["rle_none"] = [dynamic(ll16, dl16, it16, "none", trim=True)]
    # one distance code of length 1 (incomplete, allowed) -- as symbol 0 and as symbol 29; and no distance code at all
    cases["dist_single_code"] = [dynamic(ll, spread([1], [0], 30), _lits(text) + [(258, 1), (3, 1), (258, 1, 284)] + _lits(text[:9]))]
    cases["dist_single_code_29"] = [stored(rnd(32768)), dynamic(ll, spread([1], [29], 30), _lits(text) + [(5, 24577), (258, 32768)])]
    cases["dist_none"] = [dynamic(ll, [0] * 30, _lits(text), "joined"), dynamic(ll, [0] * 30, _lits(text[:7]), "none", trim=False)]
    # untrimmed tables
    tail = [(4, 1), (5, 2), (3, 1), (258, 8)]
    cases["hlit29_hdist29"] = [dynamic(ll, spread(random_complete(8, 4, rng), range(8), 30), _lits(text) + tail, "table", trim=False)]
    # empty blocks between others, a stored block after a Huffman block that ends inside a byte, many blocks
    cases["empty_blocks"] = [fixed(_lits(b"abc")), stored(b""), fixed(_lits(b"defg") + [(4, 2)]), fixed([]), stored(b"tail"),
                             fixed([]), stored(b""), dynamic(ll, dl17, _lits(text[:50]) + [(5, 4)]), stored(b"")]
    cases["stored_after_unaligned"] = [fixed(_lits(b"a")), stored(b"0123456789"), fixed(_lits(b"ab")), stored(b"x" * 300),
                                       dynamic(ll, dl17, _lits(text[:21])), stored(rnd(1000)), fixed([(258, 1000)])]
    cases["only_empty"] = [stored(b""), fixed([]), stored(b"")]
    # overlapping copies next to far ones in one block, fixed and dynamic
    mixed = _lits(b"xyz") + [(258, 1), (258, 2), (258, 3), (257, 1), (100, 2), (3, 3), (258, 1, 284), (200, 3)]
    mixed += [(258, 20000), (40, 1), (258, 20483), (3, 20000), (130, 2)]
    cases["overlap_and_far_fixed"] = [stored(rnd(20000)), fixed(mixed)]
    ls, ds = used_symbols(mixed)
    cases["overlap_and_far_dynamic"] = [stored(rnd(20000)),
                                        dynamic(lengths_for(ls, 286, 12, rng), lengths_for(ds, 30, 11, rng), mixed, "joined")]
    # every length symbol and every distance symbol once, fixed and dynamic
    every = [(LEN_BASE[s] + max(0, (1 << LEN_EXTRA[s]) - 2), DIST_BASE[(s * 7) % 30]) for s in range(29)]
    every += [(3 + s, DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1) for s in range(30)] + [(258, 1, 284)]
    cases["every_symbol_fixed"] = [stored(rnd(32768)), fixed(every)]
    ls, ds = used_symbols(every)
    cases["every_symbol_dynamic"] = [stored(rnd(32768)), dynamic(lengths_for(ls, 286, 15, rng), lengths_for(ds, 30, 15, rng), every)]
    return cases


# ---- random members ----------------------------------------------------------------------------------------------------
def _random_items(rng, have, room, n_items, alphabet, max_symbols=None):
    """Items for one block: `have` bytes are already out, `room` more may be written."""
    items, made = [], 0
    lens_used = set()
    for _ in range(n_items):
        k = rng.random()
        if have + made == 0 or k < 0.45 or room - made < 258:
            if room - made < 1:
                break
            items.append(int(alphabet[int(rng.integers(0, len(alphabet)))]))
            made += 1
            continue
        cur = have + made
        j = rng.random()
        if j < 0.3:
            dist = int(rng.integers(1, 4))
        elif j < 0.4:
            dist = int([1, 16385, 24577, 32768, 4, 5, 8193][int(rng.integers(0, 7))])
        else:
            dist = int(rng.integers(1, min(cur, 32768) + 1))
        dist = min(dist, cur, 32768)
        j = rng.random()
        length = 258 if j < 0.2 else int(rng.integers(3, 259)) if j < 0.6 else int(rng.integers(3, 12))
        sym = length_symbol(length)[0]
        if max_symbols is not None and sym not in lens_used and len(lens_used) >= max_symbols:
            length = LEN_BASE[min(lens_used) - 257]
        lens_used.add(length_symbol(length)[0])
        items.append((length, dist, 284) if length == 258 and rng.random() < 0.5 and (max_symbols is None or 284 in lens_used)
                     else (length, dist))
        made += length
    return items, made


def random_blocks(seed):
    """A random member's blocks: one to eight blocks of all three types, code lengths up to 15 bits, all header codings."""
    rng = np.random.default_rng([seed, 0xDEF1A7E])
    blocks, have = [], 0
    budget_raw = 60000  # bytes of raw stream, estimated generously: 2 bytes per literal, 8 per match
    if rng.random() < 0.4:
        n = int(rng.integers(1, 33001))
        blocks.append(stored(rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
        have += n
        budget_raw -= n + 5
    for _ in range(int(rng.integers(1, 8))):
        k = rng.random()
        room = min(MAX_OUT - have, 20000)
        if k < 0.12:
            n = 0 if rng.random() < 0.4 else int(rng.integers(1, 400))
            n = min(n, room)
            blocks.append(stored(rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
            have += n
            budget_raw -= n + 5
            continue
        if k < 0.2:
            blocks.append(fixed([]))
            continue
        skew = k > 0.85
        n_alpha = int(rng.integers(1, 10)) if skew else int([2, 20, 90, 256][int(rng.integers(0, 4))])
        alphabet = rng.permutation(256)[:n_alpha]
        n_items = min(int(rng.integers(1, 400)), budget_raw // 8)
        items, made = _random_items(rng, have, room, n_items, alphabet, max_symbols=(15 - n_alpha) if skew else None)
        budget_raw -= 8 * len(items) + 330
        if k < 0.4:
            blocks.append(fixed(items))
        else:
            ls, ds = used_symbols(items)
            lo = max(2, (max(len(ls), 2) - 1).bit_length())
            ml = 15 if skew else int(rng.integers(lo, 16))
            ll = lengths_for(ls, 286, ml, rng, skew=skew)
            j = rng.random()
            if not ds:
                dl = [0] * 30 if j < 0.5 else spread([1], [int(rng.integers(0, 30))], 30)
            elif len(ds) == 1 and j < 0.5:
                dl = spread([1], list(ds), 30)
            else:
                dlo = max(1, (max(len(ds), 2) - 1).bit_length())
                dl = lengths_for(ds, 30, int(rng.integers(dlo, 16)), rng, skew=len(ds) <= 16 and j > 0.8)
            blocks.append(dynamic(ll, dl, items, ["none", "table", "joined", "joined"][int(rng.integers(0, 4))],
                                  trim=bool(rng.random() < 0.5)))
        have += made
    return blocks


def random_member(seed, **header):
    """-> (member bytes, the bytes it stands for, its blocks)."""
    blocks = random_blocks(seed)
    raw, data = deflate(blocks)
    return member(raw, data, **header), data, blocks


# ---- compress ----------------------------------------------------------------------------------------------------------
def compress(data, seed=0, block_items=3000):
    """`data` (at most 65536 bytes) as blocks of this writer: greedy matches found through a table of 3-byte prefixes, cut into
    dynamic blocks whose code lengths are random complete codes (short codes to frequent symbols, longest code 9..15 bits) with
    joined header coding, now and then a fixed block.  Falls back to stored blocks if that would outgrow a BGZF member."""
    assert len(data) <= MAX_OUT
    rng = np.random.default_rng([seed, len(data)])
    items, table, i, n = [], {}, 0, len(data)
    while i < n:
        key = data[i:i + 3]
        j = table.get(key)
        table[key] = i
        if j is not None and len(key) == 3 and i - j <= 32768:
            k = 3
            while k < 258 and i + k < n and data[j + k] == data[i + k]:
                k += 1
            items.append((k, i - j, 284) if k == 258 and (i & 1) else (k, i - j))
            i += k
        else:
            items.append(data[i])
            i += 1
    blocks = []
    for a in range(0, len(items), block_items):
        part = items[a:a + block_items]
        if rng.random() < 0.15:
            blocks.append(fixed(part))
            continue
        ls, ds = used_symbols(part)
        lo = max(9, (len(ls) - 1).bit_length())
        ll = lengths_for(ls, 286, int(rng.integers(lo, 16)), rng, by_frequency=True)
        if not ds:
            dl = [0] * 30
        elif len(ds) == 1:
            dl = spread([1], list(ds), 30)
        else:
            dl = lengths_for(ds, 30, int(rng.integers(max(5, (len(ds) - 1).bit_length()), 16)), rng, by_frequency=True)
        blocks.append(dynamic(ll, dl, part, "joined", trim=bool(rng.random() < 0.7)))
    if not blocks:
        blocks = [fixed([])]
    raw, back, _ = _encode(blocks, check=False)
    assert back == bytes(data)
    if 18 + len(raw) + 8 > MAX_MEMBER:
        blocks = [stored(data[a:a + 65535]) for a in range(0, n, 65535)]
    return blocks


def compress_member(data, seed=0):
    raw, back = deflate(compress(data, seed))
    assert back == bytes(data)
    return member(raw, back)


# ---- what the two test modules share ------------------------------------------------------------------------------------
encode = _encode  # blocks -> (raw, data, features)

RANDOM_SEEDS = (1, 2, 3)   # corpus(): RANDOM_PER_SEED members for each
RANDOM_PER_SEED = 100


def corpus():
    """[(name, member, data, features)]: the directed cases, then RANDOM_PER_SEED random members for each of RANDOM_SEEDS.
    Nothing is left out: a member that breaks a limit fails an assertion of the writer."""
    out = []
    for name, blocks in directed_cases().items():
        raw, data, feat = _encode(blocks)
        out.append((name, member(raw, data), data, feat))
    for seed in RANDOM_SEEDS:
        for k in range(RANDOM_PER_SEED):
            raw, data, feat = _encode(random_blocks(seed * 100000 + k))
            out.append(("random %d.%d" % (seed, k), member(raw, data), data, feat))
    return out


STRIPE_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 65535, 65536)


def stripe_edge_members(seed=5):
    """[(name, member, data)]: outputs of STRIPE_SIZES bytes (the CRC stripes of k_bgzf_inflate are ceil(n / 64) bytes), each as a
    stored, a fixed and a dynamic member (the two largest: mostly stored).  The data is text over 20 letters with repeats, so the large ones fit a member."""
    rng = np.random.default_rng(seed)
    out = []
    for n in STRIPE_SIZES:
        words = [bytes(rng.integers(97, 117, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(50)]
        data = b"".join(words[i] for i in rng.integers(0, 50, n // 2 + 1))[:n]
        assert len(data) == n
        items = [it for b in compress(data, seed, block_items=1 << 30) for it in b["items"]] if n > 300 else list(data)
        ls, ds = used_symbols(items)
        dl = lengths_for(ds, 30, 9, rng, by_frequency=True) if len(ds) > 1 else spread([1], list(ds), 30)
        cut, k = 0, 0  # a stored block takes its bytes as they are, so a member holds 65505 of them at most: the first 60000
        while n > 60000 and cut < 60000:  # bytes stored and the rest as a fixed block in that case
            cut += 1 if isinstance(items[k], int) else items[k][0]
            k += 1
        forms = {"stored": [stored(data[:cut]), fixed(items[k:])] if cut else [stored(data)], "fixed": [fixed(items)],
                 "dynamic": [dynamic(lengths_for(ls, 286, 12, rng, by_frequency=True), dl, items)]}
        for form, blocks in forms.items():
            raw, back = deflate(blocks)
            assert back == data
            out.append(("%d %s" % (n, form), member(raw, data), data))
    return out


HEADER_VARIANTS = {
    "htslib": {},
    "subfield before BC": {"before": subfield(b"RA", b"\x01\x02\x03")},
    "subfield after BC": {"after": subfield(b"XY", b"")},
    "subfields around BC": {"before": subfield(b"AB", b"12345678") + subfield(b"BC", b"\x00"), "after": subfield(b"ZZ", b"\xff" * 40)},
    "FTEXT": {"ftext": True},
    "MTIME XFL OS": {"mtime": 1_700_000_000, "xfl": 2, "os_": 3},
    "all": {"before": subfield(b"BD", b"\x00\x00"), "after": subfield(b"CB", b"\x01\x02"), "ftext": True, "mtime": 0xFFFFFFFF, "xfl": 4,
            "os_": 0},
}


def foreign_bam(header, records, layout, block=0xFF00, seed=0, deflater=None):
    """A BAM file's bytes whose members carry the header variants in turn (other writers' gzip headers) around zlib's raw
    streams, or around this writer's with deflater=compress.  Blocks as synth.bgzf_blocks cuts them; the EOF marker last."""
    from gffx_amd import synth
    variants = list(HEADER_VARIANTS.values())
    out = []
    for i, b in enumerate(synth.bgzf_blocks(header, records, layout, True, block)):
        if deflater is None:
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            raw = c.compress(b) + c.flush()
        else:
            raw, back = deflate(deflater(b, seed + i))
            assert back == b
        out.append(member(raw, b, **variants[i % len(variants)]))
    return b"".join(out) + synth.BGZF_EOF
