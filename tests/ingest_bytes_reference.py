"""A byte-level reference of the N-Triples ingest, written from the contract text of include/rgcn_mi355x.h and DESIGN.md 20 alone:
pure Python on ``bytes``, nothing imported from ``graphs.py`` or ``ingest.py``, no ``str`` anywhere (names stay ``bytes``).  Where
tests/ingest_reference.py goes through ``graphs.Graph`` -- and so cannot hold invalid UTF-8, the extra separators of ``splitlines()``
or characters that Unicode ``lower()`` changes -- this one follows the bytewise contract there too.

``lines`` / ``tokens`` / ``expected`` are the reference; everything below them builds the inputs of tests/test_gpu_ingest_edges.py
and tests/test_gpu_ingest_past_2gib.py, and tests/test_ingest_bytes_reference.py checks each builder for the property its GPU test
relies on."""
import random

import numpy as np

RDF_TYPE = b"<http://www.w3.org/1999/02/22-rdf-syntax-ns#type>"
TYPE = b"<type>"
ONTOLOGY = b"http://swrc.ontoware.org/ontology"
_FOLD = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))


def fold(b: bytes) -> bytes:
    """'A'..'Z' -> 'a'..'z'; every other byte is kept"""
    return bytes(b).translate(_FOLD)


# ---- the reference -------------------------------------------------------------------------------------------------------------
def lines(data: bytes):
    """[(start, end, past)] per line: ``data[start:end]`` is the line without its '\\n' and without one '\\r' before it (or before
    the end of the file), ``data[start:past]`` the raw line.  Lines end at '\\n' only; a piece after the last '\\n' is a line if it
    is not empty.  ``len(lines(data))`` is what rgcn_nt_lines answers."""
    out, start, n = [], 0, len(data)
    while start < n:
        nl = data.find(b"\n", start)
        end, past = (n, n) if nl < 0 else (nl, nl + 1)
        if end > start and data[end - 1] == 13:
            end -= 1
        out.append((start, end, past))
        start = past
    return out


def tokens(data: bytes) -> dict:
    """occ: per triple the three (offset, length) pairs into ``data``; T; longest term; the 1-based first malformed line and first
    line holding a NUL (on the raw line, its '\\r' and '\\n' included), each 0 when none.  A line of at most 2 bytes is skipped;
    every other line loses 2 bytes and splits at its first two 0x20 bytes."""
    occ, longest, bad, nul = [], 0, 0, 0
    for number, (start, end, past) in enumerate(lines(data), 1):
        if not nul and data.find(b"\x00", start, past) >= 0:
            nul = number
        if end - start <= 2:
            continue
        end -= 2
        sp1 = data.find(b" ", start, end)
        sp2 = data.find(b" ", sp1 + 1, end) if sp1 >= 0 else -1
        if sp2 < 0:
            bad = bad or number
            continue
        tri = ((start, sp1 - start), (sp1 + 1, sp2 - sp1 - 1), (sp2 + 1, end - sp2 - 1))
        occ.append(tri)
        longest = max(longest, *(ln for _, ln in tri))
    return {"occ": occ, "T": len(occ), "longest": longest, "bad_line": bad, "nul_line": nul}


def first_error(data: bytes):
    """None, or what the loader must raise for: ("nul" | "malformed", line).  The first offending line; NUL on a tie."""
    tk = tokens(data)
    bad, nul = tk["bad_line"], tk["nul_line"]
    if not bad and not nul:
        return None
    return ("nul", nul) if nul and (not bad or nul <= bad) else ("malformed", bad)


def common_prefix(a: bytes, b: bytes) -> int:
    n = min(len(a), len(b))
    return next((i for i in range(n) if a[i] != b[i]), n)


def rounds_by_definition(terms) -> int:
    """a term is final in the first round j in which its zero-padded first 4 (j + 1) bytes are unique among the
    (distinct, folded) terms; rounds = the largest such j, plus 1; no term: 0.  Quadratic in spirit: for small sets."""
    terms = sorted(set(terms))
    longest = max((len(t) for t in terms), default=0)
    worst = -1
    for t in terms:
        j = 0
        while True:
            w = 4 * (j + 1)
            key = t[:w].ljust(w, b"\x00")
            if sum(1 for u in terms if u[:w].ljust(w, b"\x00") == key) == 1:
                break
            j += 1
            assert 4 * j <= longest + 4, "two terms tie after their padding: a NUL byte or a duplicate"
        worst = max(worst, j)
    return worst + 1


def rounds(sorted_terms) -> int:
    """``rounds_by_definition`` for sorted distinct NUL-free terms, in linear time: the term that shares the longest zero-padded
    prefix with t is a neighbour of t in bytewise order, and two such terms first differ at their common prefix length d (a proper
    prefix pads with 0 where the longer one holds a byte >= 1) -- unique from round d // 4 on."""
    worst = -1 if not sorted_terms else 0
    for a, b in zip(sorted_terms, sorted_terms[1:]):
        worst = max(worst, common_prefix(a, b) // 4)
    return worst + 1


def expected(data: bytes) -> dict:
    """The id spaces (sorted folded ``bytes``), edges in file order, labelled nodes and rows, U, T, the longest term and the round
    count of a file without malformed lines and NUL bytes."""
    tk = tokens(data)
    if tk["bad_line"] or tk["nul_line"]:
        raise ValueError(f"not loadable: {first_error(data)}")
    tri = [tuple(fold(data[o:o + n]) for o, n in t) for t in tk["occ"]]
    terms = sorted({x for t in tri for x in t})

    def filtered(s: bytes) -> bool:                   # the subject's bytes up to its first '#' are the ontology prefix
        return s.split(b"#", 1)[0] == ONTOLOGY

    nodes = sorted({s for s, _, _ in tri} | {o for _, _, o in tri})
    rels = sorted({p for _, p, _ in tri if p != RDF_TYPE and p != TYPE})
    typed = [(s, o) for s, p, o in tri if p == RDF_TYPE and not filtered(s)]
    classes = sorted({o for _, o in typed})
    node_id = {t: i for i, t in enumerate(nodes)}
    rel_id = {t: i for i, t in enumerate(rels)}
    cls_id = {t: i for i, t in enumerate(classes)}
    msg = [(node_id[s], rel_id[p], node_id[o]) for s, p, o in tri if p in rel_id]
    e = len(msg)
    edge_index = np.zeros((2, 2 * e), dtype=np.int64)
    edge_type = np.zeros(2 * e, dtype=np.int64)
    for i, (s, r, o) in enumerate(msg):
        edge_index[:, 2 * i] = (s, o)
        edge_index[:, 2 * i + 1] = (o, s)
        edge_type[2 * i], edge_type[2 * i + 1] = 2 * r, 2 * r + 1
    labelled = sorted({node_id[s] for s, _ in typed})
    row = {n: j for j, n in enumerate(labelled)}
    labels = np.zeros((len(labelled), len(classes)), dtype=np.int64)
    for s, o in typed:
        labels[row[node_id[s]], cls_id[o]] = 1
    return {"edge_index": edge_index, "edge_type": edge_type, "nodes": nodes, "relations": rels, "classes": classes,
            "labelled_idx": np.asarray(labelled, dtype=np.int64), "labels": labels, "U": len(terms), "T": tk["T"],
            "longest": tk["longest"], "rounds": rounds(terms), "terms": terms}


# ---- a. tokenizer ---------------------------------------------------------------------------------------------------------------
SPACE_AT = (0, 1, 62, 63, 64, 65, 127, 128, 129)     # offsets of a space from the line's start: lanes 0 / 1 / 62 / 63 of three pieces
ALIGNMENTS = (0, 1, 63)                              # line start mod 64


def _filler(length: int) -> bytes:
    """a triple line of ``length`` >= 16 bytes, '\\n' included"""
    assert length >= 16
    return b'<f> <p> "' + b"f" * (length - 13) + b'" .\n'


def tokenizer_sweep(align: int):
    """(data, line_starts): for every pair sp1 < sp2 of SPACE_AT a line whose first two spaces sit at those offsets, once with the
    object ``<o>`` and once with an empty object (the second space is then the last byte before the two-byte cut); a filler triple
    line in front of each puts its start at ``align`` mod 64.  Adjacent pairs have an empty predicate, sp1 = 0 an empty subject."""
    out, pos, starts = [], 0, []
    for sp1 in SPACE_AT:
        for sp2 in SPACE_AT:
            if sp2 <= sp1:
                continue
            for obj in (b"<o>", b""):
                fill = 16 + (align - (pos + 16)) % 64
                out.append(_filler(fill))
                pos += fill
                starts.append(pos)
                line = b"s" * sp1 + b" " + b"p" * (sp2 - sp1 - 1) + b" " + obj + b" .\n"
                out.append(line)
                pos += len(line)
    return b"".join(out), starts


GOOD = b"<a> <p> <b> .\n"


def error_cases() -> dict:
    """name -> bytes that must be refused; what for and at which line is ``first_error``'s to say (the CPU test pins each)"""
    many = [GOOD] * 3000
    many[2499] = b"<a> <p> .\n"                       # line 2,500: workgroup 624 of the tokenizer (4 lines each)
    many[2899] = b"nospace\n"
    many[2999] = b"<a> <p>\n"
    return {
        "second_space_in_the_cut": GOOD + b"<a> <p> .\n" + GOOD,
        "no_space": GOOD + GOOD + b"abcdef\n",
        "one_space": GOOD + b"<a> <p>xx\n",
        "first_line": b"<a> <p>.\n" + GOOD + b"<a>  \n",
        "above_2048": b"".join(many),
        "last_line_no_newline": GOOD + GOOD + b"<a> <p> .",
        "nul_and_malformed_on_one_line": GOOD + b"<a>\x00<p> .\n" + GOOD,
        "nul_after_malformed": GOOD + b"<a> <p>.\n" + b"<a> <p> <\x00> .\n",
        "nul_before_malformed": b"<a> <p> <\x00> .\n" + GOOD + b"<a> <p>.\n",
        "two_nuls": GOOD + GOOD + b"<a> <\x00> <b> .\n" + b"\x00<a> <p> <b> .\n",
        "nul_in_a_skipped_line": GOOD + b"\n" + b"\x00\n" + GOOD,
        "nul_at_the_cr_position": GOOD + b"<a> <p> <b> .\x00\n" + GOOD,
    }


ERRORS_EXPECTED = {
    "second_space_in_the_cut": ("malformed", 2), "no_space": ("malformed", 3), "one_space": ("malformed", 2),
    "first_line": ("malformed", 1), "above_2048": ("malformed", 2500), "last_line_no_newline": ("malformed", 3),
    "nul_and_malformed_on_one_line": ("nul", 2), "nul_after_malformed": ("malformed", 2), "nul_before_malformed": ("nul", 1),
    "two_nuls": ("nul", 3), "nul_in_a_skipped_line": ("nul", 3), "nul_at_the_cr_position": ("nul", 2),
}

# ---- b. byte passes -------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 3, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8191, 8192, 8193)
BASES = (0, 1, 8, 15)
_PATTERN = (GOOD, b"\n", b"<c> <q> <a> .\r\n", b"<b> <p> <c> .\n", b"\r\n", b"<a> <q> <c> .\n", b"\n\n")     # 62 bytes a turn


def sized_file(n: int, final_newline: bool) -> bytes:
    """exactly ``n`` bytes of short triple lines and blank lines, cut at ``n``; the last byte is '\\n' iff ``final_newline`` (else
    a '\\n' there becomes '.').  Whether the cut leaves a loadable file is the reference's to say."""
    reps = n // sum(len(p) for p in _PATTERN) + 1
    data = bytearray((b"".join(_PATTERN) * reps)[:n])
    if final_newline:
        data[n - 1] = 10
    elif data[n - 1] == 10:
        data[n - 1] = ord(".")
    return bytes(data)


def nul_files():
    """(name, bytes): a NUL at byte 0, at byte n - 1 with and without a '\\n' after it, and at 15, 16, 4,095 and 4,096"""
    out = []
    for n in (16, 17, 4096, 4097):
        base = sized_file(n, False)
        out.append((f"n{n}_first", b"\x00" + base[1:]))
        out.append((f"n{n}_last", base[:-1] + b"\x00"))
        out.append((f"n{n}_last_then_newline", base[:-1] + b"\x00\n"))
    big = sized_file(8193, True)
    for at in (15, 16, 4095, 4096):
        out.append((f"at{at}", big[:at] + b"\x00" + big[at + 1:]))
    return out


# ---- c. bytes beyond graphs.Graph -----------------------------------------------------------------------------------------------
TERM_BYTES = tuple(v for v in range(1, 256) if v not in (10, 32))


def all_bytes_file() -> bytes:
    """terms that together hold every byte 0x01..0xFF but '\\n' and ' ': one-byte terms, ``<v>`` terms, and one term of all of them.
    0x0D is never the byte before a '\\n' (every line ends in " .")."""
    every = bytes(TERM_BYTES)
    out = [b"<all> <holds> " + every + b" .\n"]
    for i, v in enumerate(TERM_BYTES):
        w = TERM_BYTES[(i + 7) % len(TERM_BYTES)]
        out.append(bytes([v]) + b" <p" + bytes([w]) + b"> <" + bytes([w]) + b"> .\n")
    return b"".join(out)


DECIDING = (0x01, 0x41, 0x61, 0x5B, 0x7F, 0x80, 0xC3, 0xFF)
PREFIX_LENGTHS = (3, 4, 5, 7, 8, 9, 63, 64, 65)      # 4k - 1, 4k, 4k + 1 for k = 1, 2, 16


def prefix_file() -> bytes:
    """terms ``"wxyzWXYZ"[:k] + v`` for k = 0..7 (the deciding byte v of DECIDING at each position of the words of rounds 0 and 1;
    0x41 and 0x61 must merge), the same with a tail, proper prefixes ``q * L`` for L in PREFIX_LENGTHS, and the empty term"""
    out = [b" <p> \x01 .\n"]                                             # the empty subject next to \x01
    for k in range(8):
        for v in DECIDING:
            t = b"wxyzWXYZ"[:k] + bytes([v])
            out.append(t + b" <p> " + t + b"tail .\n")
    for n in PREFIX_LENGTHS:
        out.append(b"q" * n + b" <p> <o> .\n")
    return b"".join(out)


SEPARATORS = (b"\x0b", b"\x0c", b"\x1c", b"\x1d", b"\x1e", b"\xc2\x85", b"\xe2\x80\xa8", b"\xe2\x80\xa9", b"\r")


def separators_file() -> bytes:
    """what ``splitlines()`` breaks at, inside terms; upper- and lower-case non-ASCII letters (four terms, none folded); and an
    invalid UTF-8 sequence (e2 82 without its third byte) across the boundary of rounds 0 and 1"""
    out = [b"<s" + sep + b"s> <p" + sep + b"> <o" + sep + b"o> .\n" for sep in SEPARATORS]
    out += ["<É> <p> <é> .\n".encode(), "<Σ> <p> <σ> .\n".encode()]
    out += [b"abc\xe2\x82x <p> abc\xe2\x83x .\n", b"abc\xe2 <p> abc\xe2\x82 .\n"]
    return b"".join(out)


# ---- d. rank rounds at scale ----------------------------------------------------------------------------------------------------
RANK_PREFIX = b"<http://example.org/shared/prefix/of/41b/"      # 41 bytes: rounds 0..9 see nothing else, round 10 byte 40 + 3 of the tail
TIED = b"c" * 12                                                # rounds 11, 12 and 13 of the big group


def rank_scale_file(seed: int = 0) -> bytes:
    """One subject per line behind RANK_PREFIX, in shuffled order.  Tails: ``bbb`` + TIED + id (2,049 terms: one group in rounds
    10..13), ``ddd`` + id (2,048), ``eee`` + id (2,047), ``ff0`` (1), ``gg0`` + id (2), and 300 groups ``h`` + two letters of 1..4
    terms -- about 6,900 terms"""
    assert len(RANK_PREFIX) == 41
    tails = [b"bbb" + TIED + b"%04d" % i for i in range(2049)]
    tails += [b"ddd%04d" % i for i in range(2048)] + [b"eee%04d" % i for i in range(2047)] + [b"ff0", b"gg0a", b"gg0b"]
    for g in range(300):
        head = b"h" + bytes([97 + g // 26, 97 + g % 26])
        tails += [head + b"%d" % i for i in range(1 + g % 4)]
    random.Random(seed).shuffle(tails)
    return b"".join(RANK_PREFIX + t + b" <p> <o> .\n" for t in tails)


def active_groups(terms, round_index: int):
    """sizes of the groups of round ``round_index``: terms that share their zero-padded first 4 * round_index bytes with another
    term (the active set), grouped by their first 4 * (round_index + 1)"""
    w = 4 * round_index
    seen = {}
    for t in terms:
        seen.setdefault(t[:w].ljust(w, b"\x00"), []).append(t)
    groups = {}
    for members in seen.values():
        if len(members) > 1:
            for t in members:
                key = t[:w + 4].ljust(w + 4, b"\x00")
                groups[key] = groups.get(key, 0) + 1
    return sorted(groups.values())


def chain_file() -> bytes:
    """x, xx, ... up to 70 bytes: each a proper prefix of the next"""
    return b"".join(b"x" * n + b" <p> <o> .\n" for n in range(1, 71))


# ---- e. verification ------------------------------------------------------------------------------------------------------------
def three_terms(kind: str):
    """three terms that differ pairwise only as ``kind`` says"""
    base = bytearray(b"v" * 70)
    if kind == "length":                              # the longest first: a run's head is its earliest occurrence, and a later, shorter
        return [b"v" * 72, b"v" * 65, b"v" * 64]      # term equals the head in all of its own bytes -- only the lengths tell them apart
    if kind == "case":
        return [b"v" * 70, b"V" * 70, b"v" * 35 + b"V" * 35]
    at = {"last_byte_of_70": 69, "byte_60": 60, "byte_0": 0}[kind]
    out = []
    for v in b"xyz":
        t = bytearray(base)
        t[at] = v
        out.append(bytes(t))
    return out


def term_lines(terms) -> bytes:
    """``A A A .`` shaped lines"""
    return b"".join(t + b" " + t + b" " + t + b" .\n" for t in terms)


SIX_TERMS = (b"<one>", b"<two>", b"<three>", b"<four>", b"<five>", b"<six>")

# ---- f. roles and labels --------------------------------------------------------------------------------------------------------


def roles_file() -> bytes:
    up = RDF_TYPE.upper()
    rows = [
        (b"<n1>", RDF_TYPE, b"<c1>"), (b"<n1>", RDF_TYPE, b"<c1>"),                 # the same class twice
        (b"<c1>", RDF_TYPE, b"<c2>"),                                               # a class that is a labelled subject
        (b"<n2>", b"<all>", b"<n1>"), (b"<n1>", RDF_TYPE, b"<all>"),                # node, relation and class at once
        (b"<n3>", up, b"<c3>"), (b"<n3>", b"<TYPE>", b"<c4>"),                      # the type predicates in upper case
        (ONTOLOGY, RDF_TYPE, b"<f-bare>"),                                          # fires
        (ONTOLOGY + b"#a#b", RDF_TYPE, b"<f-two-hashes>"),                          # fires
        (ONTOLOGY + b"x#a", RDF_TYPE, b"<k-longer>"),                               # does not fire
        (ONTOLOGY.upper() + b"#Q", RDF_TYPE, b"<f-upper>"),                         # fires
        (b"<" + ONTOLOGY + b"#z>", RDF_TYPE, b"<k-brackets>"),                      # never fires
        # (the filter reads the subject alone, so one node cannot have both filtered and unfiltered class triples; the nearest
        # case: its class is a class through another subject, and it is a plain node of an edge)
        (ONTOLOGY + b"#n", RDF_TYPE, b"<k-shared>"), (b"<m>", RDF_TYPE, b"<k-shared>"), (b"<m>", b"<knows>", ONTOLOGY + b"#n"),
    ]
    return b"".join(s + b" " + p + b" " + o + b" .\n" for s, p, o in rows)


def all_filtered_file() -> bytes:
    return b"".join(ONTOLOGY + b"#s%d " % i + RDF_TYPE + b" <c%d> .\n" % (i % 3) for i in range(7)) + b"<a> <p> <c0> .\n"


def labels_scale_file(seed: int = 0) -> bytes:
    """4,200 labelled nodes over 70 classes, three class triples per node (some the same class twice), every second node also
    the subject of an edge to an unlabelled node: node ids and label flags run past 2,048 and 4,096"""
    rng = random.Random(seed)
    out = []
    for i in range(4200):
        for _ in range(3):
            out.append(b"<n%05d> " % i + RDF_TYPE + b" <class%02d> .\n" % rng.randrange(70))
        if i % 2:
            out.append(b"<n%05d> <p> <m%05d> .\n" % (i, i))
    rng.shuffle(out)
    return b"".join(out)


# ---- past 2^31 ------------------------------------------------------------------------------------------------------------------
SLAB = 65536
NUM_SLABS = 65535                                    # 0xFFFF0000 bytes
REAL_SLABS = (0, 32767, 32768, 65534)                # the first, the one that ends at 2^31, the one that starts there, the last


def _pad_line(tag: int, length: int) -> bytes:
    """``<pad> <p> "z<tag>pp...p" .\\n`` of exactly ``length`` >= 21 bytes (21: a literal of 8); no other term starts with ``"z``, so
    the literal's place in the bytewise order is decided by its first 4 bytes, whatever its length"""
    head, tail = b'<pad> <p> "z%d' % tag, b'" .\n'
    assert 0 <= tag <= 9 and length >= 21
    return head + b"p" * (length - len(head) - len(tail)) + tail


def limit_slabs(twin: bool):
    """(padding slab, {slab index: real slab}).  The full file is NUM_SLABS slabs of SLAB bytes; ``twin``: the same slabs with every
    padding literal cut to 8 bytes.  A real slab holds short triple lines (one type triple, one upper-case spelling) and its own
    padding line; slabs 32,767 and 65,534 end in their short lines, and the last one without '\\n'."""
    def pad(tag, length):
        return _pad_line(tag, 21 if twin else length)

    real = {}
    for tag, k in enumerate(REAL_SLABS, 1):
        short = (b"<r%da> <q> <r%db> .\n" % (k, k) + b"<r%da> " % k + RDF_TYPE + b" <cls%d> .\n" % (k % 2) +
                 b"<R%dA> <Q> <pad> .\n" % k + b'<r%db> <q> "lit %d" .\n' % (k, k) + b"<r%db> <q> <r%da> ." % (k, k))
        if k == NUM_SLABS - 1:
            real[k] = pad(tag, SLAB - len(short)) + short
        elif k == 32767:
            real[k] = pad(tag, SLAB - len(short) - 1) + short + b"\n"
        else:
            real[k] = short + b"\n" + pad(tag, SLAB - len(short) - 1)
        assert twin or len(real[k]) == SLAB
    return pad(0, SLAB), real


def limit_twin() -> bytes:
    pad, real = limit_slabs(True)
    return b"".join(real.get(k, pad) for k in range(NUM_SLABS))


def is_pad_literal(name: bytes) -> bool:
    return name.startswith(b'"z')
