"""The byte-level reference (tests/ingest_bytes_reference.py) against the host loader wherever both are defined, hand-written
byte strings at the points where the two differ by design, the round count by its definition, and every input builder of the GPU
edge tests checked for the property its test relies on.  CPU only."""
import os

import numpy as np
import pytest

from scaling_rgcn_training_amd import graphs as G
from tests import ingest_bytes_reference as B
from tests import ingest_reference as R
from tests.conftest import GOLDEN_DIR

TEST_NT = os.path.join(GOLDEN_DIR, "TEST", "TEST_complete.nt")
DEGENERATE = (b"", b"\n\n\r\n\n", b"\n", b"<a> " + G.RDF_TYPE.encode() + b" <c> .\n<b> <type> <c> .\n", b"   .\n")


def _shared_files():
    with open(TEST_NT, "rb") as f:
        yield "toy", f.read()
    yield "generate0", R.generate(0)
    yield "generate1", R.generate(1)
    for n in (1, 682, 683, 2047, 2048, 2049):
        yield f"simple{n}", R.simple(n)
    for n in (2045, 2046, 2047):
        yield f"distinct{n}", R.simple(n, distinct_subjects=True)
    for i, d in enumerate(DEGENERATE):
        yield f"degenerate{i}", d


SHARED = list(_shared_files())


@pytest.mark.parametrize("name,data", SHARED, ids=[n for n, _ in SHARED])
def test_expected_equals_the_host_loader_where_both_are_defined(name, data):
    got, want = B.expected(data), R.expected(data)
    assert np.array_equal(got["edge_index"], want["edge_index"]) and np.array_equal(got["edge_type"], want["edge_type"])
    for k in ("nodes", "relations", "classes"):
        assert [t.decode("utf-8") for t in got[k]] == list(want[k]), k
    assert np.array_equal(got["labelled_idx"], want["labelled_idx"])
    assert got["labels"].shape == want["labels"].shape and np.array_equal(got["labels"], want["labels"])
    # tokens, sliced, folded and decoded, are split_triples
    tk = B.tokens(data)
    mine = [tuple(B.fold(data[o:o + n]).decode("utf-8") for o, n in tri) for tri in tk["occ"]]
    assert mine == G.split_triples(R.lines_of(data)) and tk["T"] == len(mine) == got["T"]
    assert tk["bad_line"] == 0 and tk["nul_line"] == 0
    assert tk["longest"] == max((len(t.encode()) for tri in mine for t in tri), default=0)
    assert got["U"] == len({t for tri in mine for t in tri}) and got["rounds"] <= tk["longest"] // 4 + 1


def test_lines_split_at_newline_only():
    assert B.lines(b"") == [] and B.lines(b"\n") == [(0, 0, 1)] and B.lines(b"a") == [(0, 1, 1)]
    assert B.lines(b"ab\r\ncd\r") == [(0, 2, 4), (4, 6, 7)]                 # one '\r' before '\n', one before the end of the file
    assert B.lines(b"ab\r\r\n") == [(0, 3, 5)]                              # only one
    assert B.lines(b"a\n\nb") == [(0, 1, 2), (2, 2, 3), (3, 4, 4)]


@pytest.mark.parametrize("sep", [b"\x0b", b"\x0c", b"\x1c", b"\xc2\x85", b"\xe2\x80\xa8", b"\r"],
                         ids=["vt", "ff", "fs", "nel", "u2028", "lone_cr"])
def test_a_separator_of_splitlines_stays_inside_its_line(sep):
    data = b"<s> <p> <o" + sep + b"x> .\n<a> <p> <b> .\n"
    assert len(B.lines(data)) == 2 and B.tokens(data)["T"] == 2
    assert b"<o" + sep + b"x>" in B.expected(data)["nodes"]
    if sep != b"\r":
        assert len(R.lines_of(data)) == 3                                   # the host loader breaks there: the documented gap


def test_non_ascii_capitals_are_not_folded():
    data = "<É> <p> <é> .\n".encode()
    assert B.fold("É".encode()) == "É".encode() and B.fold(b"AZ[@az") == b"az[@az"
    assert B.expected(data)["nodes"] == ["<É>".encode(), "<é>".encode()]
    assert len(R.expected(data)["nodes"]) == 1                              # the host loader's lower() merges them


def test_round_count_is_the_definitions():
    assert B.rounds_by_definition([b'"ab"', b'"ab"@en']) == 2 == B.rounds([b'"ab"', b'"ab"@en'])      # differ at byte 4
    a, b = b"0123456789abX", b"0123456789abY"                               # differ first at byte 12: round 3
    assert B.rounds_by_definition([a, b]) == 4 == B.rounds([a, b])
    assert B.rounds_by_definition([b"anything at all"]) == 1 == B.rounds([b"anything at all"])
    assert B.rounds_by_definition([]) == 0 == B.rounds([])
    assert B.expected(b"")["rounds"] == 0 and B.expected(b"<a> <a> <a> .\n")["rounds"] == 1
    # the linear form is the definition on every small builder
    for data in (B.prefix_file(), B.separators_file(), B.chain_file(), B.roles_file(), R.generate(0)[:20000].rsplit(b"\n", 1)[0]):
        terms = B.expected(data)["terms"]
        assert B.rounds(terms) == B.rounds_by_definition(terms)


# ---- the builders of tests/test_gpu_ingest_edges.py ------------------------------------------------------------------------------
@pytest.mark.parametrize("align", B.ALIGNMENTS)
def test_tokenizer_sweep_puts_the_spaces_where_it_says(align):
    data, starts = B.tokenizer_sweep(align)
    tk = B.tokens(data)
    assert tk["bad_line"] == 0 and tk["nul_line"] == 0 and tk["T"] == 2 * len(starts) == 2 * 72
    by_start = {tri[0][0]: tri for tri in tk["occ"]}
    seen = set()
    for s in starts:
        assert s % 64 == align
        (_, ls), (po, lp), (oo, lo) = by_start[s]
        sp1, sp2 = ls, po - s + lp
        assert data[s + sp1] == 32 and data[s + sp2] == 32 and lo in (0, 3)
        seen.add((sp1, sp2, lo))
    pairs = {(a, b) for a in B.SPACE_AT for b in B.SPACE_AT if a < b}
    assert seen == {(a, b, lo) for a, b in pairs for lo in (0, 3)}
    assert (63, 64) in pairs and (0, 1) in pairs and (62, 63) in pairs and (0, 129) in pairs     # lane 63 / lane 0; one piece; three
    assert len(data) < 300_000


def test_error_cases_are_refused_for_what_and_where_the_issue_says():
    cases = B.error_cases()
    assert sorted(cases) == sorted(B.ERRORS_EXPECTED)
    for name, data in cases.items():
        assert B.first_error(data) == B.ERRORS_EXPECTED[name], name
    tk = B.tokens(cases["above_2048"])
    assert tk["bad_line"] == 2500 and B.tokens(cases["above_2048"].replace(b"<a> <p> .\n", B.GOOD))["bad_line"] == 2900
    assert not cases["last_line_no_newline"].endswith(b"\n")
    assert B.tokens(cases["nul_after_malformed"])["nul_line"] == 3 and B.tokens(cases["two_nuls"])["nul_line"] == 3
    assert B.first_error(B.GOOD) is None


def test_sized_files_have_their_size_and_last_byte():
    loadable = 0
    for n in B.SIZES:
        for final_newline in (False, True):
            data = B.sized_file(n, final_newline)
            assert len(data) == n and (data[-1] == 10) == final_newline and b"\x00" not in data
            loadable += B.first_error(data) is None
    assert 10 <= loadable < 2 * len(B.SIZES)                 # both outcomes occur
    for name, data in B.nul_files():
        err = B.first_error(data)
        assert err is not None and (err[0] == "nul" or err[1] < B.tokens(data)["nul_line"]), name
        assert data.count(b"\x00") == 1
    at = {name: data.index(b"\x00") for name, data in B.nul_files()}
    assert at["at15"] == 15 and at["at4096"] == 4096 and at["n4096_last"] == 4095 and at["n17_first"] == 0
    assert dict(B.nul_files())["n4096_last_then_newline"].endswith(b"\x00\n")


def test_byte_files_hold_what_they_claim():
    data = B.all_bytes_file()
    terms = B.expected(data)["terms"]
    assert {b for t in terms for b in t} == set(B.TERM_BYTES) - set(range(65, 91)) and b"\r\n" not in data
    assert {b for b in data} >= set(B.TERM_BYTES)
    with pytest.raises(UnicodeDecodeError):
        data.decode("utf-8")
    exp = B.expected(B.prefix_file())
    terms = set(exp["terms"])
    assert b"" in terms and exp["terms"][:2] == [b"", b"\x01"]
    for k in range(8):
        p = b"wxyzwxyz"[:k]
        assert p + b"a" in terms and p + b"A" not in terms                    # 0x41 merged into 0x61
        got = [t for t in exp["terms"] if len(t) == k + 1 and t[:k] == p and t[k] in B.DECIDING]
        assert got == [p + bytes([v]) for v in (0x01, 0x5B, 0x61, 0x7F, 0x80, 0xC3, 0xFF)]       # unsigned order
    assert {len(t) for t in terms if t.startswith(b"q")} == set(B.PREFIX_LENGTHS)
    exp = B.expected(B.separators_file())
    assert len(B.lines(B.separators_file())) == len(B.SEPARATORS) + 4
    assert "<É>".encode() in exp["nodes"] and "<Σ>".encode() in exp["nodes"] and "<σ>".encode() in exp["nodes"]
    assert b"abc\xe2" in exp["nodes"] and b"abc\xe2\x82" in exp["nodes"] and exp["rounds"] >= 2


def test_rank_scale_file_keeps_the_rounds_busy():
    exp = B.expected(B.rank_scale_file())
    terms = exp["terms"]
    assert 6000 <= exp["U"] <= 7000 and exp["U"] - 1 >= 1 << 12                # sort_bits = 32 + 13 > 40
    for j in range(1, 10):
        assert sum(B.active_groups(terms, j)) == exp["U"] - 2 and len(B.active_groups(terms, j)) == 1     # all but <p> and <o>
    sizes = B.active_groups(terms, 10)
    assert len(sizes) >= 300 and sum(sizes) == exp["U"] - 2
    assert all(sizes.count(k) >= 1 for k in (1, 2, 3, 4, 2047, 2048, 2049))
    r11 = B.active_groups(terms, 11)                                          # every other group falls apart into single terms
    assert r11[-1] == 2049 and set(r11[:-1]) == {1} and len(r11) > 4096
    for j in (12, 13):
        assert B.active_groups(terms, j) == [2049]                            # the big group stays whole for three more rounds
    assert B.active_groups(terms, 14) == [1] * 2049 and exp["rounds"] == 15 <= exp["longest"] // 4 + 1
    assert sum(B.active_groups(terms, 3)) >= 2049 and len(B.active_groups(terms, 10)) >= 300
    chain = B.expected(B.chain_file())
    assert chain["longest"] == 70 and chain["rounds"] == 18 == chain["longest"] // 4 + 1
    assert all(b.startswith(a) for a, b in zip(chain["terms"][4:], chain["terms"][5:]))


@pytest.mark.parametrize("kind,where", [("length", None), ("last_byte_of_70", 69), ("byte_60", 60), ("byte_0", 0)])
def test_three_terms_differ_pairwise_only_where_they_say(kind, where):
    a, b, c = B.three_terms(kind)
    for x, y in ((a, b), (a, c), (b, c)):
        if where is None:
            assert len(x) != len(y) and set(x) == set(y) == {ord("v")} and [len(a), len(b), len(c)] == [72, 65, 64]     # heads first
        else:
            assert len(x) == len(y) == 70 and [i for i in range(70) if x[i] != y[i]] == [where]
    assert B.expected(B.term_lines([a, b, c]))["U"] == 3


def test_case_only_terms_and_the_six_terms():
    terms = B.three_terms("case")
    assert len(set(terms)) == 3 and len({B.fold(t) for t in terms}) == 1
    assert B.expected(B.term_lines(terms))["U"] == 1
    assert B.expected(B.term_lines(B.SIX_TERMS))["U"] == 6


def test_roles_and_label_files():
    exp = B.expected(B.roles_file())
    cls, nodes = exp["classes"], exp["nodes"]
    assert cls == [b"<all>", b"<c1>", b"<c2>", b"<c3>", b"<k-brackets>", b"<k-longer>", b"<k-shared>"]
    assert not any(c.startswith(b"<f-") for c in cls) and all(n in nodes for n in (b"<f-bare>", b"<f-upper>", b"<c4>"))
    assert b"<all>" in nodes and exp["relations"] == [b"<all>", b"<knows>"]
    lab = {nodes[i]: [cls[c] for c in np.flatnonzero(row)] for i, row in zip(exp["labelled_idx"], exp["labels"])}
    assert lab[b"<n1>"] == [b"<all>", b"<c1>"] and lab[b"<c1>"] == [b"<c2>"] and lab[b"<n3>"] == [b"<c3>"]
    assert lab[b"<m>"] == [b"<k-shared>"] and B.ONTOLOGY + b"#n" in nodes and B.ONTOLOGY + b"#n" not in lab
    assert B.ONTOLOGY + b"x#a" in lab and b"<" + B.ONTOLOGY + b"#z>" in lab and len(lab) == 6
    exp = B.expected(B.all_filtered_file())
    assert exp["classes"] == [] and exp["labels"].shape == (0, 0) and len(exp["labelled_idx"]) == 0
    assert all(b"<c%d>" % i in exp["nodes"] for i in range(3)) and len(exp["edge_type"]) == 2
    exp = B.expected(B.labels_scale_file())
    assert len(exp["labelled_idx"]) == 4200 and exp["labels"].shape == (4200, 70) and exp["T"] > 4096 * 3
    assert exp["labelled_idx"].max() > 4096 and len(exp["nodes"]) == 4200 + 2100 + 70
    per_node = exp["labels"].sum(1)
    assert per_node.min() >= 1 and per_node.max() == 3 and 2.8 < per_node.mean() < 3.0
    assert not np.array_equal(exp["labelled_idx"], np.arange(4200))           # unlabelled nodes in between


def test_limit_twin_ranks_every_padding_literal_as_the_full_file_does():
    pad_t, real_t = B.limit_slabs(True)
    pad_f, real_f = B.limit_slabs(False)
    assert len(pad_f) == B.SLAB and all(len(real_f[k]) == B.SLAB for k in B.REAL_SLABS) and sorted(real_f) == list(B.REAL_SLABS)
    assert B.NUM_SLABS * B.SLAB == 0xFFFF0000 and (B.REAL_SLABS[1] + 1) * B.SLAB == 1 << 31 == B.REAL_SLABS[2] * B.SLAB
    assert not real_f[B.NUM_SLABS - 1].endswith(b"\n") and pad_f.endswith(b"\n")
    # the distinct terms of the full file are those of its five different slabs
    full = B.expected(pad_f + b"".join(real_f[k] for k in B.REAL_SLABS[:-1]) + pad_f + real_f[B.REAL_SLABS[-1]])
    twin = B.expected(pad_t + b"".join(real_t[k] for k in B.REAL_SLABS[:-1]) + pad_t + real_t[B.REAL_SLABS[-1]])
    assert np.array_equal(full["edge_index"], twin["edge_index"]) and np.array_equal(full["labels"], twin["labels"])
    assert full["rounds"] == twin["rounds"] and full["U"] == twin["U"]
    pads = 0
    for f, t in zip(full["terms"], twin["terms"]):
        if B.is_pad_literal(f):
            pads += 1
            assert B.is_pad_literal(t) and len(t) == 8 and f[:7] == t[:7] and f.endswith(b'pppppp"') and len(f) > 65000
            others = [u for u in full["terms"] if u != f]
            assert max(B.common_prefix(f, u) for u in others) < 4 <= 8          # its rank is decided by its first 4 bytes
        else:
            assert f == t
    assert pads == 5
    whole = B.limit_twin()
    exp = B.expected(whole)
    assert len(whole) < 1_500_000 and exp["T"] == B.NUM_SLABS - 4 + 4 * 6 and exp["U"] == full["U"]
