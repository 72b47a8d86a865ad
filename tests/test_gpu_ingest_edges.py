"""The ingest kernels (csrc/rgcn_ingest.hip) where tests/test_gpu_ingest.py stops, against the byte-level reference
(tests/ingest_bytes_reference.py; its builders are checked in tests/test_ingest_bytes_reference.py).  Every comparison is exact:
occurrence offsets and lengths, T, the longest term, line numbers of refusals, U, the round count, ids, edges, labels and the bytes
the term tables point at.

a. the tokenizer's ballot loop with the two spaces at lanes 0 / 1 / 62 / 63 of one, two or three 64-byte pieces, lines that start
   at 0, 1 and 63 mod 64; which line a refusal names.
b. the byte passes: 15 file sizes around 16, 32, 4,096 and 8,192 x last byte '\\n' or not x 4 base alignments; a NUL at lane,
   block and file edges.
c. bytes the host loader cannot follow: every byte value, unsigned order at each position of a round's word, separators of
   ``splitlines()``, unfolded non-ASCII capitals, invalid UTF-8.
d. rank rounds with ~6,900 active terms for ten rounds, 300+ groups, a group of 2,049 tied for three rounds more; a chain of
   proper prefixes that needs every round the bound allows.
e. verification forced by pigeonhole (``hash_bits = 1`` and three terms): differences in length, past byte 64, in lane 7's piece,
   in byte 0 are collisions; a difference in case is none.
f. roles, the literal class filter, label scans past 2,048 and 4,096."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import ingest_bytes_reference as B

pytestmark = pytest.mark.gpu


def _ingest():
    from scaling_rgcn_training_amd import ingest
    return ingest


def _dev(data: bytes, base: int = 0) -> torch.Tensor:
    """the bytes on the device, ``base`` bytes past an aligned allocation"""
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    return torch.cat([torch.zeros(base, dtype=torch.uint8), src]).cuda()[base:]


def _num_lines(text: torch.Tensor) -> int:
    """rgcn_nt_lines, as ``ingest.tokenize`` calls it"""
    from scaling_rgcn_training_amd import _lib
    lib, n = _lib.load(), int(text.shape[0])
    nb = lib.rgcn_nt_lines_workspace_bytes(n)
    ws = torch.empty(nb, dtype=torch.uint8, device=text.device)
    lines = C.c_int64(0)
    _lib.check(lib.rgcn_nt_lines(text.data_ptr(), n, ws.data_ptr(), nb, C.byref(lines), _lib._stream(text)), "rgcn_nt_lines")
    return int(lines.value)


def _u32(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def _assert_tokens(text: torch.Tensor, data: bytes):
    tk = B.tokens(data)
    occ_off, occ_len, t, longest = _ingest().tokenize(text)
    assert (t, longest) == (tk["T"], tk["longest"])
    flat = [pair for tri in tk["occ"] for pair in tri]
    assert _u32(occ_off).tolist() == [o for o, _ in flat] and _u32(occ_len).tolist() == [n for _, n in flat]
    return occ_off, occ_len, t, longest


def _names(data: bytes, off: np.ndarray, length: np.ndarray):
    assert (off + length <= len(data)).all()
    return [B.fold(data[o:o + n]) for o, n in zip(off.tolist(), length.tolist())]


def _assert_emitted(data: bytes, exp: dict, counts, emitted):
    edge_index, edge_type, labelled_idx, labels, tabs = emitted
    assert [int(c) for c in counts[:6]] == [exp["U"], len(exp["nodes"]), len(exp["relations"]), len(exp["classes"]),
                                            len(exp["edge_type"]), len(exp["labelled_idx"])]
    assert np.array_equal(edge_index.cpu().numpy(), exp["edge_index"]) and np.array_equal(edge_type.cpu().numpy(), exp["edge_type"])
    assert np.array_equal(labelled_idx.cpu().numpy(), exp["labelled_idx"])
    assert labels.shape == exp["labels"].shape and np.array_equal(labels.cpu().numpy(), exp["labels"])
    for i, k in enumerate(("nodes", "relations", "classes")):
        assert _names(data, tabs[2 * i], tabs[2 * i + 1]) == exp[k], k


def _build_and_check(data: bytes, exp: dict, base: int = 0):
    """tokenize -> build -> emit through the Python wrappers of the four ABI calls; returns the build's counts"""
    ingest = _ingest()
    text = _dev(data, base)
    occ_off, occ_len, t, longest = _assert_tokens(text, data)
    st, counts, ws = ingest.build(text, occ_off, occ_len, t, longest, 64, 0)
    assert st == 0
    _assert_emitted(data, exp, counts, ingest.emit(text, t, counts, ws))
    assert int(counts[7]) == exp["rounds"] <= exp["longest"] // 4 + 1
    return counts


def _assert_graph(g, data: bytes, exp: dict):
    """an NTGraph of ``load_nt``: tensors, table bytes, and names that survive ``surrogateescape`` both ways"""
    assert np.array_equal(g.edge_index.cpu().numpy(), exp["edge_index"]) and np.array_equal(g.edge_type.cpu().numpy(), exp["edge_type"])
    assert g.num_nodes == len(exp["nodes"]) and g.num_relations == 2 * len(exp["relations"])
    assert np.array_equal(g.labelled_idx.cpu().numpy(), exp["labelled_idx"])
    assert g.labels.shape == exp["labels"].shape and np.array_equal(g.labels.cpu().numpy(), exp["labels"])
    for table, k in ((g.nodes, "nodes"), (g.relations, "relations"), (g.classes, "classes")):
        assert _names(data, table.offset, table.length) == exp[k], k
        names = table.names()
        assert [n.encode("utf-8", errors="surrogateescape") for n in names] == exp[k], k
        assert [table.index(n) for n in names] == list(range(len(names))), k


def _assert_refused(source, err):
    kind, line = err
    with pytest.raises(ValueError) as e:
        _ingest().load_nt(source)
    msg = str(e.value)
    assert msg.startswith(f"line {line}:") and ("NUL" in msg) == (kind == "nul"), (msg, err)


# ---- a. tokenizer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", B.ALIGNMENTS)
def test_tokenizer_finds_the_two_spaces_at_every_lane_edge(align):
    data, _ = B.tokenizer_sweep(align)
    text = _dev(data)
    assert _num_lines(text) == len(B.lines(data))
    _assert_tokens(text, data)


def test_tokenizer_sweep_from_a_misaligned_base_and_through_the_whole_build():
    data, _ = B.tokenizer_sweep(63)
    _assert_tokens(_dev(data, 1), data)
    _build_and_check(data, B.expected(data), base=8)


@pytest.mark.parametrize("name", sorted(B.ERRORS_EXPECTED))
def test_refusals_name_the_first_offending_line(name):
    data = B.error_cases()[name]
    assert B.first_error(data) == B.ERRORS_EXPECTED[name]
    _assert_refused(data, B.ERRORS_EXPECTED[name])


# ---- b. byte passes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", B.SIZES)
def test_byte_passes_at_every_size_last_byte_and_base(n):
    ingest = _ingest()
    for final_newline in (False, True):
        data = B.sized_file(n, final_newline)
        err = B.first_error(data)
        exp = None if err else B.expected(data)
        for base in B.BASES:
            text = _dev(data, base)
            assert text.data_ptr() % 16 == base
            assert _num_lines(text) == len(B.lines(data)), (n, final_newline, base)
            if err:
                _assert_refused(text, err)
            else:
                _assert_tokens(text, data)
                _assert_graph(ingest.load_nt(text), data, exp)


def test_a_nul_at_lane_block_and_file_edges_names_its_line():
    for name, data in B.nul_files():
        for base in (0, 1):
            text = _dev(data, base)
            assert _num_lines(text) == len(B.lines(data)), name
            _assert_refused(text, B.first_error(data))


# ---- c. bytes beyond graphs.Graph -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [B.all_bytes_file, B.prefix_file, B.separators_file], ids=["all_bytes", "prefixes", "separators"])
def test_bytewise_contract_where_the_host_loader_cannot_follow(builder):
    data = builder()
    exp = B.expected(data)
    _build_and_check(data, exp)
    _assert_graph(_ingest().load_nt(data), data, exp)


# ---- d. rank rounds -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rank_scale():
    data = B.rank_scale_file()
    return data, B.expected(data)


def test_rank_rounds_with_thousands_of_active_terms_and_hundreds_of_groups():
    data, exp = _rank_scale()
    counts = _build_and_check(data, exp)
    assert int(counts[0]) == exp["U"] > 4096 and int(counts[7]) == 15


def test_rank_rounds_on_a_chain_of_proper_prefixes():
    data = B.chain_file()
    exp = B.expected(data)
    counts = _build_and_check(data, exp)
    assert int(counts[7]) == 18 == exp["longest"] // 4 + 1


# ---- e. verification ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["length", "last_byte_of_70", "byte_60", "byte_0"])
def test_one_hash_bit_and_three_terms_must_collide(kind):
    ingest = _ingest()
    data = B.term_lines(B.three_terms(kind))
    text = _dev(data)
    occ_off, occ_len, t, longest = _assert_tokens(text, data)
    for seed in range(4):
        st, counts, _ = ingest.build(text, occ_off, occ_len, t, longest, 1, seed)
        assert st == ingest.ERR_COLLISION, (kind, seed)
    _build_and_check(data, B.expected(data))


def test_spellings_that_differ_in_case_are_one_term_not_a_collision():
    ingest = _ingest()
    data = B.term_lines(B.three_terms("case"))
    exp = B.expected(data)
    text = _dev(data)
    occ_off, occ_len, t, longest = _assert_tokens(text, data)
    for seed in range(4):
        st, counts, ws = ingest.build(text, occ_off, occ_len, t, longest, 1, seed)
        assert st == 0 and int(counts[0]) == 1 == exp["U"]
        _assert_emitted(data, exp, counts, ingest.emit(text, t, counts, ws))


def test_six_terms_collide_or_give_the_exact_tensors():
    ingest = _ingest()
    data = B.term_lines(B.SIX_TERMS)
    exp = B.expected(data)
    text = _dev(data)
    occ_off, occ_len, t, longest = _assert_tokens(text, data)
    tally = {}
    for bits in range(2, 9):
        for seed in range(8):
            st, counts, ws = ingest.build(text, occ_off, occ_len, t, longest, bits, seed)
            assert st in (0, ingest.ERR_COLLISION)
            if st == 0:
                _assert_emitted(data, exp, counts, ingest.emit(text, t, counts, ws))
            tally[bits] = tally.get(bits, 0) + (st == 0)
    print("\nbuilds without a collision, of 8 seeds, by hash bits:", tally)
    assert tally[2] == 0                                  # six terms, four values
    assert sum(tally.values()) >= 1                       # a hash that spreads: all 8 seeds colliding at 8 bits is below 1e-9


# ---- f. roles and labels --------------------------------------------------------------------------------------------------------
def test_roles_and_the_literal_class_filter():
    data = B.roles_file()
    exp = B.expected(data)
    _build_and_check(data, exp)
    g = _ingest().load_nt(data)
    _assert_graph(g, data, exp)
    assert g.classes.index("<f-two-hashes>") == -1 and g.classes.index("<k-longer>") >= 0 and g.nodes.index("<f-two-hashes>") >= 0


def test_every_class_triple_filtered():
    data = B.all_filtered_file()
    exp = B.expected(data)
    counts = _build_and_check(data, exp)
    assert int(counts[3]) == 0 and int(counts[5]) == 0
    g = _ingest().load_nt(data)
    _assert_graph(g, data, exp)
    assert g.labels.shape == (0, 0) and len(g.classes) == 0 and g.nodes.index("<c1>") >= 0


def test_label_scans_past_2048_and_4096_and_rows_wider_than_a_wave():
    data = B.labels_scale_file()
    exp = B.expected(data)
    counts = _build_and_check(data, exp)
    assert int(counts[5]) == 4200 and int(counts[3]) == 70
