"""The oracle of the GPU ingest tests (tests/ingest_reference.py) against what is already pinned -- the golden arrays of the toy
graph and ``graphs.Dataset`` -- and the host half of ``ingest``: ``TermTable`` and the refusals that need no device.  CPU only."""
import os

import numpy as np
import pytest
import torch

from scaling_rgcn_training_amd import graphs as G
from scaling_rgcn_training_amd import ingest
from tests import ingest_reference as R
from tests.conftest import GOLDEN_DIR, load_golden

TEST_NT = os.path.join(GOLDEN_DIR, "TEST", "TEST_complete.nt")


def test_expected_matches_the_golden_arrays_and_the_dataset():
    exp = R.expected(TEST_NT)
    z = load_golden("test_l1")
    assert np.array_equal(exp["edge_index"], z["edge_index"]) and np.array_equal(exp["edge_type"], z["edge_type"])
    d = G.Dataset(TEST_NT)
    d.init_dataset()
    assert exp["classes"] == list(d.enum_classes) and exp["nodes"] == d.orgGraph.nodes
    assert exp["relations"] == list(d.orgGraph.relations) and len(exp["nodes"]) == 12 and len(exp["relations"]) == 2
    td = d.orgGraph.training_data
    assert sorted(torch.cat([td.x_train, td.x_val, td.x_test]).tolist()) == exp["labelled_idx"].tolist()
    assert exp["labels"].tolist() == [[1]] * 3
    # line 8 ends in two spaces and a dot: its object keeps one of them
    assert any(n.endswith(" ") for n in exp["nodes"])


def test_generator_is_deterministic_and_seeded():
    assert R.generate(0) == R.generate(0) and R.generate(0) != R.generate(1)
    assert R.simple(50) == R.simple(50) and R.simple(50, True) == R.simple(50, True)


def test_generator_emits_every_case():
    data = R.generate(0)
    got = R.features(data)
    assert sorted(got) == sorted(R.FEATURES)
    assert all(got.values()), [k for k, v in got.items() if not v]
    exp = R.expected(data)
    assert 1900 <= len(G.split_triples(R.lines_of(data))) <= 2100 and 300 <= len(exp["nodes"]) <= 450
    assert b"\x00" not in data and len(exp["classes"]) == 4                     # the class of the ontology subject is filtered
    assert "<http://swrc.ontoware.org/ontology#onlyonontologysubjects>" in exp["nodes"]
    assert exp["labels"].sum(1).max() >= 2 and exp["labels"].min() == 0
    # a term in angle brackets never matches the filter, whatever its namespace
    tri = [("<http://swrc.ontoware.org/ontology#x>", G.RDF_TYPE, "<c>")]
    assert G.get_classes(tri) == ["<c>"]


def test_simple_files_have_the_sizes_the_edge_cases_need():
    for n in (1, 682, 683, 2047, 2048, 2049):
        data = R.simple(n)
        assert data.count(b"\n") == n and len(R.expected(data)["edge_type"]) == 2 * n
    for n in (2045, 2047):
        assert len(R.expected(R.simple(n, True))["nodes"]) == n + 1            # + <p>: n + 2 distinct terms


def _table(names):
    blob = " ".join(names).encode("utf-8", errors="surrogateescape")
    off, pos = [], 0
    for n in names:
        off.append(pos)
        pos += len(n.encode("utf-8", errors="surrogateescape")) + 1
    length = [len(n.encode("utf-8", errors="surrogateescape")) for n in names]
    return ingest.TermTable(np.frombuffer(blob, dtype=np.uint8), np.asarray(off), np.asarray(length))


def test_term_table_names_index_and_lookup():
    names = sorted(['"ab"', '"ab"@en', "<A/Upper>", "<b>", "x", '"grüße"', "<zz" + "z" * 300 + ">"], key=lambda s: s.lower().encode())
    t = _table(names)
    assert len(t) == len(names)
    assert t.names() == [n.lower() for n in names]                    # ASCII folding of the stored bytes
    assert t.names([2, 0]) == [names[2].lower(), names[0].lower()]
    assert t.names(torch.tensor([1])) == [names[1].lower()]
    for i, n in enumerate(t.names()):
        assert t.index(n) == i
    assert t.index("<absent>") == -1 and t.index("") == -1 and t.index("~") == -1
    assert t.lookup([names[3].lower(), "<absent>"]).tolist() == [3, -1]
    assert t.lookup([]).dtype == torch.int64
    with pytest.raises(IndexError):
        t.names([len(names)])
    empty = ingest.TermTable(np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    assert len(empty) == 0 and empty.names() == [] and empty.index("x") == -1
    # bytes that are not UTF-8 survive the round trip
    raw = ingest.TermTable(np.frombuffer(b"\xff\xfeX", dtype=np.uint8), np.asarray([0]), np.asarray([3]))
    assert raw.index(raw.names()[0]) == 0


def test_load_nt_refuses_a_cpu_device_and_bad_sources():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.load_nt(TEST_NT, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.load_nt(b"<a> <b> <c> .\n", device=torch.device("cpu"))
    with pytest.raises(ValueError):
        ingest.load_nt(torch.zeros(4, dtype=torch.int64), device="cuda")
    with pytest.raises(ValueError):
        ingest.load_nt(12, device="cuda")


def test_first_attempt_hash_bits_are_whole_sort_passes():
    for n in (0, 1, 3, 6000, 3_000_000, 0xFFFF0000):
        b = ingest._hash_bits(n)
        assert b % 8 == 0 and 8 <= b <= 64 and (b == 64 or 2 ** b >= 64 * max(n, 2) ** 2)
    assert ingest._hash_bits(6000) < ingest._hash_bits(3_000_000) <= 64
