"""``ingest.load_nt`` on the GPU against the repository's host loader (tests/ingest_reference.py ``expected``), bit for bit: the
toy graph, a generated file with every case the device path has to get right, the sizes at which a sort segment, a scan block or a
byte block fills up, degenerate files, refusals, a forced hash collision, and the way into ``TensorDataset`` / ``Trainer``."""
import functools
import os

import numpy as np
import pytest
import torch

from scaling_rgcn_training_amd import graphs as G
from tests import ingest_reference as R
from tests.conftest import GOLDEN_DIR, load_golden

pytestmark = pytest.mark.gpu
TEST_NT = os.path.join(GOLDEN_DIR, "TEST", "TEST_complete.nt")


def _ingest():
    from scaling_rgcn_training_amd import ingest
    return ingest


@functools.lru_cache(maxsize=None)
def _generated():
    data = R.generate(0)
    return data, R.expected(data)


def _assert_equal(g, exp):
    assert g.edge_index.dtype == torch.int64 and g.edge_type.dtype == torch.int64 and g.edge_index.is_cuda
    assert g.edge_index.shape == (2, len(exp["edge_type"])) and g.edge_index.is_contiguous()
    assert np.array_equal(g.edge_index.cpu().numpy(), exp["edge_index"])
    assert np.array_equal(g.edge_type.cpu().numpy(), exp["edge_type"])
    assert g.num_nodes == len(exp["nodes"]) and g.num_relations == 2 * len(exp["relations"])
    assert g.nodes.names() == exp["nodes"]
    assert g.relations.names() == exp["relations"]
    assert g.classes.names() == exp["classes"]
    assert g.labelled_idx.dtype == torch.int64 and g.labels.dtype == torch.int64
    assert np.array_equal(g.labelled_idx.cpu().numpy(), exp["labelled_idx"])
    assert g.labels.shape == exp["labels"].shape and np.array_equal(g.labels.cpu().numpy(), exp["labels"])


def test_toy_graph_matches_the_golden_arrays_and_the_host_loader():
    g = _ingest().load_nt(TEST_NT)
    z = load_golden("test_l1")
    assert g.num_nodes == 12 and g.num_relations == 2 * 2 and g.edge_type.shape[0] == 14
    assert np.array_equal(g.edge_index.cpu().numpy(), z["edge_index"]) and np.array_equal(g.edge_type.cpu().numpy(), z["edge_type"])
    host = G.Graph("host")
    host.init_graph(G.parse_graph_nt(TEST_NT))
    assert g.nodes.names() == host.nodes and g.relations.names() == list(host.relations)
    for i, n in enumerate(host.nodes):
        assert g.nodes.index(n) == i
    assert g.nodes.index("<absent>") == -1 and g.relations.index(host.nodes[0]) == -1
    assert g.nodes.lookup([host.nodes[3], "nope"]).tolist() == [3, -1]
    _assert_equal(g, R.expected(TEST_NT))


@pytest.mark.parametrize("source", ["bytes", "tensor", "cuda_tensor", "path"])
def test_generated_file_with_every_case(source, tmp_path):
    data, exp = _generated()
    if source == "path":
        p = tmp_path / "generated.nt"
        p.write_bytes(data)
        src = str(p)
    elif source == "bytes":
        src = data
    else:
        src = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        if source == "cuda_tensor":
            src = torch.cat([torch.zeros(3, dtype=torch.uint8), src]).cuda()[3:]          # a base that is not 16-byte aligned
    _assert_equal(_ingest().load_nt(src), exp)


@pytest.mark.parametrize("kind,n", [("lines", 1), ("lines", 2047), ("lines", 2048), ("lines", 2049), ("triples", 682),
                                    ("triples", 683), ("terms", 2045), ("terms", 2047), ("terms", 2046)])
def test_segment_and_scan_edges(kind, n):
    """2,048 is the keys of a sort segment and the elements of a scan block (rgcn_sort_scan.h): line counts around it (the scans
    over lines and triples), 3 x 682 = 2,046 and 3 x 683 = 2,049 occurrences, and n + 2 = 2,047 / 2,048 / 2,049 distinct terms"""
    data = R.simple(n, distinct_subjects=kind == "terms")
    g = _ingest().load_nt(data)
    _assert_equal(g, R.expected(data))
    assert g.edge_type.shape[0] == 2 * n and g.labels.shape == (0, 0)


def test_blank_lines_between_triples_and_a_4096_byte_block_edge():
    """'\\n' bytes as the last byte of one 4,096-byte block and the first of the next; lines of 1 and 2 bytes are skipped"""
    line = b"<a> <p> <b> .\n"
    pad = 4096 - 2 * len(line) - 1
    data = line + b"\n" * pad + line + b"\n\n" + b".\n" + b" .\n" + b"<c> <p> <a> ."
    assert data[4095:4097] == b"\n\n"
    _assert_equal(_ingest().load_nt(data), R.expected(data))


@pytest.mark.parametrize("data", [b"", b"\n\n\r\n\n", b"\n", b"<a> " + G.RDF_TYPE.encode() + b" <c> .\n<b> <type> <c> .\n"],
                         ids=["empty", "blank_lines", "one_newline", "type_triples_only"])
def test_degenerate_files(data):
    g = _ingest().load_nt(data)
    exp = R.expected(data)
    assert g.edge_index.shape == (2, 0) and g.edge_type.shape == (0,) and g.num_relations == 0
    _assert_equal(g, exp)
    if data.startswith(b"<a>"):
        assert g.num_nodes == 3 and g.labelled_idx.tolist() == [0] and g.labels.tolist() == [[1]] and g.classes.names() == ["<c>"]
    else:
        assert g.num_nodes == 0 and len(g.nodes) == 0 and g.labels.shape == (0, 0)


def test_refusals():
    ingest = _ingest()
    good = b"<a> <p> <b> .\n"
    with pytest.raises(ValueError, match="line 3"):
        ingest.load_nt(good + b"\n" + b"<a> <p>.\n" + good + b"<a>  \n")
    with pytest.raises(ValueError, match="line 2.*NUL"):
        ingest.load_nt(good + b"<a> <p> <\x00> .\n" + b"<a> <p>.\n")
    with pytest.raises(ValueError, match="line 1"):
        ingest.load_nt(b"<a> <p>.\n" + b"<a> <p> <\x00> .\n")
    with pytest.raises(ValueError, match="line 2.*NUL"):
        ingest.load_nt(good + b"\x00\n" + good)                       # in a line that would be skipped
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.load_nt(good, device="cpu")
    # a lone dot and two spaces: three empty terms, as the host loader reads it
    data = b"   .\n"
    _assert_equal(ingest.load_nt(data), R.expected(data))


def test_forced_collision_through_the_abi_and_the_retry(monkeypatch):
    ingest = _ingest()
    data, exp = _generated()
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    occ_off, occ_len, t, max_len = ingest.tokenize(text)
    assert t == len(exp["edge_type"]) // 2 + sum(1 for _, p, _ in G.split_triples(R.lines_of(data)) if p in G.TYPE_PREDICATES)
    st, counts, _ = ingest.build(text, occ_off, occ_len, t, max_len, 4, 0)
    assert st == ingest.ERR_COLLISION == -12
    torch.cuda.synchronize()
    st, counts, _ = ingest.build(text, occ_off, occ_len, t, max_len, 64, 0)
    assert st == 0 and counts[1] == len(exp["nodes"]) and counts[4] == len(exp["edge_type"])
    tried = []
    first = ingest._hash_bits
    monkeypatch.setattr(ingest, "_hash_bits", lambda n: tried.append(first(n)) or 4)
    _assert_equal(ingest.load_nt(data), exp)
    assert len(tried) == 1


def test_ids_do_not_depend_on_the_hash():
    ingest = _ingest()
    data, exp = _generated()
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    occ_off, occ_len, t, max_len = ingest.tokenize(text)
    seen = set()
    for bits, seed in ((64, 0), (64, 5), (40, 1), (33, 2)):
        st, counts, _ = ingest.build(text, occ_off, occ_len, t, max_len, bits, seed)
        assert st == 0
        seen.add(tuple(counts[:6]))
    assert len(seen) == 1


def test_end_to_end_into_the_trainer():
    from scaling_rgcn_training_amd import summaries
    from scaling_rgcn_training_amd.trainer import Trainer
    g = _ingest().load_nt(TEST_NT)
    data = g.dataset()
    sg = data.add_summary(k=1)
    host = G.Graph("host")
    host.init_graph(G.parse_graph_nt(TEST_NT))
    td = host.training_data
    want = summaries.node_partition(td.edge_index.cuda(), td.edge_type.cuda(), host.num_nodes, 2 * len(host.relations), k=1)
    assert int(want.num_blocks) == sg.num_nodes and torch.equal(want.block, sg.org_block)
    trainer = Trainer(data, 8, 2, 8, 0.01, 0.0005, verbose=False, hipgraph=False)
    trainer.train_summaries({"dataset": "TEST", "num_sums": 1, "e_trans": True, "e_freeze": False, "w_trans": True, "w_grad": True})
    assert sg.embedding.shape == (sg.num_nodes, 8) and sg.embedding.is_cuda and torch.isfinite(sg.embedding).all()
