"""The ingest's 32-bit offsets with bit 31 set and at the limit: one text of exactly 0xFFFF0000 bytes, built on the device from
65,535 slabs of 65,536 bytes (tests/ingest_bytes_reference.py ``limit_slabs``).  All but four slabs are one padding line with a
literal of 65,519 bytes; the four real slabs -- the first, the one that ends at byte 2^31, the one that starts there, and the last,
which ends without '\\n' at byte 0xFFFF0000 - 1 -- hold short triples.  Expected values come from the byte-level reference on the
TWIN file (the same slabs, every padding literal cut to 8 bytes; tests/test_ingest_bytes_reference.py shows that the cut keeps every
literal's rank): ids, edges, labels, every count and the round count are the twin's, exactly.  One byte more is refused before any
launch.  The case's time is the 4 GiB device -> host copy ``load_nt`` makes for the term tables; it prints its peak device memory."""
import gc

import numpy as np
import pytest
import torch

from tests import ingest_bytes_reference as B

pytestmark = pytest.mark.gpu
LIMIT = 0xFFFF0000


def _release():
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _fresh_memory():
    _release()
    torch.cuda.reset_peak_memory_stats()
    yield
    print(f"\npeak device memory: {torch.cuda.max_memory_allocated() / 1e9:.1f} GB")
    _release()


def _device_text() -> torch.Tensor:
    pad, real = B.limit_slabs(False)
    dev = torch.device("cuda")
    text = torch.empty(B.NUM_SLABS, B.SLAB, dtype=torch.uint8, device=dev)
    text.copy_(torch.frombuffer(bytearray(pad), dtype=torch.uint8).to(dev))            # (broadcast over the slabs)
    for k, slab in real.items():
        text[k].copy_(torch.frombuffer(bytearray(slab), dtype=torch.uint8).to(dev))
    return text.view(-1)


def test_a_text_of_exactly_the_limit_against_its_short_twin():
    from scaling_rgcn_training_amd import ingest
    twin = B.limit_twin()
    exp = B.expected(twin)
    text = _device_text()
    assert text.shape[0] == LIMIT == ingest.MAX_BYTES

    # the tokenizer: occurrence offsets past 2^31 and in the last slab; lengths are the twin's but for the padding literals
    occ_off, occ_len, t, longest = ingest.tokenize(text)
    assert t == exp["T"] and longest == B.SLAB - len(b'<pad> <p>  .\n')
    off, length = occ_off.cpu().numpy().view(np.uint32).astype(np.int64), occ_len.cpu().numpy().view(np.uint32).astype(np.int64)
    assert (off + length <= LIMIT).all() and (np.diff(off) > 0).all()
    assert (off >= 1 << 31).any() and (off >= 0xFFFE0000).any() and int((off + length).max()) == LIMIT - 2
    twin_len = np.asarray([n for tri in B.tokens(twin)["occ"] for _, n in tri], dtype=np.int64)
    assert ((length == twin_len) | ((twin_len == 8) & (length > 65000))).all()

    st, counts, ws = ingest.build(text, occ_off, occ_len, t, longest, 64, 0)
    assert st == 0
    want = [exp["U"], len(exp["nodes"]), len(exp["relations"]), len(exp["classes"]), len(exp["edge_type"]), len(exp["labelled_idx"])]
    assert [int(c) for c in counts[:6]] == want and int(counts[7]) == exp["rounds"]
    del ws, occ_off, occ_len
    _release()

    g = ingest.load_nt(text)
    assert np.array_equal(g.edge_index.cpu().numpy(), exp["edge_index"]) and np.array_equal(g.edge_type.cpu().numpy(), exp["edge_type"])
    assert g.num_nodes == len(exp["nodes"]) and g.num_relations == 2 * len(exp["relations"])
    assert np.array_equal(g.labelled_idx.cpu().numpy(), exp["labelled_idx"])
    assert g.labels.shape == exp["labels"].shape and np.array_equal(g.labels.cpu().numpy(), exp["labels"])
    pads = 0
    for table, k in ((g.nodes, "nodes"), (g.relations, "relations"), (g.classes, "classes")):
        assert len(table) == len(exp[k]) and table.offset.dtype == np.int64
        assert (table.offset >= 0).all() and (table.offset + table.length <= LIMIT).all()
        for i, name in enumerate(exp[k]):
            o, n = int(table.offset[i]), int(table.length[i])
            if B.is_pad_literal(name):
                pads += 1
                assert n > 65000 and table.text[o:o + 8].tobytes() == name[:7] + b"p"
                assert table.text[o + n - 8:o + n].tobytes() == b'ppppppp"'
            else:
                assert B.fold(table.text[o:o + n].tobytes()) == name, (k, i)
    assert pads == 5
    assert (g.nodes.offset >= 1 << 31).any() and (g.nodes.offset >= 0xFFFE0000).any()
    assert g.nodes.index("<r65534a>") >= 0 and g.nodes.names([g.nodes.index("<r32768b>")]) == ["<r32768b>"]


def test_one_byte_past_the_limit_is_refused_before_any_launch():
    from scaling_rgcn_training_amd import ingest
    text = torch.empty(LIMIT + 1, dtype=torch.uint8, device="cuda")         # (never read: its bytes do not matter)
    with pytest.raises(ValueError, match=str(LIMIT)):
        ingest.tokenize(text)
