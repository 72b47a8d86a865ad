"""The builders' workspace and index sizes are part of the C ABI: callers allocate by them, and a build refuses a buffer one byte
short.  tests/golden/workspace_bytes.json pins them, argument tuple by argument tuple, at the edges where a term of a carve
switches: no and one edge, one key short of / exactly / one key over a 2,048-key sort segment, node counts that outgrow the
edge count (the scan length follows the nodes), 1 and 65,536 relations, the three summary directions, fan-out -1 and 256, and
arguments that must be refused with 0.  CPU only: the size queries touch no device.

The file was recorded from the library as it stood before the carves moved onto rgcn_sort_scan.h's Arena; run this module as a
script (python tests/test_workspace_bytes.py) to re-record the byte counts of the tuples in it from the library in the tree --
only when a size is meant to change."""
import json
import os

import pytest

from scaling_rgcn_training_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_bytes.json")
FUNCTIONS = ["rgcn_plan_workspace_bytes", "rgcn_summary_workspace_bytes", "rgcn_sample_index_workspace_bytes",
             "rgcn_sample_hop_workspace_bytes", "rgcn_mb_index_bytes", "rgcn_mb_index_workspace_bytes"]


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_every_size_function():
    g = _golden()
    assert sorted(g) == sorted(FUNCTIONS)
    for name in FUNCTIONS:
        assert len(g[name]) >= 12, name
        assert any(want == 0 for _, want in g[name]), name          # a refusal
        assert any(want > 0 for _, want in g[name]), name


@pytest.mark.parametrize("name", FUNCTIONS)
def test_sizes_match_the_recorded_bytes(name):
    fn = getattr(_lib.load(), name)
    got = [[args, int(fn(*args))] for args, _ in _golden()[name]]
    assert got == _golden()[name]


@pytest.mark.parametrize("name", FUNCTIONS)
def test_sizes_are_whole_256_byte_pieces(name):
    assert all(want % 256 == 0 for _, want in _golden()[name])


if __name__ == "__main__":
    lib = _lib.load()
    rec = {name: [[args, int(getattr(lib, name)(*args))] for args, _ in cases] for name, cases in _golden().items()}
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(n) + ": [\n" + ",\n".join("  " + json.dumps(c) for c in rec[n]) + "\n]" for n in FUNCTIONS)
                + "\n}\n")
