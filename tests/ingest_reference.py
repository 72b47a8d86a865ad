"""What ``ingest.load_nt`` must give, from the repository's own host loader: a seeded generator of ``.nt`` bytes with every case the
device path has to get right, and ``expected`` -- ``graphs.Graph.init_graph`` + ``graphs.get_classes`` + ``graphs.nodes2type_mapping``
on the same bytes.  The generated files hold nothing on which the two loaders differ by design (characters that Unicode ``lower()``
changes and ASCII folding does not; the extra separators of ``splitlines()``)."""
import random

import numpy as np

from scaling_rgcn_training_amd import graphs as G

PREFIX = "<http://www.Example-University.org/Publications/viewPublicationOWL/"       # 67 bytes shared: 16 rounds before a difference
ONTO = "<http://swrc.ontoware.org/ontology#"
LENGTHS = (1, 7, 8, 9, 255, 256, 257, 5003)
DIFF_AT = (11, 12, 13, 31, 32, 33)           # 4k - 1, 4k, 4k + 1 for k = 3 and 8
FEATURES = ("shared_prefix", "diff_at", "proper_prefix", "upper_case", "non_ascii", "spaces_in_literal", "embedded_dot", "duplicates",
            "crlf", "empty_lines", "no_final_newline", "lengths", "predicate_as_node", "two_classes", "type_triple", "ontology_subject",
            "object_ends_in_space")


def _term_of_length(n: int) -> str:
    if n == 1:
        return "x"
    return "<" + chr(ord("b") + LENGTHS.index(n)) * (n - 2) + ">"


def generate(seed: int = 0, triples: int = 2000, nodes: int = 300) -> bytes:
    """About ``triples`` triples over about ``nodes`` nodes, with every case of FEATURES; deterministic in its arguments."""
    rng = random.Random(seed)
    ids = [f"{PREFIX}id{i}instance>" for i in range(nodes)]
    preds = [f"{ONTO}pred{k}>" for k in range(7)]
    classes = [f"{ONTO}Class{k}>" for k in range(4)]
    special = []
    for n in LENGTHS:                                                   # terms of the listed lengths, as subject and as object
        special.append(f"{_term_of_length(n)} {preds[0]} {rng.choice(ids)} .")
        special.append(f"{rng.choice(ids)} {preds[1]} {_term_of_length(n)} .")
    for p in DIFF_AT:                                                   # pairs that first differ at byte p
        for last in "ak":
            special.append(f"<{'q' * (p - 1)}{last}tail> {preds[2]} {rng.choice(ids)} .")
    special += [
        f'{ids[0]} {preds[3]} "ab" .', f'{ids[1]} {preds[3]} "ab"@en .',              # a term that is a proper prefix of another
        f'{ids[2]} {preds[3]} "grüße ñandú 中文" .',       # lower-case non-ASCII UTF-8
        f'{ids[3]} {preds[3]} "one two  three" .',                                    # spaces in the object
        f'{ids[4]} {preds[3]} "the end . and more" .',                                # an embedded " ."
        f'{ids[5]} {preds[3]} "trailing"^^<http://www.w3.org/2001/XMLSchema#string>  .',      # object ends in a space
        f"{ids[6]} {preds[4]} {preds[5]} .", f"{preds[5]} {preds[4]} {ids[7]} .",     # a predicate that is a node too
        f"{ids[8]} {G.RDF_TYPE} {classes[0]} .", f"{ids[8]} {G.RDF_TYPE} {classes[1]} .",     # two classes on one node
        f"{ids[9]} <type> {classes[2]} .",                                            # a <type> triple: no edge, no label
        f"{G.ONTOLOGY_PREFIX}#Thing {G.RDF_TYPE} {ONTO}OnlyOnOntologySubjects> .",     # the class filter fires
        f"{ids[10].upper()} {preds[6].upper()} {ids[11]} .",                          # upper case folds onto existing terms
    ]
    lines = list(special)
    while len(lines) < triples - 40:
        s, o = rng.choice(ids), rng.choice(ids)
        if rng.random() < 0.1:
            s = s.replace("id", "ID")
        r = rng.random()
        if r < 0.08:
            lines.append(f"{s} {G.RDF_TYPE} {rng.choice(classes)} .")
        elif r < 0.18:
            lines.append(f'{s} {rng.choice(preds)} "literal {rng.randrange(25)} of many" .')
        else:
            lines.append(f"{s} {rng.choice(preds)} {o} .")
    lines += [rng.choice(lines) for _ in range(40)]                     # duplicate triples
    rng.shuffle(lines)
    out = []
    for i, line in enumerate(lines):
        out.append(line + ("\r\n" if i % 7 == 3 else "\n"))
        if i % 97 == 5:
            out.append("\n" if i % 2 else "\r\n")                        # empty lines
    return "".join(out).rstrip("\r\n").encode("utf-8")                  # no final newline


def simple(num_triples: int, distinct_subjects: bool = False, seed: int = 0) -> bytes:
    """``num_triples`` lines, each a message-passing triple, '\\n' after every one.  ``distinct_subjects``: every subject once,
    one predicate, one object (num_triples + 2 distinct terms); else a small random graph."""
    rng = random.Random(seed)
    if distinct_subjects:
        return "".join(f"<s{i}> <p> <o> .\n" for i in range(num_triples)).encode()
    n = max(2, num_triples // 6)
    return "".join(f"<n{rng.randrange(n)}> <p{rng.randrange(3)}> <n{rng.randrange(n)}> .\n" for _ in range(num_triples)).encode()


def lines_of(data: bytes):
    """the host loader's view of the bytes: a universal-newlines text read, then ``splitlines`` (graphs.parse_graph_nt)"""
    return data.decode("utf-8").replace("\r\n", "\n").splitlines()


def features(data: bytes) -> dict:
    """which of FEATURES the bytes hold (tests/test_ingest_reference.py asserts all of them for ``generate``)"""
    raw = data.decode("utf-8")
    triples = G.split_triples(lines_of(data))
    terms = {t for tr in triples for t in tr}
    nodes = {s for s, _, _ in triples} | {o for _, _, o in triples}
    preds = {p for _, p, _ in triples}
    types = G.nodes2type_mapping(triples, G.get_classes(triples))

    def first_difference(a, b):
        return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)

    tl = sorted(t.encode() for t in terms)
    diffs = {first_difference(a, b) for a, b in zip(tl, tl[1:])}
    raw_terms = {t for line in lines_of(data) if line[:-2] for t in line[:-2].split(" ", 2)}
    return {
        "shared_prefix": sum(t.startswith(PREFIX.lower()) for t in terms) > 100 and len(PREFIX) >= 48,
        "diff_at": set(DIFF_AT) <= diffs,
        "proper_prefix": '"ab"' in terms and '"ab"@en' in terms,
        "upper_case": any(t != t.lower() for t in raw_terms) and all(t.lower() in terms for t in raw_terms),
        "non_ascii": any(any(ord(ch) > 127 for ch in t) for t in terms),
        "spaces_in_literal": any(" " in o for _, _, o in triples),
        "embedded_dot": any(" ." in o for _, _, o in triples),
        "duplicates": len(set(triples)) < len(triples),
        "crlf": "\r\n" in raw,
        "empty_lines": "\n\n" in raw.replace("\r\n", "\n"),
        "no_final_newline": not raw.endswith("\n"),
        "lengths": {len(t.encode()) for t in nodes} >= set(LENGTHS),
        "predicate_as_node": bool((preds - set(G.TYPE_PREDICATES)) & nodes),
        "two_classes": any(len(v) >= 2 for v in types.values()),
        "type_triple": "<type>" in preds,
        "ontology_subject": any(p == G.RDF_TYPE and s.split("#")[0] == G.ONTOLOGY_PREFIX for s, p, _ in triples),
        "object_ends_in_space": any(o.endswith(" ") for _, _, o in triples),
    }


def expected(source) -> dict:
    """``source``: a path or the bytes.  edge_index / edge_type (int64 numpy), the sorted node, relation and class names, the
    labelled node ids in ascending order and their 0/1 rows (int64 [L, C])."""
    if not isinstance(source, (bytes, bytearray)):
        with open(source, "rb") as f:
            source = f.read()
    lines = lines_of(bytes(source))
    triples = G.split_triples(lines)
    g = G.Graph("expected")
    g.init_graph(lines)
    classes = G.get_classes(triples)
    types = G.nodes2type_mapping(triples, classes)
    enum = {c: i for i, c in enumerate(classes)}
    labelled = sorted(g.node_to_enum[s] for s, t in types.items() if t and s in g.node_to_enum)
    rows = np.zeros((len(labelled), len(classes)), dtype=np.int64)
    for j, node in enumerate(labelled):
        for c in types[g.nodes[node]]:
            rows[j, enum[c]] = 1
    return {"edge_index": g.training_data.edge_index.numpy(), "edge_type": g.training_data.edge_type.numpy(), "nodes": g.nodes,
            "relations": sorted(g.relations), "classes": classes, "labelled_idx": np.asarray(labelled, dtype=np.int64), "labels": rows}
