"""MI355X-native R-GCN layer (forward + backward) behind the reference's model/trainer API.

Importable name of the ``scaling-rgcn-training_amd`` package (a hyphen cannot be imported).
Sub-modules:

* ``plan``    -- graph plan (tile / chunk layout in HBM), pure tensor plumbing, runs anywhere
* ``_lib``    -- ctypes binding of ``librgcn_mi355x.so`` (the C ABI of include/rgcn_mi355x.h)
* ``conv``    -- ``RGCNConv``: PyG-2.3.1-compatible ``nn.Module`` whose forward/backward are the HIP kernels
* ``data``    -- ``Data`` attribute bag (stand-in for ``torch_geometric.data.Data``)
* ``layers``  -- ``Emb_Layers`` / ``Emb_ATT_Layers`` / ``Emb_MLP_Layers`` (reference model/layers.py API)
* ``trainer`` -- full-batch loop of reference model/modelTrainer.py (+ device-correct evaluation)
* ``graphs``  -- N-Triples ingest, dataset assembly, summary -> original embedding transfer (graphs/*.py, embeddingTricks.py)
* ``dist``    -- one-process-per-GPU edge partition + per-layer collective over RCCL
* ``summaries`` -- attribute-summary generation (murmur3 x64-128 of predicate sets; graphs/createAttributeSum.py), and on
  the GPU ``node_partition`` (k-bisimulation partition refinement) / ``quotient_graph`` over the layer's int64 COO
* ``sampling`` -- ``NeighborSampler``: fan-out neighbour sampling on the GPU into the layered bipartite ``Block`` lists that
  ``forward_blocks`` / ``Trainer.train_minibatch`` walk; ``block_index`` / ``BlockIndex``: the index ``RGCNConv.forward_block``
  runs a layer from, straight from a block, without graph plans
* ``sparse_optim`` -- ``RowAdam``: Adam on the embedding rows a mini-batch step gathered, nothing else of the table is touched
* ``linkpred`` -- link prediction: the ``DistMult`` decoder, ``corrupt`` negatives, filtered ``ranks`` / ``metrics``,
  ``FilterIndex``, ``with_inverse_edges``; ``Trainer.train_link_prediction`` is the loop around them
* ``transfer`` -- summaries -> original graph on tensors: ``summary_labels`` (the fractional labels of a partition's blocks),
  ``TransferredEmbedding`` and the ``stack`` / ``concat`` / ``sum_embeddings`` tricks ``Trainer.train_original`` takes
* ``tensor_data`` -- ``TensorDataset`` / ``TensorGraph``: the dataset ``Trainer`` reads, for a graph that has no node names
* ``ingest`` -- ``load_nt``: an N-Triples file -> COO tensors, labels and ``TermTable`` name tables on the GPU (``NTGraph``), with
  ``graphs.py``'s contract and no per-line Python

There is no CPU compute path: the layer raises if the HIP library or a GPU is missing.
"""
__version__ = "0.1.0"

from .plan import CHUNK, TilePlan, GraphPlans, build_plan, build_graph_plans, edge_weights  # noqa: F401


def __getattr__(name):
    # lazy: these need torch.nn / the HIP library, keep `import scaling_rgcn_training_amd` light
    if name in ("RGCNConv", "rgcn_conv_function", "target_block"):
        from . import conv
        return getattr(conv, name)
    if name == "Data":
        from .data import Data
        return Data
    if name in ("Emb_Layers", "Emb_ATT_Layers", "Emb_MLP_Layers"):
        from . import layers
        return getattr(layers, name)
    if name == "Trainer":
        from .trainer import Trainer
        return Trainer
    if name in ("create_sum_map", "hash128", "node_partition", "quotient_graph", "Partition"):
        from . import summaries
        return getattr(summaries, name)
    if name in ("NeighborSampler", "Block", "BlockIndex", "block_index"):
        from . import sampling
        return getattr(sampling, name)
    if name == "RowAdam":
        from .sparse_optim import RowAdam
        return RowAdam
    if name in ("DistMult", "corrupt", "with_inverse_edges", "FilterIndex", "ranks", "metrics"):
        from . import linkpred
        return getattr(linkpred, name)
    if name in ("TensorDataset", "TensorGraph"):
        from . import tensor_data
        return getattr(tensor_data, name)
    if name in ("load_nt", "NTGraph", "TermTable"):
        from . import ingest
        return getattr(ingest, name)
    if name in ("TransferredEmbedding", "summary_labels"):
        from . import transfer
        return getattr(transfer, name)
    raise AttributeError(name)
