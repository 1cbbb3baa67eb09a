"""ovlgraph — MI355X-native drop-in for the overlap-scoring path of
roiteichman/Genome-Assembly-Using-Overlap-Graphs (aligners.py / overlapGraphs.py).

    from ovlgraph.overlapGraphs import construct_overlap_graph_nx_k
    from ovlgraph.aligners import overlap_alignment
    from ovlgraph.performanceMeasures import calculate_measures

Candidate pairs are enumerated on the host (Python), every pair is scored by
hand-written gfx950 HIP kernels behind the C ABI of include/ovl.h; the evaluation
stage aligns all contigs of an assembly to the genome in one batched launch.
"""
from ._lib import OvlError  # noqa: F401
from .engine import INDEL_DEFAULT, OverlapEngine, default_engine, encode_reads, score_reads  # noqa: F401

__all__ = ["OvlError", "OverlapEngine", "default_engine", "encode_reads", "score_reads", "INDEL_DEFAULT",
           "transitive_reduction", "assemble_contigs_string", "transitive_reduction2", "find_unitigs",
           "assemble_contigs", "pileup", "polish_contigs", "pileup_placed", "best_successor_layout", "layout_loop",
           "assemble_contigs_best_successor", "kmer_spectrum", "solid_threshold", "correct_reads",
           "reduced_string_graph", "assemble_contigs_direct"]


def __getattr__(name):
    # the string and unitig pipelines' entry points live in overlapGraphs, which imports networkx: loaded on first use, so
    # scoring-only processes (the sharded workers) do not pay for it
    if name in ("transitive_reduction", "assemble_contigs_string", "transitive_reduction2", "find_unitigs",
                "assemble_contigs"):
        from . import overlapGraphs
        return getattr(overlapGraphs, name)
    if name in ("pileup", "polish_contigs", "pileup_placed", "pileup_placed_loop"):
        from . import consensus
        return getattr(consensus, name)
    # the best-successor layout's entry points.  The function layout.layout is best_successor_layout here: the name
    # ovlgraph.layout is the submodule's, as the import system binds it, whatever was imported first
    if name in ("best_successor_layout", "layout_loop", "assemble_contigs_best_successor"):
        from .layout import assemble_contigs_best_successor, layout as best_successor_layout, layout_loop
        return {"best_successor_layout": best_successor_layout, "layout_loop": layout_loop,
                "assemble_contigs_best_successor": assemble_contigs_best_successor}[name]
    if name in ("reduced_string_graph", "assemble_contigs_direct"):
        from . import unitigs
        return getattr(unitigs, name)
    if name in ("kmer_spectrum", "solid_threshold", "correct_reads"):
        from . import correct
        return getattr(correct, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
