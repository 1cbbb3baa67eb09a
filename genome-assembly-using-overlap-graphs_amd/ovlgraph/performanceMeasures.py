"""The reference pipeline's evaluation stage (performanceMeasures.py:6-73, 124-143, 190-252):
genome coverage, N50 and the two mismatch rates of an assembly, from the local alignment of every
contig to the genome.

``calculate_measures`` keeps the reference's signature, return value, keys, key order and Python value
types.  Its alignments -- the reference's per-contig loop over ``align_read_or_contig_to_reference`` --
come from one ``aligners.align_to_reference_batch`` call, which gives every contig a wavefront of one
GPU launch.  Plotting is not part of this project: ``plots`` may be any object with
``plot_genome_coverage`` and ``plot_genome_depth`` (the reference's ``plots`` module fits); it is called
with the reference's arguments under the reference's condition, and never when it is ``None``.
"""
from __future__ import annotations

import numpy as np

from .aligners import align_to_reference_batch


def calculate_genome_coverage_and_mismatch_rate(contigs_alignment_details, reference_genome, expected_coverage,
                                                experiment_name, num_iteration, path="plots", plots=None):
    """performanceMeasures.py:6-73: ``(coverage_rate, mismatch_rate_aligned_regions, mismatch_rate_full_genome)``.

    The reference's indexing is kept as it is: genome position ``start + i`` is marked as a mismatch from
    ``aligned_ref[i]`` and ``aligned_query[i]`` for ``i < end - start``, gap columns included.
    """
    genome_length = len(reference_genome)
    coverage = np.zeros(genome_length)
    mismatched = np.zeros(genome_length)
    for details in contigs_alignment_details.values():
        start, end = details["Start Position"], details["End Position"]
        if start == -1 or end == -1:
            continue
        aligned_ref, aligned_query = details["Alignment_reference"], details["Alignment_query"]
        coverage[start:end] += 1
        for i in range(end - start):
            if aligned_query[i] == "-" or aligned_query[i] != aligned_ref[i]:
                mismatched[start + i] += 1
    # performanceMeasures.py:53-58: later iterations with uniform coverage are not plotted
    if plots is not None and not (num_iteration != 1 and np.all(coverage == coverage[0])):
        plots.plot_genome_coverage(coverage, genome_length, experiment_name, num_iteration, path)
        plots.plot_genome_depth(coverage, expected_coverage, genome_length, experiment_name, num_iteration, path)
    covered = np.count_nonzero(coverage)
    uncovered = genome_length - covered
    bad = np.count_nonzero(mismatched)
    coverage_rate = covered / genome_length
    rate_aligned = bad / covered if covered > 0 else 0.0
    rate_genome = (bad + uncovered) / genome_length
    return coverage_rate, rate_aligned, rate_genome


def calculate_n50(contigs):
    """performanceMeasures.py:124-143: the length of the contig at which the running sum of the lengths, longest
    first, reaches half their total (0 for no contigs)."""
    lengths = sorted((len(c) for c in contigs), reverse=True)
    half = sum(lengths) / 2
    running = 0
    for length in lengths:
        running += length
        if running >= half:
            return length
    return 0


def calculate_measures(contigs, reads, num_reads, reads_length, error_prob, k, ref_genome, experiment_name,
                       num_iteration, path="plots", engine=None, plots=None):
    """performanceMeasures.py:190-252: ``(measures, contigs_alignment_details)``.

    The details dict is keyed by the contig string, so a repeated contig keeps its first position and its
    (identical) last details, as in the reference.
    """
    print(f"Calculating performance measures for {experiment_name} (Iteration {num_iteration})")
    expected_coverage = num_reads * reads_length / len(ref_genome)
    contigs = list(contigs)
    aligned = align_to_reference_batch(contigs, ref_genome, reads_length, engine=engine)
    contigs_alignment_details = {}
    for contig, (to_print, aligned_ref, aligned_query, score, start, end) in zip(contigs, aligned):
        contigs_alignment_details[contig] = {
            "Print": to_print,
            "Alignment_reference": aligned_ref,
            "Alignment_query": aligned_query,
            "Alignment Score": score,
            "Start Position": start,
            "End Position": end,
        }
    genome_coverage, rate_aligned, rate_genome = calculate_genome_coverage_and_mismatch_rate(
        contigs_alignment_details, ref_genome, expected_coverage, experiment_name, num_iteration, path, plots=plots)
    measures = {
        "Number of Contigs": len(contigs),
        "Genome Coverage": genome_coverage,
        "N50": calculate_n50(contigs),
        "Mismatch Rate Aligned Regions": rate_aligned,
        "Mismatch Rate Genome Level": rate_genome,
    }
    print(f"Performance measures for experiment_name={experiment_name} - N={num_reads}, l={reads_length}, "
          f"p={error_prob}, k={k}, num_iteration={num_iteration}:\n{measures}")
    return measures, contigs_alignment_details
