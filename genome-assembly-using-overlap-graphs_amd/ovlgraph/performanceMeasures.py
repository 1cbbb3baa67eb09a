"""The reference pipeline's evaluation stage (performanceMeasures.py:6-73, 124-143, 190-252):
genome coverage, N50 and the two mismatch rates of an assembly, from the local alignment of every
contig to the genome.

``calculate_measures`` keeps the reference's signature, return value, keys, key order and Python value
types.  Its alignments -- the reference's per-contig loop over ``align_read_or_contig_to_reference`` --
come from one ``aligners.align_to_reference_batch`` call, which gives every contig a wavefront of one
GPU launch.  Plotting is not part of this project: ``plots`` may be any object with
``plot_genome_coverage`` and ``plot_genome_depth`` (the reference's ``plots`` module fits); it is called
with the reference's arguments under the reference's condition, and never when it is ``None``.

``read_depth`` and ``plot_reconstructed_coverage`` are the step the reference left switched off (plots.py:97-168,
performanceMeasures.py:234-236): the read-depth coverage of the contigs, every read against every contig in one
``ovl_read_best`` call, with the same rule for drawing: ``plots.plot_contig_depth`` when ``plots`` is given.
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


# read_depth(device=None) takes the GPU from this many DP cells, counted as (sum of the read lengths) x (sum of the
# contig lengths).  From tools/read_depth_probe.py's sweep over the first r reads and c contigs of the PhiX workload
# (profiles/read_depth.json, host form on an EPYC 9575F): at 90,000 cells the host form took 0.44 ms against the
# device call's 1.13 ms; at 300,800 cells 1.44 ms against 1.14 ms, with the repetitions' ranges 0.008 and 0.013 ms
# wide; from there the device call won at every point (2.2 M cells: 9.5 ms against 1.2 ms; 132 M: 557 ms against
# 1.4 ms).  The device call costs about 1.1 ms whatever it holds, the host form fills 2.3 * 10^8 cells a second, so
# the crossover moves with the box's CPU.  The constant is the first point from which the device call won.
READ_DEPTH_DEVICE_MIN_CELLS = 300_800


class ReadDepth:
    """What ``read_depth`` returns: ``coverage`` (dict contig string -> float array, first-occurrence order,
    repeated contigs sharing one array), the int32 arrays ``best_score``, ``first_best``, ``n_best``, ``chosen``
    (-1 without contigs), ``start``, ``end`` over the reads, and ``ties(r)``: the contig positions that attain read
    r's best score, in order."""

    def __init__(self, coverage, best_score, first_best, n_best, chosen, start, end, tie_bits, n_contigs):
        self.coverage = coverage
        self.best_score = best_score
        self.first_best = first_best
        self.n_best = n_best
        self.chosen = chosen
        self.start = start
        self.end = end
        self._tie_bits = tie_bits
        self._n_contigs = n_contigs

    def ties(self, r):
        if self._n_contigs == 0:
            return np.zeros(0, dtype=np.int64)
        bits = np.unpackbits(self._tie_bits[r].astype("<u4").view(np.uint8), bitorder="little")
        return np.flatnonzero(bits[: self._n_contigs])


def read_depth(contigs, reads, read_length, match_score=10, mismatch=-1, indel=-1, engine=None, device=None,
               rng=None):
    """The read-depth coverage of plots.py:115-135 (``plot_reconstructed_coverage`` without its drawing): every
    read is aligned to every contig by ``align_read_or_contig_to_reference``, given to one of its best-scoring
    contigs -- ``rng.randint(0, n_ties)``, which consumes numpy's legacy stream exactly as the reference's
    ``np.random.choice(best_contigs)`` does; ``rng`` defaults to the ``np.random`` module -- and adds one to that
    contig's depth over the stretch ``[start:end)`` of its alignment to the *first* best contig (numpy slice
    semantics), as the reference does.  The reference's tuple indices are fixed to the six-tuple its aligner
    returns; its ``start != -1`` guard is not restated.

    The alignments and the selection run in native code: ``ovl_read_best`` on the GPU or ``ovl_read_best_host`` on
    one host thread.  ``device=None`` takes the host form when no GPU is visible or the pairs hold fewer than
    ``READ_DEPTH_DEVICE_MIN_CELLS`` cells; True / False force the choice."""
    from .engine import default_engine, read_best_host, use_device
    contigs, reads = list(contigs), list(reads)
    if use_device(device, lambda: sum(len(r) for r in reads) * sum(len(c) for c in contigs),
                  READ_DEPTH_DEVICE_MIN_CELLS, engine):
        res = (engine or default_engine()).read_best(reads, contigs, read_length, match_score, mismatch, indel)
    else:
        res = read_best_host(reads, contigs, read_length, match_score, mismatch, indel)
    rng = np.random if rng is None else rng
    coverage = {}
    for contig in contigs:
        if contig not in coverage:
            coverage[contig] = np.zeros(len(contig), dtype=float)
    R, C = len(reads), len(contigs)
    chosen = np.full(R, -1, dtype=np.int32)
    out = ReadDepth(coverage, res["best_score"], res["first_best"], res["n_best"], chosen, res["start"], res["end"],
                    res["tie_bits"], C)
    if C == 0:
        return out
    for r in range(R):
        ties = out.ties(r) if out.n_best[r] > 1 else (int(out.first_best[r]),)
        chosen[r] = ties[rng.randint(0, len(ties))]
        coverage[contigs[chosen[r]]][int(out.start[r]):int(out.end[r])] += 1
    return out


def plot_reconstructed_coverage(contigs, reads, num_reads, read_length, reference_genome, experiment_name,
                                num_iteration, path, engine=None, device=None, rng=None, plots=None):
    """plots.py:97-168 with the reference's signature: ``read_depth`` over the contigs and reads, then one
    ``plots.plot_contig_depth(contig_idx, coverage_array, expected_coverage, experiment_name, num_iteration,
    path)`` per contig position (0-based) when ``plots`` is not None.  Returns the ``read_depth`` object."""
    contigs = list(contigs)
    depth = read_depth(contigs, reads, read_length, engine=engine, device=device, rng=rng)
    if plots is not None:
        expected_coverage = num_reads * read_length / len(reference_genome)
        for contig_idx, contig in enumerate(contigs):
            plots.plot_contig_depth(contig_idx, depth.coverage[contig], expected_coverage, experiment_name,
                                    num_iteration, path)
    return depth
