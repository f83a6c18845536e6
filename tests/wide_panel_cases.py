"""TEST INFRASTRUCTURE: the case table of the wide-panel tests -- graphs of a few sites under cohort-size haplotype panels, on
both sides of every word count at which a carrier-bitset kernel's loop changes shape.  tests/test_wide_panels_host.py checks
on the CPU that each case reaches the bitset routes and that the words past the switch decide expected counts;
tests/test_gpu_wide_panels.py runs the library on the same cases.  Both import CASES: one list of (H, seed, W, regions).

The switches, in bitset words (hw = ceil(H / 64)): 16 a trip of count_by_bitsets (graph_extract.hip), 64 a pass of the
lane-per-word kernels (count_by_bitsets_wave, hh_mask_hit, ha_entry_kernel) and the 4 096 haplotypes of a score / affinity
block, 80 a pass of graph_count_jobs_kernel, 128 the last register-resident row of pair_kernel."""
import functools

import numpy as np

from graph_table_checks import random_bitset_index

W = 16
LENGTH, N_SITES = 200, 14
SWITCHES = (16, 64, 80, 128)

# H: 1 024, 4 096, 5 120 fill their last word (no tail mask); 1 025, 4 097, 5 121 leave a later trip nothing but one masked
# word; 5 096 is the documented panel (80 words, 40 bits in the last); 8 193 is 129 words and three haplotype blocks.
# Regions: the whole chromosome, one or two short ones around site clusters, one clipped at an end of the chromosome.
CASES = [
    (1024, 1927, W, ((0, 200), (60, 100), (85, 125), (-8, 60))),
    (1025, 1927, W, ((0, 200), (60, 100), (85, 125), (-8, 60))),
    (4096, 5023, W, ((0, 200), (88, 140), (50, 80), (-8, 40))),
    (4097, 5023, W, ((0, 200), (88, 140), (50, 80), (-8, 40))),
    (5096, 6019, W, ((0, 200), (95, 140), (20, 60), (-8, 45))),
    (5120, 6040, W, ((0, 200), (28, 70), (85, 125), (-8, 30))),
    (5121, 6040, W, ((0, 200), (28, 70), (85, 125), (-8, 30))),
    (8193, 9125, W, ((0, 200), (45, 100), (60, 110), (-8, 40))),
]


class Args:
    """the members of the workflow object the graph tables read"""

    def __init__(self, threshold=0.2, no_reverse=False, recomb=False, qvalue_t=False, no_qvalue=True):
        self.threshold, self.noreverse, self.recomb = threshold, no_reverse, recomb
        self.noqvalue, self.qvalueT = no_qvalue, qvalue_t


def switch_words(H):
    """the largest switch below hw -- the words a kernel that never took its later trip would have read; a panel that sits on
    its first switch (1 024: 16 words) has none below: all but its last word"""
    hw = (H + 63) // 64
    below = [s for s in SWITCHES[:3] if s < hw]
    return max(below) if below else hw - 1


@functools.lru_cache(maxsize=None)
def graph(H, seed):
    return random_bitset_index(H, seed, length=LENGTH, n_sites=N_SITES)


def truncated(idx, n_hap):
    """the same graph over the first n_hap haplotypes (n_hap a multiple of 64)"""
    from grafimo_amd.extract_regions import GraphIndex
    assert n_hap % 64 == 0 and 0 < n_hap < idx.n_haplotypes
    return GraphIndex(idx.chrom, idx.ref, idx.pos, idx.n_alts, idx.alt_bases, np.ascontiguousarray(idx.alt_bits[:, :, :n_hap // 64]),
                      n_hap, del_len=idx.del_len, ins_len=idx.ins_len, ins_off=idx.ins_off, ins_bases=idx.ins_bases)


def motif(width=W, seed=0):
    from grafimo_amd import synth
    rec = synth.synthetic_motif(width, np.random.default_rng(4700 + 13 * width + seed), np.array([0.3, 0.2, 0.2, 0.3]))
    return synth.motif_object(rec, f"SYN{width}")


def groups(H):
    """thirds, an overlapping group, an empty one, all, and one group that lives entirely in the words past the switch"""
    third = H // 3
    past = 64 * switch_words(H)
    return {"first": list(range(third)), "second": list(range(third, 2 * third)), "third": list(range(2 * third, H)),
            "overlap": list(range(H // 4, H // 2 + 1)), "none": [], "all": list(range(H)), "past": list(range(past, H))}
