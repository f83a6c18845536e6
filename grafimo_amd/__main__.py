"""``grafimo findmotif`` on the GPU.

The reference's ``findmotif`` runs ``get_motif_pwm`` -> ``scan_graph`` (external ``vg find``) ->
``compute_results`` -> ``write_results`` (grafimo.py:80-190).  Flags keep the names, defaults and meaning of the
reference CLI (__main__.py:119-415): -g/--genome-graph, -d/--genome-graph-dir, -b/--bedfile, --chroms-find,
--chroms-prefix-find, --chroms-namemap-find, -m/--motif, -k/--bgfile, -p/--pseudo, -t/--threshold, -q/--no-qvalue,
-r/--no-reverse, -f/--text-only, --recomb, --qvalueT, -j/--cores, -o/--out, --verbose, --debug.

With -g XG or -d DIR (+ -b BED) the run is the reference's: scan_graph over the chromosomes' graphs -- vg's own
chrN.xg + chrN.gbwt, read by grafimo_amd/vg_files.py, or the .gfmidx.npz saved beside them -- then compute_results per
motif.  The reference's tutorial runs as written (tutorials/findmotif_tutorial):

    python -m grafimo_amd -d data/mygenome/ -m data/example.meme -b data/regions.bed

``--sequences`` starts after ``scan_graph``: the directory it would have produced (``width_W/REGION.tsv``).

    python -m grafimo_amd -m MA0139.1.meme -s /tmp/grafimo_XXXX -t 1e-4 -o out_dir

Without vg, the k-mers can also come from the extraction kernel: give the inputs of ``grafimo buildvg``
(-l/--linear-genome FASTA, -v/--vcf phased VCF) and the -b/--bedfile of ``findmotif`` instead of -s;
substitutions, insertions and deletions of the VCF are part of that graph (grafimo_amd/extract_regions.py).

    python -m grafimo_amd -m MA0139.1.meme -l chr22.fa -v chr22.vcf.gz -b peaks.bed -o out_dir
"""
import argparse
import importlib
import sys
import time

from .motif_ops import get_motif_pwm
from .res_writer import DEFAULT_OUTDIR, print_results, write_results
from .score_sequences import compute_results, compute_results_many
from .utils import UNIF
from .workflow import Findmotif


class _Workflow(Findmotif):
    def __init__(self, a):
        super().__init__(cores=a.cores, threshold=a.threshold, no_qvalue=a.no_qvalue, qval_t=a.qval_t,
                         no_reverse=a.no_reverse, recomb=a.recomb, verbose=a.verbose, bgfile=a.bgfile,
                         pseudo=a.pseudo, graph_genome=a.genome_graph or "", graph_genome_dir=a.genome_graph_dir or "",
                         bedfile=a.bedfile or "", chroms=a.chroms_find, chroms_prefix=a.chroms_prefix or "",
                         namemap=_parse_namemap(a.chroms_namemap_find))
        self.outdir = a.out
        self.top_graphs = 0
        self.text_only = a.text_only


NOMAP = "NOMAP"


def _parse_namemap(fn):
    """utils.parse_namemap (utils.py:83-120): original chromosome name, the name its graph is stored under"""
    if not fn or fn == NOMAP:
        return {}
    import os
    if not os.path.isfile(fn):
        sys.exit(f"ERROR: Unable to find {fn}.")
    out = {}
    with open(fn) as fh:
        for line in fh:
            f = line.split()
            if len(f) >= 2:
                out[f[0]] = f[1]
    return out


def get_parser():
    p = argparse.ArgumentParser(prog="python -m grafimo_amd", description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("-m", "--motif", nargs="+", required=True, metavar="MOTIF-FILE")
    p.add_argument("-g", "--genome-graph", dest="genome_graph", metavar="XG",
                   help="whole-genome graph: vg's XG (the GBWT beside it), or the .gfmidx.npz saved under its name")
    p.add_argument("-d", "--genome-graph-dir", dest="genome_graph_dir", metavar="DIR",
                   help="directory of per-chromosome graphs (chrN.xg + chrN.gbwt, or chrN.gfmidx.npz)")
    p.add_argument("--chroms-find", dest="chroms_find", nargs="*", default=[], metavar="CHR",
                   help="scan only these chromosomes (default: every chromosome of the BED file)")
    p.add_argument("--chroms-namemap-find", dest="chroms_namemap_find", nargs="?", default=NOMAP, metavar="NAME-MAP-FILE",
                   help="two columns: chromosome name, name its graph is stored under")
    p.add_argument("-s", "--sequences", metavar="DIR",
                   help="directory holding width_W/*.tsv as written by vg find -K W -E")
    p.add_argument("-l", "--linear-genome", dest="linear_genome", metavar="FASTA",
                   help="reference FASTA (with -v and -b: extract the k-mers on the GPU instead of -s)")
    p.add_argument("-v", "--vcf", metavar="VCF", help="phased VCF (.vcf or .vcf.gz): substitutions, insertions, deletions")
    p.add_argument("-b", "--bedfile", metavar="BED", help="regions to scan (UCSC BED: lines starting with chr)")
    p.add_argument("--chroms-prefix-find", dest="chroms_prefix", nargs="?", default="", metavar="PREFIX",
                   help="graph files / chromosome names in the FASTA and VCF = PREFIX + the BED name without its leading chr")
    p.add_argument("--strict-variants", action="store_true", dest="strict_variants",
                   help="fail on VCF records with a symbolic ALT (<DEL>, <CN0>, breakends, '*') instead of leaving them "
                        "out with a warning, which is what vg construct does without --handle-sv")
    p.add_argument("--skip-unmodelled-variants", action="store_true", dest="skip_unmodelled",
                   help="accepted for compatibility (it is the default now: complex alleles are modelled, records with "
                        "symbolic ALTs are left out with a warning)")
    p.add_argument("-k", "--bgfile", default=UNIF)
    p.add_argument("-p", "--pseudo", type=float, default=0.1)
    p.add_argument("-t", "--threshold", type=float, default=1e-4)
    p.add_argument("-q", "--no-qvalue", action="store_true", dest="no_qvalue")
    p.add_argument("-r", "--no-reverse", action="store_true", dest="no_reverse")
    p.add_argument("-f", "--text-only", action="store_true", dest="text_only")
    p.add_argument("--recomb", action="store_true")
    p.add_argument("--qvalueT", action="store_true", dest="qval_t")
    p.add_argument("--variant-effects", action="store_true", dest="variant_effects",
                   help="also write grafimo_variant_effects[_MOTIF].tsv (printed with -f): the best REF and ALT hit of every "
                        "variant site, rows kept on p < -t (graph routes only; no q-values, so not with --qvalueT)")
    p.add_argument("--haplotype-hits", action="store_true", dest="haplotype_hits",
                   help="also write grafimo_haplotype_hits[_MOTIF].tsv (printed with -f): per region, how many of the report's "
                        "rows each haplotype carries, one column per haplotype (graph routes only)")
    p.add_argument("--haplotype-scores", action="store_true", dest="haplotype_scores",
                   help="also write grafimo_haplotype_scores[_MOTIF].tsv (printed with -f): per region, each haplotype's best "
                        "motif score whatever the threshold, beside the reference's (graph routes only)")
    p.add_argument("--haplotype-affinity", action="store_true", dest="haplotype_affinity",
                   help="also write grafimo_haplotype_affinity[_MOTIF].tsv (printed with -f): per region, the log2 of each "
                        "haplotype's total binding affinity -- the sum of 2^(log-odds / T) over every k-mer of its own "
                        "sequence --, beside the reference's (graph routes only)")
    p.add_argument("--affinity-temperature", dest="affinity_temperature", type=float, default=None, metavar="T",
                   help="with --haplotype-affinity, --variant-affinity, --haplotype-classes, --query-variants, --mutation-scan, --indel-scan, --deletion-scan, --substitution-scan, --insertion-scan or --shuffle-null: the temperature T > 0 the log-odds scores are "
                        "divided by; default 1")
    p.add_argument("--variant-affinity", action="store_true", dest="variant_affinity",
                   help="also write grafimo_variant_affinity[_MOTIF].tsv (printed with -f): per variant, the log2 of the mean "
                        "total binding affinity of the REF carriers over the allele's footprint beside the ALT carriers', "
                        "and their difference -- every k-mer counts, whatever the threshold (graph routes only)")
    p.add_argument("--variant-affinity-delta", dest="variant_affinity_delta", type=float, default=None, metavar="X",
                   help="with --variant-affinity: keep only the rows with |delta_log2_affinity| >= X; default: every row")
    p.add_argument("--hit-alleles", action="store_true", dest="hit_alleles",
                   help="also write grafimo_hit_alleles[_MOTIF].tsv (printed with -f): the report's rows, each with the variant "
                        "alleles that make its k-mer and, with --haplotype-groups, its carriers per group (graph routes only)")
    p.add_argument("--haplotype-groups", dest="haplotype_groups", metavar="FILE",
                   help="with --hit-alleles, --hit-pairs, --haplotype-classes, --haplotype-sequences, --query-variants, --mutation-scan, --indel-scan, --deletion-scan, --substitution-scan, --insertion-scan, --site-distance or --shuffle-null: SAMPLE GROUP lines (the 1000 Genomes panel file reads as is), one "
                        "haplotypes_GROUP column per group")
    p.add_argument("--haplotype-classes", action="store_true", dest="haplotype_classes",
                   help="also write grafimo_haplotype_classes[_MOTIF].tsv (printed with -f) and "
                        "grafimo_haplotype_class_members.tsv: per region the distinct allele combinations the haplotypes hold, "
                        "each with its count, its counts per --haplotype-groups group, its alleles and its representative's "
                        "best score and total affinity (--affinity-temperature) (graph routes only)")
    p.add_argument("--class-min-haplotypes", dest="class_min_haplotypes", type=int, default=None, metavar="N",
                   help="with --haplotype-classes: keep only the classes of at least N haplotypes; default 1")
    p.add_argument("--haplotype-sequences", action="store_true", dest="haplotype_sequences",
                   help="also write grafimo_haplotype_sequences.fa and grafimo_haplotype_sequence_versions.tsv (the table is "
                        "printed with -f): per region the distinct sequences the haplotypes spell in it, each with its count, "
                        "its counts per --haplotype-groups group, the haplotype classes that spell it and its bases "
                        "(graph routes only)")
    p.add_argument("--query-variants", dest="query_variants", metavar="FILE",
                   help="also write grafimo_query_variants[_MOTIF].tsv and grafimo_query_variant_contexts[_MOTIF].tsv (printed "
                        "with -f): the variants of the VCF FILE, which need not be in the panel, applied to every sequence "
                        "background the haplotypes spell around them -- per background the best hit and the total affinity "
                        "(--affinity-temperature) before and after, gain / loss on p < -t, and its haplotypes, also per "
                        "--haplotype-groups group (graph routes only)")
    p.add_argument("--query-all", action="store_true", dest="query_all",
                   help="with --query-variants: keep every variant, not only those that create or destroy a hit on some "
                        "background")
    p.add_argument("--mutation-scan", action="store_true", dest="mutation_scan",
                   help="also write grafimo_mutation_scan[_MOTIF].tsv and grafimo_mutation_scan_summary[_MOTIF].tsv (printed "
                        "with -f): in-silico saturation mutagenesis -- every single-base change at every base of every "
                        "sequence the haplotypes spell in a region (inserted bases too) and of the reference sequence, with "
                        "the best hit and the total affinity (--affinity-temperature) before and after, gain / loss on "
                        "p < -t and its haplotypes, also per --haplotype-groups group; rows are kept on gain or loss "
                        "(graph routes only)")
    p.add_argument("--mutation-delta", dest="mutation_delta", type=float, default=None, metavar="X",
                   help="with --mutation-scan: also keep the rows with |delta_log2_affinity| >= X")
    p.add_argument("--mutation-all", action="store_true", dest="mutation_all",
                   help="with --mutation-scan: keep every row, three per base")
    p.add_argument("--mutation-profile", action="store_true", dest="mutation_profile",
                   help="also write grafimo_mutation_profile.tsv and grafimo_mutation_profile_summary.tsv (printed with -f): the "
                        "mutation scan folded over the whole motif set on the GPU -- per single-base change how many motifs "
                        "gain and lose a site (p < -t), the most significant gain and loss, and the motifs whose total "
                        "affinity (--affinity-temperature) moves most, up and down; a row carries its sequence's "
                        "haplotypes, also per --haplotype-groups group; one table per call; rows are kept when some motif gains or loses "
                        "(graph routes only)")
    p.add_argument("--mutation-profile-delta", dest="mutation_profile_delta", type=float, default=None, metavar="X",
                   help="with --mutation-profile: also keep the rows whose up or down champion has |delta_log2_affinity| >= X")
    p.add_argument("--mutation-profile-all", action="store_true", dest="mutation_profile_all",
                   help="with --mutation-profile: keep every row, three per base")
    p.add_argument("--indel-scan", action="store_true", dest="indel_scan",
                   help="also write grafimo_indel_scan[_MOTIF].tsv and grafimo_indel_scan_summary[_MOTIF].tsv (printed with "
                        "-f): the mutation scan's companion for one-base indels -- the deletion of every base and the insertion "
                        "of A, C, G and T behind every base of every sequence the haplotypes spell in a region (inserted "
                        "bases too) and of the reference sequence, with the best hit and the total affinity "
                        "(--affinity-temperature) before and after, gain / loss on p < -t and its haplotypes, also per "
                        "--haplotype-groups group; rows are kept on gain or loss; in a homopolymer a change is reported "
                        "once, at its leftmost offset (graph routes only)")
    p.add_argument("--indel-delta", dest="indel_delta", type=float, default=None, metavar="X",
                   help="with --indel-scan: also keep the rows with |delta_log2_affinity| >= X")
    p.add_argument("--indel-all", action="store_true", dest="indel_all",
                   help="with --indel-scan: keep every row, up to five per base")
    p.add_argument("--deletion-scan", dest="deletion_scan", nargs="+", type=int, default=None, metavar="L",
                   help="also write grafimo_deletion_scan[_MOTIF].tsv and grafimo_deletion_scan_summary[_MOTIF].tsv (printed "
                        "with -f): the indel scan's companion for block deletions -- the deletion of every block of L bases, "
                        "for each given L in 1 .. 64 (duplicates are merged, the list is sorted), at every offset of every "
                        "sequence the haplotypes spell in a region (inserted bases too) and of the reference sequence, with "
                        "the best hit and the total affinity before and after, the effect, and the haplotypes that spell the "
                        "sequence, in all and per --haplotype-groups group; rows are kept on gain or loss; in a repeat a "
                        "deletion is reported once, at its leftmost offset (graph routes only)")
    p.add_argument("--deletion-delta", dest="deletion_delta", type=float, default=None, metavar="X",
                   help="with --deletion-scan: also keep the rows with |delta_log2_affinity| >= X")
    p.add_argument("--deletion-all", action="store_true", dest="deletion_all",
                   help="with --deletion-scan: keep every row, up to one per base and length")
    p.add_argument("--substitution-scan", dest="substitution_scan", nargs="+", type=int, default=None, metavar="L",
                   help="also write grafimo_substitution_scan[_MOTIF].tsv and grafimo_substitution_scan_summary[_MOTIF].tsv "
                        "(printed with -f): the deletion scan's companion for blocks replaced in place -- every block of L "
                        "bases, for each given L in 1 .. 64 (duplicates are merged, the list is sorted), replaced by its image "
                        "under --substitution-map at every offset of every sequence the haplotypes spell in a region (inserted "
                        "bases too) and of the reference sequence, with the best hit and the total affinity before and after, "
                        "the effect, and the haplotypes that spell the sequence, in all and per --haplotype-groups group; rows "
                        "are kept on gain or loss; a block the map does not change is no row (graph routes only)")
    p.add_argument("--substitution-map", dest="substitution_map", default=None, metavar="MAP",
                   help="with --substitution-scan: transversion (A>C C>A G>T T>G), complement, transition, or the images of "
                        "A, C, G, T as four letters over ACGT, such as AAAA for a poly-A linker; default transversion")
    p.add_argument("--substitution-delta", dest="substitution_delta", type=float, default=None, metavar="X",
                   help="with --substitution-scan: also keep the rows with |delta_log2_affinity| >= X")
    p.add_argument("--substitution-all", action="store_true", dest="substitution_all",
                   help="with --substitution-scan: keep every row, up to one per base and length")
    p.add_argument("--insertion-scan", dest="insertion_scan", nargs="+", default=None, metavar="SEQ",
                   help="also write grafimo_insertion_scan[_MOTIF].tsv and grafimo_insertion_scan_summary[_MOTIF].tsv (printed "
                        "with -f): the deletion scan's companion for block insertions -- each given SEQ, 1 .. 16 inserts of "
                        "1 .. 64 letters of ACGT (case is folded, a repeated SEQ is dropped), inserted behind every base of "
                        "every sequence the haplotypes spell in a region (inserted bases too) and of the reference sequence, "
                        "with the best hit and the total affinity before and after, the effect, and the haplotypes that spell "
                        "the sequence, in all and per --haplotype-groups group; rows are kept on gain or loss; in a repeat an "
                        "insertion is reported once, at its leftmost offset (graph routes only)")
    p.add_argument("--insertion-delta", dest="insertion_delta", type=float, default=None, metavar="X",
                   help="with --insertion-scan: also keep the rows with |delta_log2_affinity| >= X")
    p.add_argument("--insertion-all", action="store_true", dest="insertion_all",
                   help="with --insertion-scan: keep every row, up to one per base and insert")
    p.add_argument("--site-distance", dest="site_distance", nargs="?", type=int, const=3, default=None, metavar="E",
                   help="also write grafimo_site_distance[_MOTIF].tsv and grafimo_site_distance_summary[_MOTIF].tsv (printed "
                        "with -f): for every window of every sequence the haplotypes spell in a region (inserted bases too) and "
                        "of the reference sequence, on both strands, the least number of substitutions, up to E in 1 .. 8 "
                        "(default 3), that lifts it to a hit at p < -t, or that drops a hit under it, with the changes and the "
                        "edited k-mer, and per coordinate the haplotypes with a site, with a near-site at each distance, in "
                        "all and per --haplotype-groups group; rows are kept for sites and near-sites (graph routes only)")
    p.add_argument("--site-distance-all", action="store_true", dest="site_distance_all",
                   help="with --site-distance: keep every window and strand, also those more than E substitutions from a site")
    p.add_argument("--shuffle-null", dest="shuffle_null", nargs="?", type=int, const=1000, default=None, metavar="K",
                   help="also write grafimo_shuffle_null[_MOTIF].tsv and grafimo_motif_enrichment.tsv (printed with -f): every "
                        "sequence the haplotypes spell in a region, and the reference sequence, against K (default 1000) "
                        "composition-preserving shuffles of itself -- the empirical p-values (1 + ge) / (K + 1) of its best "
                        "score and of its total affinity (--affinity-temperature), with its haplotypes, also per "
                        "--haplotype-groups group --, and per motif how many regions hold a hit at p < -t against the same "
                        "count over the shuffles (graph routes only)")
    p.add_argument("--null-seed", dest="null_seed", type=int, default=None, metavar="N",
                   help="with --shuffle-null: the seed of the shuffles, 0 .. 2^64 - 1; default 0")
    p.add_argument("--null-order", dest="null_order", type=int, choices=(1, 2), default=None, metavar="{1,2}",
                   help="with --shuffle-null: 1, mononucleotide shuffles (the default), or 2, shuffles that keep every "
                        "sequence's doublet counts, first and last base -- the null for genomic peaks, whose CpG depletion "
                        "and poly-A/T runs a mononucleotide shuffle destroys; both files then end in a null_order column")
    p.add_argument("--hit-pairs", action="store_true", dest="hit_pairs",
                   help="also write grafimo_hit_pairs.tsv (printed with -f): the pairs of report rows -- of one motif or of "
                        "two -- of a region that lie within --pair-gap of each other and share carrier haplotypes, with how "
                        "many haplotypes carry both (graph routes only)")
    p.add_argument("--pair-gap", dest="pair_gap", nargs=2, type=int, default=None, metavar=("MIN", "MAX"),
                   help="with --hit-pairs: the reference bases between the two rows of a pair, MIN <= gap <= MAX (negative: "
                        "overlapping by that many); default 0 50")
    p.add_argument("--hit-linkage", action="store_true", dest="hit_linkage",
                   help="also write grafimo_hit_linkage[_MOTIF].tsv (printed with -f): per report row the variant alleles "
                        "within --linkage-flank of it whose carriers are in linkage disequilibrium with the row's, "
                        "r2 >= --linkage-r2, with r2, r and D' (graph routes only)")
    p.add_argument("--linkage-flank", dest="linkage_flank", type=int, default=None, metavar="N",
                   help="with --hit-linkage: the reference bases around a row in which variants are tested; default 10000")
    p.add_argument("--linkage-r2", dest="linkage_r2", type=float, default=None, metavar="X",
                   help="with --hit-linkage: the smallest r2 listed, 0 .. 1; default 0.8")
    p.add_argument("-j", "--cores", type=int, default=0, help="host threads for TSV ingest (0 = all)")
    p.add_argument("-o", "--out", default=DEFAULT_OUTDIR)
    p.add_argument("--verbose", action="store_true")
    p.add_argument("--debug", action="store_true")
    return p


def buildvg(argv):
    """`grafimo buildvg -l FASTA -v VCF [--chroms-build 1 X] [--chroms-prefix-build P | --chroms-namemap-build FILE] [-o DIR]`
    (__main__.py:200-260, constructVG.py:137-300): one graph per chromosome, named as the reference names its chrN.xg --
    here the .gfmidx.npz scan_graph takes in the XG's place (GraphIndex.from_fasta_vcf: the library's VCF reader, host only)."""
    import os
    from .extract_regions import GraphIndex, INDEX_SUFFIX
    p = argparse.ArgumentParser(prog="python -m grafimo_amd buildvg", description=buildvg.__doc__)
    p.add_argument("-l", "--linear-genome", dest="linear_genome", required=True, metavar="FASTA")
    p.add_argument("-v", "--vcf", required=True, metavar="VCF")
    p.add_argument("--chroms-build", dest="chroms_build", nargs="*", default=[], metavar="CHR")
    p.add_argument("--chroms-prefix-build", dest="chroms_prefix_build", nargs="?", default="", metavar="PREFIX")
    p.add_argument("--chroms-namemap-build", dest="chroms_namemap_build", nargs="?", default=NOMAP, metavar="NAME-MAP-FILE")
    p.add_argument("--strict-variants", action="store_true", dest="strict_variants")
    p.add_argument("-j", "--cores", type=int, default=0)
    p.add_argument("-o", "--out", default="")
    p.add_argument("--verbose", action="store_true")
    p.add_argument("--debug", action="store_true")
    a = p.parse_args(argv)
    for f in (a.linear_genome, a.vcf):
        if not os.path.isfile(f):
            sys.exit(f"ERROR: Unable to locate {f}")
    if a.chroms_prefix_build and a.chroms_namemap_build != NOMAP:
        sys.exit('ERROR: "--chroms-prefix-build" and "chroms-namemap-build" cannot be used together')
    namemap = _parse_namemap(a.chroms_namemap_build)
    available = []
    with open(a.linear_genome) as fh:                 # get_chromlist (constructVG.py:407-470): the FASTA's sequence names
        for line in fh:
            if line.startswith(">"):
                available.append(line.rstrip().split()[0][1:])
    chroms = a.chroms_build or available
    for c in chroms:
        if c not in available:
            sys.exit(f'ERROR: Chromosome "{c}" not found among names in {a.linear_genome}.')
    out = a.out or os.getcwd()
    os.makedirs(out, exist_ok=True)
    start = time.time()
    for c in chroms:
        if namemap and c not in namemap:
            sys.exit(f'ERROR: Missing out name map for chromosome "{c}".')
        name = namemap[c] if namemap else a.chroms_prefix_build + c
        t0 = time.time()
        index = GraphIndex.from_fasta_vcf(a.linear_genome, a.vcf, c, threads=a.cores, allow_skipped=not a.strict_variants)
        path = index.save(os.path.join(out, name))
        if a.verbose:
            print(f"{c}: {len(index.ref)} bases, {len(index.pos)} variant sites, {index.n_haplotypes} haplotypes -> {path} "
                  "in %.2fs" % (time.time() - t0))
    print("Elapsed time %.2fs" % (time.time() - start))


# the per-graph result tables: option -> (its flag, what the rows of -s / of scan_graph's TSV files lack for it)
_GRAPH_TABLES = {"variant_effects": ("--variant-effects", "alleles"), "haplotype_hits": ("--haplotype-hits", "walks"),
                 "haplotype_scores": ("--haplotype-scores", "walks"), "haplotype_affinity": ("--haplotype-affinity", "walks"),
                 "variant_affinity": ("--variant-affinity", "walks"), "hit_alleles": ("--hit-alleles", "walks"),
                 "hit_pairs": ("--hit-pairs", "walks"), "hit_linkage": ("--hit-linkage", "walks"),
                 "haplotype_classes": ("--haplotype-classes", "haplotypes"),
                 "haplotype_sequences": ("--haplotype-sequences", "haplotypes"),
                 "query_variants": ("--query-variants", "haplotypes"), "mutation_scan": ("--mutation-scan", "haplotypes"),
                 "mutation_profile": ("--mutation-profile", "haplotypes"),
                 "indel_scan": ("--indel-scan", "haplotypes"), "deletion_scan": ("--deletion-scan", "haplotypes"),
                 "substitution_scan": ("--substitution-scan", "haplotypes"), "insertion_scan": ("--insertion-scan", "haplotypes"),
                 "site_distance": ("--site-distance", "haplotypes"),
                 "shuffle_null": ("--shuffle-null", "haplotypes")}


def _graph_only(a, table):
    """refuse a graph table asked for over the rows of -s"""
    if getattr(a, table) and a.sequences:
        flag, lacks = _GRAPH_TABLES[table]
        sys.exit(f"ERROR: {flag} needs the graph (-g / -d with -b, or -l -v -b): the rows of -s carry no {lacks}")


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if argv and argv[0] == "buildvg":                  # the reference's two workflows (__main__.py:119-415); findmotif is the default
        return buildvg(argv[1:])
    if argv and argv[0] == "findmotif":
        argv = argv[1:]
    a = get_parser().parse_args(argv)
    if a.threshold <= 0 or a.threshold > 1:
        sys.exit("ERROR: the threshold must be in (0, 1]")
    if a.qval_t and a.no_qvalue:
        sys.exit("ERROR: --qvalueT needs q-values (drop -q)")
    from_vg = bool(a.genome_graph or a.genome_graph_dir)
    if from_vg:
        if a.genome_graph and a.genome_graph_dir:
            sys.exit("ERROR: give -g XG or -d DIR, not both")
        if not a.bedfile or a.sequences or a.linear_genome or a.vcf:
            sys.exit("ERROR: -g / -d go with -b BED (and without -s, -l, -v)")
        if a.chroms_prefix and a.chroms_namemap_find != NOMAP:
            sys.exit('ERROR: "--chroms-prefix-find" and "chroms-namemap-find" cannot be used together')
        if len(set(a.chroms_find)) != len(a.chroms_find):
            sys.exit('ERROR: Duplicated chromosome names given to "--chroms-find"')
    from_graph = not from_vg and bool(a.linear_genome or a.vcf or a.bedfile)
    _graph_only(a, "variant_effects")
    if a.variant_effects and a.qval_t:
        sys.exit("ERROR: --variant-effects has no q-values: its rows are kept on p < -t, which --qvalueT makes a q-value "
                 "threshold (drop --qvalueT)")
    _graph_only(a, "haplotype_hits")
    _graph_only(a, "haplotype_scores")
    if a.affinity_temperature is not None and not (a.haplotype_affinity or a.variant_affinity or a.haplotype_classes
                                                    or a.query_variants or a.mutation_scan or a.mutation_profile or a.indel_scan
                                                    or a.deletion_scan or a.substitution_scan or a.insertion_scan or a.shuffle_null):
        sys.exit("ERROR: --affinity-temperature goes with --haplotype-affinity or --variant-affinity or --haplotype-classes")
    if a.affinity_temperature is not None and not a.affinity_temperature > 0:
        sys.exit(f"ERROR: --affinity-temperature {a.affinity_temperature} is not > 0")
    _graph_only(a, "haplotype_affinity")
    if a.variant_affinity_delta is not None and not a.variant_affinity:
        sys.exit("ERROR: --variant-affinity-delta goes with --variant-affinity")
    if a.variant_affinity_delta is not None and not a.variant_affinity_delta >= 0:
        sys.exit(f"ERROR: --variant-affinity-delta {a.variant_affinity_delta} is not >= 0")
    _graph_only(a, "variant_affinity")
    if a.haplotype_groups and not (a.hit_alleles or a.hit_pairs or a.haplotype_classes or a.haplotype_sequences
                                   or a.query_variants or a.mutation_scan or a.mutation_profile or a.indel_scan
                                   or a.deletion_scan or a.substitution_scan or a.insertion_scan or a.site_distance or a.shuffle_null):
        sys.exit("ERROR: --haplotype-groups goes with --hit-alleles or --hit-pairs or --haplotype-classes or "
                 "--haplotype-sequences or --site-distance")
    if a.class_min_haplotypes is not None and not a.haplotype_classes:
        sys.exit("ERROR: --class-min-haplotypes goes with --haplotype-classes")
    if a.class_min_haplotypes is not None and a.class_min_haplotypes < 1:
        sys.exit(f"ERROR: --class-min-haplotypes {a.class_min_haplotypes} < 1")
    _graph_only(a, "haplotype_classes")
    _graph_only(a, "haplotype_sequences")
    if a.query_all and not a.query_variants:
        sys.exit("ERROR: --query-all goes with --query-variants")
    if a.query_variants:
        import os
        if not os.path.isfile(a.query_variants):
            sys.exit(f"ERROR: Unable to locate {a.query_variants}")
    _graph_only(a, "query_variants")
    if a.mutation_all and not a.mutation_scan:
        sys.exit("ERROR: --mutation-all goes with --mutation-scan")
    if a.mutation_delta is not None and not a.mutation_scan:
        sys.exit("ERROR: --mutation-delta goes with --mutation-scan")
    if a.mutation_delta is not None and not a.mutation_delta >= 0:
        sys.exit(f"ERROR: --mutation-delta {a.mutation_delta} is not >= 0")
    _graph_only(a, "mutation_scan")
    if a.mutation_profile_all and not a.mutation_profile:
        sys.exit("ERROR: --mutation-profile-all goes with --mutation-profile")
    if a.mutation_profile_delta is not None and not a.mutation_profile:
        sys.exit("ERROR: --mutation-profile-delta goes with --mutation-profile")
    if a.mutation_profile_delta is not None and not a.mutation_profile_delta >= 0:
        sys.exit(f"ERROR: --mutation-profile-delta {a.mutation_profile_delta} is not >= 0")
    _graph_only(a, "mutation_profile")
    if a.indel_all and not a.indel_scan:
        sys.exit("ERROR: --indel-all goes with --indel-scan")
    if a.indel_delta is not None and not a.indel_scan:
        sys.exit("ERROR: --indel-delta goes with --indel-scan")
    if a.indel_delta is not None and not a.indel_delta >= 0:
        sys.exit(f"ERROR: --indel-delta {a.indel_delta} is not >= 0")
    _graph_only(a, "indel_scan")
    if a.deletion_all and not a.deletion_scan:
        sys.exit("ERROR: --deletion-all goes with --deletion-scan")
    if a.deletion_delta is not None and not a.deletion_scan:
        sys.exit("ERROR: --deletion-delta goes with --deletion-scan")
    if a.deletion_delta is not None and not a.deletion_delta >= 0:
        sys.exit(f"ERROR: --deletion-delta {a.deletion_delta} is not >= 0")
    if a.deletion_scan:
        bad = [L for L in a.deletion_scan if not 1 <= L <= 64]
        if bad:
            sys.exit(f"ERROR: --deletion-scan {bad[0]}: a length lies in 1 .. 64")
        a.deletion_scan = sorted(set(a.deletion_scan))
    _graph_only(a, "deletion_scan")
    if a.substitution_all and not a.substitution_scan:
        sys.exit("ERROR: --substitution-all goes with --substitution-scan")
    if a.substitution_delta is not None and not a.substitution_scan:
        sys.exit("ERROR: --substitution-delta goes with --substitution-scan")
    if a.substitution_map is not None and not a.substitution_scan:
        sys.exit("ERROR: --substitution-map goes with --substitution-scan")
    if a.substitution_delta is not None and not a.substitution_delta >= 0:
        sys.exit(f"ERROR: --substitution-delta {a.substitution_delta} is not >= 0")
    if a.substitution_scan:
        bad = [L for L in a.substitution_scan if not 1 <= L <= 64]
        if bad:
            sys.exit(f"ERROR: --substitution-scan {bad[0]}: a length lies in 1 .. 64")
        a.substitution_scan = sorted(set(a.substitution_scan))
        from .substitution_scan import checked_map
        try:
            checked_map(a.substitution_map or "transversion")
        except ValueError as e:
            sys.exit(f"ERROR: --substitution-map: {e}")
    _graph_only(a, "substitution_scan")
    if a.insertion_all and not a.insertion_scan:
        sys.exit("ERROR: --insertion-all goes with --insertion-scan")
    if a.insertion_delta is not None and not a.insertion_scan:
        sys.exit("ERROR: --insertion-delta goes with --insertion-scan")
    if a.insertion_delta is not None and not a.insertion_delta >= 0:
        sys.exit(f"ERROR: --insertion-delta {a.insertion_delta} is not >= 0")
    if a.insertion_scan:
        from .insertion_scan import checked_inserts
        try:
            a.insertion_scan = list(checked_inserts(list(dict.fromkeys(s.upper() for s in a.insertion_scan))))
        except ValueError as e:
            sys.exit(f"ERROR: --insertion-scan: {e}")
    _graph_only(a, "insertion_scan")
    if a.site_distance_all and a.site_distance is None:
        sys.exit("ERROR: --site-distance-all goes with --site-distance")
    if a.site_distance is not None and not 1 <= a.site_distance <= 8:
        sys.exit(f"ERROR: --site-distance {a.site_distance}: the number of substitutions lies in 1 .. 8")
    _graph_only(a, "site_distance")
    if a.null_seed is not None and a.shuffle_null is None:
        sys.exit("ERROR: --null-seed goes with --shuffle-null")
    if a.null_seed is not None and not 0 <= a.null_seed < 2**64:
        sys.exit(f"ERROR: --null-seed {a.null_seed} outside [0, 2^64 - 1]")
    if a.null_order is not None and a.shuffle_null is None:
        sys.exit("ERROR: --null-order goes with --shuffle-null")
    if a.shuffle_null is not None and not 1 <= a.shuffle_null <= 2**20:
        sys.exit(f"ERROR: --shuffle-null {a.shuffle_null} outside [1, 2^20]")
    _graph_only(a, "shuffle_null")
    if a.pair_gap is not None and not a.hit_pairs:
        sys.exit("ERROR: --pair-gap goes with --hit-pairs")
    if a.pair_gap is not None and a.pair_gap[0] > a.pair_gap[1]:
        sys.exit(f"ERROR: --pair-gap MIN MAX: {a.pair_gap[0]} > {a.pair_gap[1]}")
    _graph_only(a, "hit_pairs")
    if (a.linkage_flank is not None or a.linkage_r2 is not None) and not a.hit_linkage:
        sys.exit("ERROR: --linkage-flank and --linkage-r2 go with --hit-linkage")
    if a.linkage_flank is not None and a.linkage_flank < 0:
        sys.exit(f"ERROR: --linkage-flank {a.linkage_flank} < 0")
    if a.linkage_r2 is not None and not 0.0 <= a.linkage_r2 <= 1.0:
        sys.exit(f"ERROR: --linkage-r2 {a.linkage_r2} outside [0, 1]")
    _graph_only(a, "hit_linkage")
    _graph_only(a, "hit_alleles")
    if not from_vg and (from_graph == bool(a.sequences) or (from_graph and not (a.linear_genome and a.vcf and a.bedfile))):
        sys.exit("ERROR: give -g XG / -d DIR with -b BED, or -s DIR, or all of -l FASTA -v VCF -b BED")
    if a.cores <= 0:
        import os
        a.cores = os.cpu_count() or 1
    wf = _Workflow(a)
    start = time.time()
    motifs = []
    for mfile in a.motif:
        # the Motif objects come back without their score distribution: the DP runs on the GPU
        # when compute_results uploads the motif
        motifs += get_motif_pwm(mfile, wf, a.cores, a.debug, pvalue_matrix=False)
    graphs, region_lists = [], []
    if from_graph:
        from .extract_regions import DeviceGraph, GraphIndex, compute_results_from_graph, read_bed_regions
        for bed_chrom, regs in read_bed_regions(a.bedfile, a.debug).items():
            chrom = a.chroms_prefix + bed_chrom.split("chr")[1]      # extract_regions.py:122,137
            index = GraphIndex.from_fasta_vcf(a.linear_genome, a.vcf, chrom, allow_skipped=not a.strict_variants)
            if a.verbose:
                print(f"{chrom}: {len(index.pos)} variant sites ({int((index.ins_len > 0).sum())} insertions, "
                      f"{int((index.del_len > 0).sum())} deletions), {index.n_haplotypes} haplotypes, "
                      f"{index.skipped} ALT alleles left out")
            graphs.append(DeviceGraph(index))
            region_lists.append(regs)
    sequences_loc = None
    if from_vg:
        # the reference's own sequence (grafimo.py:176-183); `compute_results` above is ours, so scan_graph leaves a manifest
        # and every motif is scored where its walks are enumerated
        from .extract_regions import scan_graph
        sequences_loc = scan_graph({int(m.width) for m in motifs}, wf, a.debug)
    # a motif set is scored in ONE call: per width one ingest / one enumeration of the walks, up to three motifs per pass
    shared = None
    if len(motifs) >= 2:
        if from_graph:
            from .extract_regions import compute_results_from_graph_many
            shared = compute_results_from_graph_many(motifs, graphs, region_lists, a.debug, wf)
        else:
            shared = compute_results_many(motifs, sequences_loc if from_vg else a.sequences, a.debug, wf)
    for k, motif in enumerate(motifs):
        if shared is not None:
            res = shared[k]
        elif from_vg:
            res = compute_results(motif, sequences_loc, a.debug, wf)
        elif from_graph:
            res = compute_results_from_graph(motif, graphs, region_lists, a.debug, wf)
        else:
            res = compute_results(motif, a.sequences, a.debug, wf)
        if a.text_only:
            print_results(res, a.debug)
        else:
            write_results(res, motif, len(motifs), wf, a.debug)

    def source(table):
        """-> (graph, regions, the first chromosome's GraphIndex) as the tables' compute_* take them"""
        if not from_vg:
            return graphs, region_lists, graphs[0].index
        from .extract_regions import _manifest_prep, read_manifest
        manifest = read_manifest(sequences_loc)
        if manifest is None:
            sys.exit(f"ERROR: {_GRAPH_TABLES[table][0]} needs the graph; scan_graph left TSV rows, which carry no "
                     f"{_GRAPH_TABLES[table][1]}")
        return manifest, None, _manifest_prep(manifest).graphs[0].index

    def groups(first_index):
        """--haplotype-groups FILE -> {group: [haplotype columns]}, or None"""
        if not a.haplotype_groups:
            return None
        from .graph_tables import haplotype_column_names
        from .hit_alleles import read_haplotype_groups
        return read_haplotype_groups(a.haplotype_groups, haplotype_column_names(first_index))

    def emit(tables, write, show, count):
        """a table per motif: printed with -f like the report (no file written), else written and its size reported"""
        for motif, t in zip(motifs, tables):
            if a.text_only:
                show(t)
                continue
            print(f"{count(t)} written to {write(t, motif, len(motifs), wf)}")

    if a.variant_effects:
        from .variant_effects import compute_variant_effects_many, write_variant_effects
        graph, regions, _ = source("variant_effects")
        emit(compute_variant_effects_many(motifs, graph, regions, a.debug, wf), write_variant_effects,
             lambda t: print(t.to_string(index=False)), lambda t: f"{len(t)} variant effect rows")
    if a.haplotype_hits:
        from .haplotype_hits import compute_haplotype_hits_many, print_haplotype_hits, write_haplotype_hits
        graph, regions, _ = source("haplotype_hits")
        emit(compute_haplotype_hits_many(motifs, graph, regions, a.debug, wf), write_haplotype_hits, print_haplotype_hits,
             lambda hh: f"{hh.counts.shape[0]} x {hh.counts.shape[1]} haplotype hit counts")
    if a.haplotype_scores:
        from .haplotype_scores import compute_haplotype_scores_many, print_haplotype_scores, write_haplotype_scores
        graph, regions, _ = source("haplotype_scores")
        emit(compute_haplotype_scores_many(motifs, graph, regions, a.debug, wf), write_haplotype_scores, print_haplotype_scores,
             lambda hs: f"{hs.best.shape[0]} x {hs.best.shape[1]} haplotype best scores")
    if a.haplotype_affinity:
        from .haplotype_affinity import compute_haplotype_affinity_many, print_haplotype_affinity, write_haplotype_affinity
        graph, regions, _ = source("haplotype_affinity")
        emit(compute_haplotype_affinity_many(motifs, graph, regions, a.debug, wf,
                                             temperature=1.0 if a.affinity_temperature is None else a.affinity_temperature),
             write_haplotype_affinity, print_haplotype_affinity,
             lambda ha: f"{ha.sums.shape[0]} x {ha.sums.shape[1]} haplotype affinities")
    if a.variant_affinity:
        from .variant_affinity import compute_variant_affinity_many, print_variant_affinity, write_variant_affinity
        graph, regions, _ = source("variant_affinity")
        emit(compute_variant_affinity_many(motifs, graph, regions, a.debug, wf,
                                           temperature=1.0 if a.affinity_temperature is None else a.affinity_temperature,
                                           min_abs_delta=a.variant_affinity_delta or 0.0),
             write_variant_affinity, print_variant_affinity, lambda va: f"{len(va)} variant affinity rows")
    if a.hit_alleles:
        from .hit_alleles import compute_hit_alleles_many, print_hit_alleles, write_hit_alleles
        graph, regions, first_index = source("hit_alleles")
        emit(compute_hit_alleles_many(motifs, graph, regions, a.debug, wf, haplotype_groups=groups(first_index)),
             write_hit_alleles, print_hit_alleles, lambda ha: f"{len(ha)} hit allele rows")
    if a.hit_pairs:                                    # (one table per call, not per motif)
        from .hit_pairs import compute_hit_pairs, print_hit_pairs, write_hit_pairs
        graph, regions, first_index = source("hit_pairs")
        min_gap, max_gap = a.pair_gap if a.pair_gap is not None else (0, 50)
        hp = compute_hit_pairs(motifs, graph, regions, a.debug, wf, haplotype_groups=groups(first_index), min_gap=min_gap,
                               max_gap=max_gap)
        if a.text_only:                                # -f: printed like the report, no file written
            print_hit_pairs(hp)
        else:
            print(f"{len(hp)} hit pair rows written to {write_hit_pairs(hp, wf)}")
    if a.hit_linkage:
        from .hit_linkage import compute_hit_linkage_many, print_hit_linkage, write_hit_linkage
        graph, regions, _ = source("hit_linkage")
        emit(compute_hit_linkage_many(motifs, graph, regions, a.debug, wf,
                                      flank=10000 if a.linkage_flank is None else a.linkage_flank,
                                      min_r2=0.8 if a.linkage_r2 is None else a.linkage_r2),
             write_hit_linkage, print_hit_linkage, lambda hl: f"{len(hl)} hit linkage rows")
    hc = None
    if a.haplotype_classes:                            # (the classes once per call, a table per motif)
        from .haplotype_classes import (compute_haplotype_class_table_many, compute_haplotype_classes, print_haplotype_classes,
                                        write_haplotype_class_members, write_haplotype_classes)
        graph, regions, first_index = source("haplotype_classes")
        hc = compute_haplotype_classes(graph, regions, a.debug, wf, haplotype_groups=groups(first_index))
        emit(compute_haplotype_class_table_many(motifs, graph, regions, a.debug, wf,
                                                temperature=1.0 if a.affinity_temperature is None else a.affinity_temperature,
                                                min_haplotypes=a.class_min_haplotypes or 1, classes=hc),
             write_haplotype_classes, print_haplotype_classes, lambda t: f"{len(t)} haplotype class rows")
        if not a.text_only:
            print(f"{hc.class_of.shape[0]} x {hc.class_of.shape[1]} haplotype class members written to "
                  f"{write_haplotype_class_members(hc, wf)}")
    if a.haplotype_sequences:                          # (motif-independent: once per call; the classes of --haplotype-classes serve)
        from .haplotype_sequences import (compute_haplotype_sequences, haplotype_sequence_paths, print_haplotype_sequence_versions,
                                          write_haplotype_sequence_versions, write_haplotype_sequences_fasta)
        graph, regions, first_index = source("haplotype_sequences")
        hs = compute_haplotype_sequences(graph, regions, a.debug, wf, haplotype_groups=groups(first_index), classes=hc)
        if a.text_only:                                # -f: printed like the report, no file written
            print_haplotype_sequence_versions(hs)
        else:
            fasta, tsv = haplotype_sequence_paths(wf)
            print(f"{len(hs)} haplotype sequences written to {write_haplotype_sequences_fasta(hs, fasta)}")
            print(f"{len(hs)} haplotype sequence versions written to {write_haplotype_sequence_versions(hs, tsv)}")
    if a.query_variants:
        from .query_variants import (MAX_ALLELE, compute_query_variants_many, normalise, print_query_variants, read_query_vcf,
                                     write_query_variant_contexts, write_query_variants)
        graph, regions, first_index = source("query_variants")
        variants, too_long = [], 0
        for v in read_query_vcf(a.query_variants):
            _, nref, nalt = normalise(v[1], v[3], v[4])
            if max(len(nref), len(nalt)) > MAX_ALLELE or not (nref or nalt):
                too_long += 1
                continue
            variants.append(v)
        if too_long:
            print(f"WARNING: {too_long} query variants with an allele of more than {MAX_ALLELE} bases after trimming, or with "
                  "REF equal to ALT, were skipped", file=sys.stderr)
        tables = compute_query_variants_many(motifs, graph, variants, a.debug, wf, haplotype_groups=groups(first_index),
                                             temperature=1.0 if a.affinity_temperature is None else a.affinity_temperature,
                                             all_variants=a.query_all, skip_unusable=True)
        emit(tables, write_query_variants, print_query_variants, lambda t: f"{len(t)} query variant rows")
        if not a.text_only:
            for motif, t in zip(motifs, tables):
                print(f"{len(t.contexts_frame())} query variant context rows written to "
                      f"{write_query_variant_contexts(t, motif, len(motifs), wf)}")
    # the sequence scans: (asked for, the module's and the source's name, the noun of the printed lines, what
    # compute_<name>_many takes beyond the shared arguments)
    temperature = 1.0 if a.affinity_temperature is None else a.affinity_temperature
    for asked, name, noun, positional, named in (
            (a.mutation_scan, "mutation_scan", "mutation scan", (),
             dict(temperature=temperature, delta=a.mutation_delta, all_rows=a.mutation_all)),
            (a.indel_scan, "indel_scan", "indel scan", (),
             dict(temperature=temperature, delta=a.indel_delta, all_rows=a.indel_all)),
            (a.deletion_scan, "deletion_scan", "deletion scan", (a.deletion_scan,),
             dict(temperature=temperature, delta=a.deletion_delta, all_rows=a.deletion_all)),
            (a.substitution_scan, "substitution_scan", "substitution scan", (a.substitution_scan, a.substitution_map or "transversion"),
             dict(temperature=temperature, delta=a.substitution_delta, all_rows=a.substitution_all)),
            (a.insertion_scan, "insertion_scan", "insertion scan", (a.insertion_scan,),
             dict(temperature=temperature, delta=a.insertion_delta, all_rows=a.insertion_all)),
            (a.site_distance is not None, "site_distance", "site distance", (),
             dict(max_edits=a.site_distance, all_rows=a.site_distance_all))):
        if not asked:
            continue
        module = importlib.import_module(f".{name}", __package__)
        compute, write, write_summary, show = (getattr(module, f"compute_{name}_many"), getattr(module, f"write_{name}"),
                                               getattr(module, f"write_{name}_summary"), getattr(module, f"print_{name}"))
        graph, regions, first_index = source(name)
        tables = compute(motifs, graph, regions, a.debug, wf, *positional, haplotype_groups=groups(first_index), **named)
        emit(tables, write, show, lambda t: f"{len(t)} {noun} rows")
        if not a.text_only:
            for motif, t in zip(motifs, tables):
                print(f"{len(t.summary_frame())} {noun} summary rows written to {write_summary(t, motif, len(motifs), wf)}")
    if a.mutation_profile:                             # (one table per call: the scan folded over the motif set)
        from .mutation_profile import (compute_mutation_profile, print_mutation_profile, write_mutation_profile,
                                       write_mutation_profile_summary)
        graph, regions, first_index = source("mutation_profile")
        mp = compute_mutation_profile(motifs, graph, regions, a.debug, wf, haplotype_groups=groups(first_index),
                                      temperature=temperature, delta=a.mutation_profile_delta, all_rows=a.mutation_profile_all)
        if a.text_only:                                # -f: printed like the report, no file written
            print_mutation_profile(mp)
        else:
            print(f"{len(mp)} mutation profile rows written to {write_mutation_profile(mp, wf)}")
            print(f"{len(mp.summary_frame())} mutation profile summary rows written to {write_mutation_profile_summary(mp, wf)}")
    if a.shuffle_null is not None:                     # (a table per motif, and one row per motif for the whole call)
        from .shuffle_null import (compute_shuffle_null_many, print_motif_enrichment, print_shuffle_null, write_motif_enrichment,
                                   write_shuffle_null)
        graph, regions, first_index = source("shuffle_null")
        tables = compute_shuffle_null_many(motifs, graph, regions, a.debug, wf, haplotype_groups=groups(first_index),
                                           temperature=1.0 if a.affinity_temperature is None else a.affinity_temperature,
                                           replicates=a.shuffle_null, seed=a.null_seed or 0, order=a.null_order or 1)
        emit(tables, write_shuffle_null, print_shuffle_null, lambda t: f"{len(t)} shuffle null rows")
        if a.text_only:
            print_motif_enrichment(tables)
        else:
            print(f"{len(tables)} motif enrichment rows written to {write_motif_enrichment(tables, wf)}")
    if sequences_loc:
        import shutil
        shutil.rmtree(sequences_loc, ignore_errors=True)
    print("Elapsed time %.2fs" % (time.time() - start))


if __name__ == "__main__":
    main()
