"""The command line with all six graph tables asked for in ONE run: every file it writes equals, byte for byte, what the
table's own compute_* and write_* give in-process for the same inputs."""
import contextlib
import io
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
TABLES = ["variant_effects", "haplotype_hits", "haplotype_scores", "hit_alleles", "hit_pairs", "hit_linkage"]


def test_all_six_tables_in_one_run(tmp_path):
    from grafimo_amd import __main__ as cli
    from grafimo_amd import haplotype_hits, haplotype_scores, hit_alleles, hit_linkage, hit_pairs, variant_effects
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex, read_bed_regions
    inputs = ["-m", os.path.join(GOLD, "MA0139.1.meme"), "-l", os.path.join(GOLD, "xy.fa"), "-v", os.path.join(GOLD, "xy2.vcf.gz"),
              "-b", os.path.join(GOLD, "regions.bed"), "-t", "0.05"]
    flags = ["--" + t.replace("_", "-") for t in TABLES]
    out = tmp_path / "cli"
    r = subprocess.run([sys.executable, "-m", "grafimo_amd"] + inputs + ["-o", str(out)] + flags, check=True, cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=600, capture_output=True, text=True)
    report = ["grafimo_out.gff", "grafimo_out.html", "grafimo_out.tsv"]
    assert sorted(os.listdir(out)) == sorted(report + [f"grafimo_{t}.tsv" for t in TABLES])
    # the tables were made and reported in the order of the flags' blocks
    told = [re.sub(r"^[\d x]+", "", line.split(" written to ")[0]) for line in r.stdout.splitlines() if " written to " in line]
    assert told == ["variant effect rows", "haplotype hit counts", "haplotype best scores",
                    "hit allele rows", "hit pair rows", "hit linkage rows"]
    # the same inputs in-process, as the command line prepares them
    a = cli.get_parser().parse_args(inputs + ["-o", str(tmp_path / "own")])
    wf = cli._Workflow(a)
    with contextlib.redirect_stdout(io.StringIO()):
        motifs = cli.get_motif_pwm(a.motif[0], wf, 1, False, pvalue_matrix=False)
        assert len(motifs) == 1
        graphs, regions = [], []
        for bed_chrom, regs in read_bed_regions(a.bedfile, False).items():
            graphs.append(DeviceGraph(GraphIndex.from_fasta_vcf(a.linear_genome, a.vcf, bed_chrom.split("chr")[1],
                                                                  allow_skipped=True)))
            regions.append(regs)
        assert len(graphs) == 2
        call = (motifs, graphs, regions, False, wf)
        per_motif = [(variant_effects.compute_variant_effects_many, variant_effects.write_variant_effects),
                     (haplotype_hits.compute_haplotype_hits_many, haplotype_hits.write_haplotype_hits),
                     (haplotype_scores.compute_haplotype_scores_many, haplotype_scores.write_haplotype_scores),
                     (hit_alleles.compute_hit_alleles_many, hit_alleles.write_hit_alleles),
                     (hit_linkage.compute_hit_linkage_many, hit_linkage.write_hit_linkage)]
        paths = [write(compute(*call)[0], motifs[0], 1, wf) for compute, write in per_motif]
        paths.append(hit_pairs.write_hit_pairs(hit_pairs.compute_hit_pairs(*call), wf))
    assert sorted(os.path.basename(p) for p in paths) == sorted(f"grafimo_{t}.tsv" for t in TABLES)
    for p in paths:
        own, got = open(p, "rb").read(), open(out / os.path.basename(p), "rb").read()
        assert own == got and own.endswith(b"\n"), os.path.basename(p)
