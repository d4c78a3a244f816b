"""eagleeverything_amd -- MI355X (gfx950) backend for the Eagle/WMAM association-mapping hot path.

The product is libeaglehip.so (HIP kernels + C ABI, include/eagle_hip.h).  This package is the host-side
mirror of the reference interface used by tests, bench.py and the sharded multi-GPU driver:

  rcpp_api   -- ReadBlock, calculateMMt_rcpp, calculate_a_and_vara_rcpp, calculate_reduced_a_rcpp
  r_api      -- calculateMMt, calcMMt, calculate_a_and_vara, find_qtl (the R wrappers' marshalling rules); the QC chain
                MarkerStats / FilterMarkers / LDPrune / SampleStats / Relatedness; grm_weights, grm_from_gram, GRM, PCA;
                Score, ProjectPCA, MarkerEffects, Predict (the fitted model used on any panel with the same markers);
                GWAS (per-marker mixed-model tests: the P3D score test and the exact test with delta re-estimated), lmm_host
                SetTest (burden and SKAT tests of marker sets under the mixed model), settest_host, skat_pvalue,
                sets_from_windows, sets_from_table;
                MaxT (max(T) permutation p-values of every marker: EMP1 and the family-wise EMP2), maxt_host,
                maxt_permutations_host, maxt_merge;
                HapLD, HapBlocks (pairwise haplotype EM, D' and haplotype blocks), hap_ld_host, hap_blocks_host, sets_from_blocks;
                TDT (the transmission disequilibrium test of parent-offspring trios with max(T) flips within families), tdt_host,
                tdt_families, tdt_summary, tdt_merge;
                ReadMarker(type="VCF"), VcfToBed (a VCF file's GT fields decoded on the device into a PLINK binary fileset, missing
                calls kept missing for every bed= route), vcf_to_bed_host
  glmm       -- GLMM (case/control association under the logistic mixed model: GMMAT's score test with saddlepoint p-values),
                null_fit, spa, spa_host, spa_pvalues; r_api.GLMM forwards to it
  host_model -- dense n x n model algebra that stays on host LAPACK by design
  sharded    -- marker-sharded multi-GPU scan / MM^T (one process per GPU, torch.distributed over RCCL)
  synth      -- seeded synthetic genotypes of the benchmark shapes
"""
__all__ = ["rcpp_api", "r_api", "host_model", "synth"]
