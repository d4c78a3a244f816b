/*
 * eagle_hip.h -- C ABI of libeaglehip.so, the MI355X (gfx950) backend for the Eagle/WMAM hot path.
 *
 * The drop-in boundary of the reference is the .Call table of Eagle.so
 * (E/src/RcppExports.cpp:154-170, E/ = MyPackage/Eagle/).  The functions of section 1 below are what the
 * bodies of the reference's exported C++ functions are replaced with; each one cites the interface it
 * replaces.  The R-side binding (plain R C API, no Rcpp) is shown in INTEGRATION.md and in
 * eagleeverything_amd/shim/ (one Rcpp-typed translation unit per exported function + eagle_backend.h).
 *
 * Conventions
 *   - plain pointers and sizes only; matrices crossing section 1 are COLUMN-major doubles (R / Eigen).
 *   - every function returns an int status: 0 ok, < 0 hard error (text via eagle_last_error), 1 = the
 *     reference's "soft" sentinel return (message printed, placeholder value written, see each function).
 *   - selected_loci is passed as the raw R doubles (NA = NaN).  Masking fires iff element 0 is not NA
 *     (calculateMMt_rcpp.cpp:88, calculate_a_and_vara_rcpp.cpp:79, calculate_reduced_a_rcpp.cpp:74).
 *   - caller owns every pointer it passes; nothing is retained past return except the HBM-resident
 *     genotype cache inside the ctx (keyed by path, size, mtime), freed by eagle_close / eagle_drop_cache.
 *   - no function throws; none calls back except through the message callback, on the calling thread.
 *   - there is NO CPU fallback: without a gfx950 device eagle_open fails.
 */
#ifndef EAGLE_HIP_H
#define EAGLE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EAGLE_OK 0
#define EAGLE_SOFT_SENTINEL 1
#define EAGLE_ERR_OPEN (-1)    /* ReadBlock.cpp:42-45: "ERROR: Could not open <file>" */
#define EAGLE_ERR_FORMAT (-2)  /* short file / short line / character outside '0'..'2' */
#define EAGLE_ERR_ARG (-3)
#define EAGLE_ERR_NOMEM (-4)
#define EAGLE_ERR_HIP (-5)
#define EAGLE_ERR_NODEVICE (-6)

typedef struct eagle_ctx eagle_ctx;

/* Receives what the reference sends through its `message` R closure argument
 * (calculateMMt_rcpp.cpp:36,107; calculate_a_and_vara_rcpp.cpp:69,124). */
typedef void (*eagle_message_fn)(const char* text, void* user);

/* ---------------------------------------------------------------------------------------------
 * 0. Context
 * ------------------------------------------------------------------------------------------- */
/* Opens HIP device `device` (must be gfx950).  Returns NULL on failure; the reason is available from
 * eagle_open_error().  One ctx per device; a process that drives several GPUs opens one ctx each. */
eagle_ctx* eagle_open(int device);
/* Several GPUs of one node behind ONE context -- the reference's unused hook is AM(..., ngpu) (E/R/AM.R:185-196, forced to 0 at
 * :214, handed to .find_qtl at :450-455).  eagle_calculateMMt / eagle_calculate_a_and_vara / eagle_calculate_reduced_a then
 * split the file's markers into ndev contiguous ranges (boundaries at multiples of 256 markers), one host thread + stream
 * per device, all joined before the call returns; results land in the caller's arrays exactly as with one device
 * (bit-identical: integer MM^T, per-marker scan, and a certification that exchanges the shards' bounds).  Exchange steps:
 * one int32 sum of the partial MM^T to the first device (ncclReduce over xGMI), the rows of W = S V S shared and
 * all-gathered (ncclAllGather), 8 bytes per device through the host for the certificate.  RCCL is dlopen()ed on first use;
 * a list that names one device twice (the one-GPU test configuration) or EAGLE_HIP_COLLECTIVES=host stages the sum through
 * device copies and computes W on every device instead.
 * eagle_open_env: the devices of EAGLE_HIP_DEVICES="0,1,..." if set, else EAGLE_HIP_DEVICE, else device 0. */
eagle_ctx* eagle_open_devices(const int* devices, int ndev);
eagle_ctx* eagle_open_env(void);
int eagle_device_count(eagle_ctx* ctx);
const char* eagle_open_error(void);
void eagle_close(eagle_ctx* ctx);
const char* eagle_last_error(eagle_ctx* ctx);
void eagle_set_message_callback(eagle_ctx* ctx, eagle_message_fn fn, void* user);
/* Drops HBM-resident genotype copies kept between calls. */
/* (round 4: also the grow-only workspaces held between calls -- the scan arena, a background reservation of it, the workspace of
 * the int8 W products; the next call allocates them again) */
void eagle_drop_cache(eagle_ctx* ctx);
/* "gfx950", CU count, HBM bytes -- for logs and bench JSON. */
int eagle_device_info(eagle_ctx* ctx, char* arch_out, int arch_len, int* cu_count, int64_t* hbm_bytes);
/* vara kernel: 1 (default) = exact int8 digit slices of W on v_mfma_i32_32x32x32_i8, 0 = fp64 MFMA
 * (v_mfma_f64_16x16x4_f64; also taken automatically when n is too large for the int32 tile sums).
 * eagle_set_scan_slices: S = 1..8 base-256 digits of the off-diagonal part of W, or 0 (default) = chosen per call:
 * the smallest S in 3..7 whose worst-case bound is below the budget (eagle_set_scan_budget; by default 1e-7 first, 5e-7 as the fallback:
 * eagle_last_scan_budget) times 0.5 * sum_k |W_kk| -- at most half of the 1e-6 relative tolerance of this path, relative to the smallest diagonal term a marker can have (at least half of its genotypes are
 * non-zero in the g-1 coding); measured errors are ~1000x below the bound.  The diagonal term
 * sum_k m_ik^2 W_kk is evaluated in fp64; every vara_i then differs from the exact m_i^T W m_i by at most
 * (sum_j |m_ij|)^2 * 2^(e+1-8S), max_{j!=k} |W_jk + W_kj| < 2^e (or < 1.96 * 2^e: the exponent is lowered by one when the largest
 * entry's mantissa leaves the balanced digits room), plus fp64 rounding of an n-term and an S-term sum. */
int eagle_set_scan_mode(eagle_ctx* ctx, int mode);
int eagle_set_scan_slices(eagle_ctx* ctx, int nslices);
/* Round 3.  The relative digit budget of the int8 scan, 1e-12 .. 5e-7 (5e-7 = half of the path's 1e-6 tolerance).  A context whose
 * budget was never set tries 1e-7 first and falls back to 5e-7 (eagle_last_scan_budget, below); this call makes its argument the only
 * budget, 0 restores that default policy.  It enters twice: the automatic digit count is the smallest S whose bound keeps a typical
 * marker inside the budget, and the certificate sends every marker whose OWN bound exceeds 1.8 x the budget in force (1.8e-7 under the
 * tight default, 0.9e-6 under the fallback) to the fp64 kernel.  With the automatic count the library also tries ONE DIGIT FEWER than the worst-case bound asks for, under a spectral
 * bound of the truncation error: |error_i| <= (u/2)(||Ds||_2 + (n_pad-1)/2) sum_j m'_ij^2, Ds = the symmetrised last digit of W,
 * ||Ds||_2^2 <= max row sum of |Ds Ds| from an exact int8 MFMA Gram product, or, one level down, max_j (Ds Ds)_jj + ||offdiag(Ds Ds)||_2
 * with the off-diagonal part bounded the same way (csrc/eagle_i8mfma.hip, k_spectral_decide) -- rigorous, deterministic, a function of
 * W alone.  At n = 10,000 this takes the scan of an AM() run from 4 digit slices to 3, with the default budget and with 1e-7 alike. */
int eagle_set_scan_budget(eagle_ctx* ctx, double relative_budget);
/* How the digits of W are rounded (digit-slice mode).  0 (default): to nearest -- every vara_i is GUARANTEED within
 * l1_i^2 / 2 * 2^(e+1-8S) of the exact quadratic form (l1_i = sum_j |m'_ij| of the re-centred marker).  1: stochastic
 * rounding -- each entry rounded down or up at random with the probabilities that make it unbiased, from a counter-based
 * generator keyed by the entry's position (independent of the data, reproducible).  The truncation errors are then
 * independent and zero-mean, Hoeffding's inequality bounds marker i's error by 8.355 q2_i 2^(e+1-8S), q2_i = sum_j m'_ij^2,
 * with failure probability below 1e-30 per marker (1e-22 over every marker of every scan of an AM() run), and the automatic
 * digit count drops by one (C2 / C3: S = 3 instead of 4, a quarter less matrix work).  The certificate is then a
 * probabilistic one; flagging, fp64 re-evaluation and the selected marker work exactly as in mode 0.  In the
 * device-resident entry points the same switch is bit 8 of the `nslices` argument (EAGLE_SLICES_STOCHASTIC). */
#define EAGLE_SLICES_STOCHASTIC 0x100
int eagle_set_scan_rounding(eagle_ctx* ctx, int stochastic);
/* Round 4.  Which engine forms W = S (V S) for a digit-slice scan (calculate_a_and_vara_rcpp.cpp:97-98).  1 (default): from 4,096
 * padded individuals up, the two n^3 products run on the int8 MFMA from exact base-256 digit slices of the off-diagonal parts of S, V
 * and X = V S (diagonal parts exactly, in fp64), under a rigorous Frobenius-norm bound eta of the error of the W delivered; the scan's
 * per-marker certificate adds eta * sum_j m'_ij^2 to its bound, the correction vector of the re-centred markers comes from
 * r = S (V (S 1)) in fp64, and the markers the certificate re-evaluates are computed as m^T (S (V (S m))) in fp64.  A call whose
 * operands the configurations on offer cannot certify to 2 % of the digit budget (wild scaling, cancelling V, non-finite or visibly
 * asymmetric matrices, no workspace) DECLINES and the fp64 GEMM runs as before.  0: always the fp64 GEMM.  2: the int8 engine at any
 * size (tests).  eagle_set_scan_mode(0) never uses it.  csrc/eagle_w8.hip. */
int eagle_set_w_mode(eagle_ctx* ctx, int mode);
typedef struct eagle_w_info {
    int int8;            /* 1: the W of the last scan_operands call came from the int8 engine */
    int declined;        /* else why not: 1 non-finite, 2 asymmetric / no yardstick, 3 / 4 no configuration for V S / S X, 5 no workspace,
                            6 the finished W failed the check against its own diagonal, 7 switched off or too small, 8 replaced by the fp64
                            products after the certificate overflowed */
    int k1, T1, pairs1;  /* V S: digits per operand, highest level p + q, int8 products (n_pad^3 MACs each) */
    int k2, T2, pairs2;  /* S X (upper triangle only) */
    double eta;          /* || folded W - truth ||_F bound; a marker's vara carries eta * sum_j m'_j^2 of it */
    double eta_x;        /* || X computed - V S ||_F bound */
    double target;       /* what the configurations were chosen for (0.02 x budget x estimate of mean |W_kk|) */
    double mean_diag;    /* mean |W_kk| of the W delivered */
    double asym_term;    /* share of eta that pays for || S - S^T ||_F, || V - V^T ||_F (measured) */
    int pipelined;       /* 1: eagle_calculate_a_and_vara formed V S column block by column block while V was still arriving over PCIe (on the
                            configuration of the context's last call, which the rule then confirmed: the bits are the same either way) */
    int pad;
} eagle_w_info;
int eagle_last_w_info(eagle_ctx* ctx, eagle_w_info* out);

/* ---------------------------------------------------------------------------------------------
 * 1. Reference-shaped entry points (host pointers, files on disk)
 * ------------------------------------------------------------------------------------------- */

/* Replaces  Eigen::MatrixXd ReadBlock(std::string asciifname, long start_row, long numcols,
 *           long numrows_in_block)               E/src/ReadBlock.cpp:16-68, RcppExports.cpp:9-21
 * out: numrows_in_block x numcols column-major, value (char-'0')-1.  The text tile is decoded on the
 * device (raw bytes -> HBM -> int8 -> fp64) and copied back. */
int eagle_read_block(eagle_ctx* ctx, const char* asciifname, long start_row, long numcols,
                     long numrows_in_block, double* out);

/* Replaces  Eigen::MatrixXd calculateMMt_rcpp(CharacterVector f_name_ascii, double max_memory_in_Gbytes,
 *           int num_cores, NumericVector selected_loci, std::vector<long> dims, bool quiet,
 *           Function message)                    E/src/calculateMMt_rcpp.cpp:19-185, RcppExports.cpp:37-52
 * dims = (n, L) of M.ascii.  MMt_out: n x n column-major.  max_memory_in_Gbytes bounds HOST staging
 * (the genotype tiles are streamed through pinned memory); num_cores bounds host reader threads.
 * A file that does not fit in HBM (or exceeds the environment variable EAGLE_HIP_MAX_RESIDENT_GB) is streamed in
 * marker windows and the exact integer partial products are accumulated; the same holds for the two scans below. */
int eagle_calculateMMt(eagle_ctx* ctx, const char* f_name_ascii, double max_memory_in_Gbytes, int num_cores,
                       const double* selected_loci, long n_selected, const long dims[2], int quiet,
                       double* MMt_out);

/* Replaces  Rcpp::List calculate_a_and_vara_rcpp(CharacterVector f_name_ascii, NumericVector selected_loci,
 *           Map<MatrixXd> inv_MMt_sqrt, Map<MatrixXd> dim_reduced_vara, double max_memory_in_Gbytes,
 *           std::vector<long> dims, VectorXd a, bool quiet, Function message)
 *                                                E/src/calculate_a_and_vara_rcpp.cpp:22-241, RcppExports.cpp:54-71
 * dims = (L, n) of Mt.ascii.  inv_MMt_sqrt, dim_reduced_vara: n x n column-major; a: n.
 * a_out, vara_out: L doubles each (the "a" and "vara" L x 1 matrices of the returned list).
 * Returns EAGLE_SOFT_SENTINEL with a_out[0] = vara_out[0] = 0 where the reference returns
 * List(a = 0, vara = 0) (:133-144). */
int eagle_calculate_a_and_vara(eagle_ctx* ctx, const char* f_name_ascii, const double* selected_loci,
                               long n_selected, const double* inv_MMt_sqrt, const double* dim_reduced_vara,
                               double max_memory_in_Gbytes, const long dims[2], const double* a, int quiet,
                               double* a_out, double* vara_out);

/* Replaces  Eigen::MatrixXd calculate_reduced_a_rcpp(CharacterVector f_name_ascii, double varG,
 *           Map<MatrixXd> P, Map<MatrixXd> y, double max_memory_in_Gbytes, std::vector<long> dims,
 *           NumericVector selected_loci, bool quiet, Function message)
 *                                                E/src/calculate_reduced_a_rcpp.cpp:20-171, RcppExports.cpp:73-90
 * dims = (n, L) of M; the file is Mt.ascii.  ar_out: L doubles.  Returns EAGLE_SOFT_SENTINEL with
 * ar_out[0] = 0 where the reference returns its 1 x 1 zero matrix (:94-103). */
int eagle_calculate_reduced_a(eagle_ctx* ctx, const char* f_name_ascii, double varG, const double* P,
                              const double* y, double max_memory_in_Gbytes, const long dims[2],
                              const double* selected_loci, long n_selected, int quiet, double* ar_out);

/* Replaces  Eigen::VectorXi extract_geno_rcpp(CharacterVector f_name_ascii, double max_memory_in_Gbytes,
 *           long selected_locus, std::vector<long> dims)   E/src/extract_geno_rcpp.cpp:16-89, RcppExports.cpp:128-141
 * Column `selected_locus` (0-based) of M.ascii as ints -1/0/1 (constructX appends it to the design matrix,
 * E/R/constructX.R:16-19).  dims = (n, L).  Served from the HBM-resident copy of the file when eagle_calculateMMt
 * has loaded it (always the case inside AM(), AM.R:403 vs :414-417); otherwise one character per line is read from
 * the file -- the reference parses the whole n x L file into doubles for this. */
int eagle_extract_geno(eagle_ctx* ctx, const char* f_name_ascii, double max_memory_in_Gbytes, long selected_locus,
                       const long dims[2], int* column_out);

/* ---------------------------------------------------------------------------------------------
 * 1b. Marker-file ingestion (the producers of M.ascii / Mt.ascii that ReadMarker() calls, E/R/create_ascii.R:27-58).
 *     Same results byte for byte; additionally the int8 images of both files stay resident in HBM under the OUTPUT
 *     paths, so the eagle_calculateMMt / eagle_calculate_a_and_vara calls that follow never parse text, and a 2-bit
 *     sidecar "<output>.e2b" (64-byte header + packed rows, a quarter of the text bytes) is left beside each text file:
 *     every loader of this library reads it instead of the text while the text file keeps the size and mtime recorded in
 *     it (EAGLE_HIP_SIDECAR=0 disables writing and reading).
 * ------------------------------------------------------------------------------------------- */

/* Replaces  std::vector<long> ReshapeM_rcpp(CharacterVector fnameM, CharacterVector fnameMt, std::vector<long> indxNA,
 *           std::vector<long> dims)              E/src/ReshapeM_rcpp.cpp:17-120 (called from E/R/ReshapeM.R:8, AM.R:345-366)
 * Drops the individuals indxNA (0-based, any order; dims = (n, L) of M) from M.ascii and Mt.ascii.  The results are named
 * fnameM + "tmp" and fnameMt + "tmp", as the reference names its files (:51,94); newdims_out = the reference's value, {lines of
 * the new M, length of the last line of M}.  A duplicate index or one outside [0, dims[0]) is EAGLE_ERR_ARG (the reference's
 * erase throws on the one and removes the wrong column on the other); a line of Mt that does not reach the largest index is
 * EAGLE_ERR_FORMAT.
 *   EAGLE_RESHAPE_FILES: writes both files, byte for byte what the reference writes (every kept line followed by '\n'), with
 *     parallel host I/O and no device work.  ctx may be NULL (errors then through eagle_last_error(NULL)).
 *   EAGLE_RESHAPE_VIEW: writes nothing.  The two names become aliases on this context (and every sub-context of an
 *     eagle_open_devices one): every call of this library that reads a file -- eagle_read_block, the MM^T and scan entry points,
 *     eagle_extract_geno, eagle_get_row_column (what the rewritten file would give), eagle_spectral_prepare -- reads the source
 *     file, its 2-bit sidecar or its resident HBM image through a keep-map of individuals, and gets exactly the int8 image the
 *     rewritten file would give, zero padding included: results are equal bit for bit.  A resident source Mt image is subset
 *     by one HBM gather (k_gather_cols_i8).  The alias's resident images are keyed by its name plus the source's size and mtime
 *     at registration; if a source changes after that, every call on the alias fails with EAGLE_ERR_FORMAT.  Registering the
 *     names again (either mode) replaces the view and drops the alias's images; eagle_drop_cache keeps the views, eagle_close
 *     frees them.  nNA == 0 gives an identity view.  A view belongs to ONE context: another process or context (a rank of
 *     eagleeverything_amd.sharded) that opens the alias path gets EAGLE_ERR_OPEN. */
#define EAGLE_RESHAPE_FILES 0
#define EAGLE_RESHAPE_VIEW 1
int eagle_reshape_m(eagle_ctx* ctx, const char* fnameM, const char* fnameMt, const long* indxNA, long nNA, const long dims[2], int mode,
                    long newdims_out[2]);

/* Replaces  std::vector<long> getRowColumn(std::string fname)      E/src/getRowColumn.cpp:20-72, RcppExports.cpp:143-151
 * dims_out = (lines, whitespace-separated tokens of the first line). */
int eagle_get_row_column(eagle_ctx* ctx, const char* fname, long dims_out[2]);

/* Replaces  bool createM_ASCII_rcpp(CharacterVector f_name, CharacterVector f_name_ascii, CharacterVector type,
 *           std::string AA, std::string AB, std::string BB, double max_memory_in_Gbytes, std::vector<long> dims,
 *           bool quiet, Function message, std::string missing)
 *                                                E/src/createM_ASCII_rcpp.cpp:18-106, RcppExports.cpp:92-111
 * type "PLINK": f_name is a ped file, dims = (individuals, 6 + 2*loci), AA/AB/BB/missing unused
 *               (E/src/CreateASCIInospace_PLINK.cpp:16-249: first-seen allele order, 0 / - = missing -> het);
 * otherwise   : a whitespace-separated genotype table, dims = (individuals, loci), tokens BB -> '2', AB -> '1',
 *               AA -> '0', missing -> '1'  (E/src/CreateASCIInospace.cpp:84-105).
 * Returns EAGLE_OK where the reference returns true, EAGLE_SOFT_SENTINEL where it prints its messages and returns
 * false (unknown token, unequal number of columns, third allele; eagle_last_error holds a one-line summary and the
 * output file keeps the rows converted before the failure, like the reference's). */
int eagle_create_M_ascii(eagle_ctx* ctx, const char* f_name, const char* f_name_ascii, const char* type, const char* AA,
                         const char* AB, const char* BB, double max_memory_in_Gbytes, const long dims[2], int quiet,
                         const char* missing);

/* Replaces  void createMt_ASCII_rcpp(CharacterVector f_name, CharacterVector f_name_ascii, CharacterVector type,
 *           double max_memory_in_Gbytes, std::vector<long> dims, bool quiet, Function message)
 *                                                E/src/createMt_ASCII_rcpp.cpp:14-247, RcppExports.cpp:113-126
 * f_name = M.ascii (dims = (n, L)), f_name_ascii = Mt.ascii to write (L lines of n characters).  The transpose runs on
 * the device from the resident image of M.ascii (loaded if it is not there; column windows if it does not fit). */
int eagle_create_Mt_ascii(eagle_ctx* ctx, const char* f_name, const char* f_name_ascii, const char* type,
                          double max_memory_in_Gbytes, const long dims[2], int quiet);

/* PLINK binary genotypes (no counterpart in the reference, whose PLINK route reads ped text): bed_path is a .bed file in SNP-major
 * mode -- 0x6c 0x1b 0x01, then one row of ceil(n/4) bytes per marker, individual 4b+q at bits 2q of byte b -- and dims = (n
 * individuals, L markers), the line counts of its .fam and .bim.  Writes what eagle_create_M_ascii followed by
 * eagle_create_Mt_ascii leave for the same genotypes: M.ascii (n lines of L characters), Mt.ascii (L lines of n characters), both
 * sidecars, both resident images when they fit, the summary messages.  Code 00 (homozygous A1) -> '0', 10 (heterozygous) and 01
 * (missing, the reference's missing -> heterozygote rule of CreateASCIInospace_PLINK.cpp:116-129) -> '1', 11 (homozygous A2) -> '2'.
 * With any genotype missing, the reference's "PLINK file contains missing alleles" warning is sent once; *n_missing_out (may be
 * NULL) = their number.  An image of M that does not fit the device (or EAGLE_HIP_MAX_RESIDENT_GB) costs one pass over the bed
 * file per band of individuals; the files are the same bytes either way.
 * EAGLE_ERR_OPEN: a file cannot be opened; EAGLE_ERR_FORMAT: not a .bed file, an individual-major one, or a size other than
 * 3 + L * ceil(n/4); EAGLE_ERR_ARG: n <= 0 or L <= 0.  A failed call leaves neither sidecar and no text file of the full size. */
int eagle_create_ascii_from_bed(eagle_ctx* ctx, const char* bed_path, const char* f_name_ascii_M, const char* f_name_ascii_Mt,
                                double max_memory_in_Gbytes, const long dims[2], int quiet, long* n_missing_out);

/* ---------------------------------------------------------------------------------------------
 * 1b-vcf. VCF ingestion (no counterpart in the reference): the GT fields of a VCF 4.x file decoded on the device into a PLINK binary
 *     fileset <prefix>.bed / .bim / .fam, which eagle_create_ascii_from_bed and every eagle_bed_* entry point then read -- with the
 *     missing calls of the VCF still missing (code 01), which the text and .ped routes cannot keep.  Agreement with the PLINK program or
 *     with bcftools is neither claimed nor tested: neither is available where this library is built.  Sex chromosomes, dosages (DS / GP),
 *     phase and the splitting of multi-allelic records are out of scope.  Single device: a multi-device context works on its first device.
 *
 *     1. Input.  Plain text (compressed files are the caller's to inflate; r_api.VcfToBed does it).  Lines end at '\n'; a '\r' before
 *        the '\n' is dropped; an unterminated last line is a line; empty lines are skipped anywhere.  Line numbers are 1-based and count
 *        every line of the file, skipped ones included.
 *     2. Header.  Lines that start with "##" are skipped.  The first other line must start with "#CHROM"; its tab-separated columns
 *        from the 10th on are the n sample names.  EAGLE_ERR_FORMAT with the line number: no #CHROM line (a data line before the
 *        header, or a file that ends without one), fewer than 10 columns, a sample name that is empty or contains a blank.
 *     3. Which data lines are kept: decided on the host from the nine fixed fields alone (CHROM POS ID REF ALT QUAL FILTER INFO
 *        FORMAT; a data line with fewer than nine is EAGLE_ERR_FORMAT).  A line is dropped and counted under the FIRST reason that holds:
 *        ALT contains a ',' (multiallelic); ALT is "." (no_alt); FORMAT is not "GT" and does not begin with "GT:" (no_gt); with
 *        EAGLE_VCF_SNPS_ONLY, REF or ALT is not one of A C G T, case-insensitive (not_snp); with EAGLE_VCF_PASS_ONLY, FILTER is
 *        neither "PASS" nor "." (filtered).  lines = the data lines seen = kept + the five drop counts.
 *        A kept line must have exactly n sample fields; otherwise EAGLE_ERR_FORMAT, naming the line and the count found.  The sample
 *        fields of a dropped line are never looked at.
 *     4. One sample field: the bytes up to the next tab or the line end.  GT is the field up to its first ':'; bytes after the first
 *        ':' are never looked at.  GT is cut at every '/' or '|' into k tokens (an empty GT is one empty token):
 *          k = 1, token "0" -> homozygous REF, counted haploid;   k = 1, token "1" -> homozygous ALT, counted haploid;
 *          k = 2, both tokens in {"0", "1"}: equal -> homozygous REF or homozygous ALT, different -> het;
 *          anything else -> missing; a missing GT whose tokens are not all "." is also counted malformed ("2/1", "10/1", "0/1/1",
 *          an empty field, an empty token).
 *     5. Output.  <prefix>.bed is SNP-major with the codes of 1b: 00 hom A1, 10 het, 01 missing, 11 hom A2, individual 4b+q at bits 2q
 *        of byte b, the unused bit pairs of a row's last byte zero.  By default A1 = ALT and A2 = REF (the PLINK program's import
 *        convention AS DOCUMENTED); EAGLE_VCF_A2_ALT makes A2 = ALT, so that the '2' allele of this library counts ALT copies.
 *        <prefix>.bim: one line per kept marker, CHROM \t ID \t 0 \t POS \t A1 \t A2, ID = CHROM:POS where the file has ".".
 *        <prefix>.fam: one line per sample, "name name 0 0 0 -9".  A failed call leaves none of the three files.
 *     6. Windows.  chunk_bytes caps the text staged per window (0: the staging rule of the eagle_bed_* calls, 64 MiB or a quarter of
 *        max_memory_in_Gbytes if less).  A window holds whole lines only and grows to the longest line when a line is longer than
 *        chunk_bytes; a line longer than a quarter of max_memory_in_Gbytes (or than 2^30 bytes) is EAGLE_ERR_ARG.  The host finds the
 *        newlines of a staged window, parses the fixed fields and sends the kept lines' table (first sample field, line end); the
 *        device finds the tabs, gives every field its ordinal, decodes GT, packs four codes a byte and counts per line (k_vcf_fields,
 *        k_vcf_pack).  The pread of window k runs under the device work of window k - 1 (the staging ring of the eagle_bed_* calls) and
 *        the .bed rows go out write-behind.  The files do not depend on chunk_bytes: the same file gives the same bytes at every value.
 *     7. Argument errors are decided before the context is used (ctx == NULL: the text is in eagle_open_error()): a NULL pointer,
 *        unknown flag bits, chunk_bytes < 0, an empty prefix.  dims_out = (n, kept markers); a file whose lines are all dropped is
 *        EAGLE_ERR_FORMAT (a fileset of no marker is none).
 * ------------------------------------------------------------------------------------------- */
#define EAGLE_VCF_A2_ALT 1
#define EAGLE_VCF_SNPS_ONLY 2
#define EAGLE_VCF_PASS_ONLY 4
typedef struct eagle_vcf_counts {
    long lines, kept, multiallelic, no_alt, no_gt, not_snp, filtered, missing, haploid, malformed;
} eagle_vcf_counts;

int eagle_vcf_to_bed(eagle_ctx* ctx, const char* vcf_path, const char* out_prefix, int flags, double max_memory_in_Gbytes, long chunk_bytes,
                     long dims_out[2], eagle_vcf_counts* counts_out);

/* ---------------------------------------------------------------------------------------------
 * 1b'. Marker QC (no counterpart in the reference, which leaves filtering to other tools): per-marker genotype counts from the
 *     genotypes this library already holds, and panels restricted to a list of markers.  Integer results only; allele
 *     frequencies, call rates and the filter rules are the caller's arithmetic on the counts (r_api.MarkerStats / FilterMarkers).
 *     Single device: a multi-device context works on its first device.  Argument errors are decided before the context is
 *     used; with ctx == NULL their text is in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */

/* counts_out[3 i .. 3 i + 2] = the numbers of '0', '1' and '2' characters of line i of Mt.ascii (dims = (n, L) of M: L lines of n
 * characters), from one HBM-bound pass over the int8 image (k_marker_counts: s = sum g, q = sum g^2 per row on v_dot4_i32_i8,
 * n2 = (q + s) / 2, n0 = (q - s) / 2, n1 = n - n0 - n2).  The file is read as every loader of this library reads it: its resident
 * image if there is one, else its 2-bit sidecar, else the text; the image stays resident when it fits, and a file that does not fit
 * (or exceeds EAGLE_HIP_MAX_RESIDENT_GB) is counted in row windows.  A VIEW alias of eagle_reshape_m gives the counts over the kept
 * individuals (dims[0] = their number).  Missing genotypes of the original data are heterozygotes by now and counted as such. */
int eagle_marker_counts(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], double max_memory_in_Gbytes, int32_t* counts_out);

/* The same from a SNP-major PLINK .bed file (the format and the checks of eagle_create_ascii_from_bed; dims = (n, L)), where missing
 * genotypes are still known: counts_out[4 i .. 4 i + 3] = homozygous A1 (code 00), heterozygous (10), homozygous A2 (11), missing
 * (01) of marker i, by popcounts on the two bit planes (k_bed_marker_counts); the unused bit pairs of a row's last byte are not
 * counted.  The rows are staged through pinned memory in windows of at most 64 MiB (a quarter of max_memory_in_Gbytes if less). */
int eagle_bed_marker_counts(eagle_ctx* ctx, const char* bed_path, const long dims[2], double max_memory_in_Gbytes, int32_t* counts_out);

/* The panel (fnameM, fnameMt; dims = (n, L) of M) restricted to the markers keep[0 .. nkeep) (0-based, strictly increasing): writes
 * outM (n lines of nkeep characters) and outMt (nkeep lines of n characters), byte for byte what eagle_create_M_ascii followed by
 * eagle_create_Mt_ascii leave for a genotype table that holds only those columns -- both sidecars, and both resident images under the
 * OUTPUT paths when they fit.  From resident sources the subset is made in HBM (row copies for Mt, k_gather_cols_i8 for M); a source
 * that is not resident is read in windows (the kept lines of Mt.ascii, bands of whole lines of M.ascii).  newdims_out = (n, nkeep).
 * EAGLE_ERR_ARG: an empty keep-list, an entry outside [0, L), a list that is not strictly increasing, an output path equal to an
 * input path or to the other output -- nothing has been written then.  A call that fails later leaves neither sidecar and no text
 * file of the full size (the rule of eagle_create_ascii_from_bed). */
int eagle_filter_markers(eagle_ctx* ctx, const char* fnameM, const char* fnameMt, const long dims[2], const long* keep, long nkeep,
                         const char* outM, const char* outMt, double max_memory_in_Gbytes, long newdims_out[2]);

/* ---------------------------------------------------------------------------------------------
 * 1b''. Linkage disequilibrium between markers (no counterpart in the reference): which markers of a panel are correlated, from
 *     integer dot products between rows of the int8 marker-major image on the int8 MFMA (csrc/eagle_ld.hip).  With g in
 *     {-1, 0, +1} over the n individuals of Mt.ascii (the kept ones of a VIEW alias; missing genotypes are heterozygotes), all int64:
 *         s_i = sum g,  q_i = sum g^2,  d_ij = sum g_i g_j,  c_ij = n d_ij - s_i s_j,  v_i = n q_i - s_i^2,  r^2_ij = c^2 / (v_i v_j).
 *     Markers i, j are IN LD AT t iff v_i > 0, v_j > 0 and (double)c * (double)c > t * ((double)v_i * (double)v_j), evaluated in
 *     exactly that order in fp64 (correctly rounded products, no sum): a restatement in numpy gives the same bits.  A monomorphic
 *     marker is in LD with nothing.  The file is read as eagle_marker_counts reads it (resident image, else sidecar, else text; a
 *     VIEW alias works); one that does not fit is processed in row windows with the bits of the resident pass.  Single device: a
 *     multi-device context works on its first device.  Argument errors (EAGLE_ERR_ARG: a NULL pointer, dims <= 0, and those named
 *     below) are decided before the context is used; with ctx == NULL their text is in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */

/* mask_out[i * W + (o - 1) / 64], W = ceil(window / 64), has bit (o - 1) % 64 set iff markers i and i + o (1 <= o <= window,
 * i + o < L) are in LD at r2; every other bit is clear.  *npairs_out = the number of set bits.  (s, q) come from k_marker_counts in
 * the same call.  Streamed windows overlap by `window` rows, so that no pair is lost or counted twice.
 * EAGLE_ERR_ARG: window outside [1, 256], r2 outside [0, 1] or NaN. */
int eagle_ld_window(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], long window, double r2, double max_memory_in_Gbytes,
                    uint64_t* mask_out, long* npairs_out);

/* dots_out[i * nloci + j] = d between marker i and marker loci[j] (0-based; repeats allowed), for every marker of the panel: L x nloci
 * int32, row-major.  r^2 follows from the counts of eagle_marker_counts (r_api.ld_r2_from_dots).
 * EAGLE_ERR_ARG: nloci outside [1, 64], a locus outside [0, L). */
int eagle_ld_dots(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const long* loci, long nloci, double max_memory_in_Gbytes,
                  int32_t* dots_out);

/* ---------------------------------------------------------------------------------------------
 * 1b'''. Sample QC (no counterpart in the reference): per-individual genotype counts, the pairwise identity-by-state counts that
 *     KING-robust kinship is made of, and the Hardy-Weinberg exact test per marker.  Genotypes are g in {-1, 0, +1} = AA, AB, BB as
 *     everywhere in this library; missing genotypes of the source are heterozygotes after ingestion.  L = the number of markers.  With
 *         D_ij = sum g_i g_j,   Q_ij = sum g_i^2 g_j^2,   q_i = Q_ii (homozygous genotypes of i),   h_i = L - q_i (heterozygous),
 *     all exact integers from two Gram products on the block-scaled fp4 MFMA (D = M M^T is eagle_calculateMMt's product; the operand
 *     of Q is the fp4 image of M with every code's sign bit cleared, byte & 0x77, written to a buffer of its own: the image cached
 *     with a resident file is never modified):
 *         ibs0_ij   = (Q_ij - D_ij) / 2          markers where i and j are opposite homozygotes (the difference is even)
 *         hethet_ij = L - q_i - q_j + Q_ij       markers where both are heterozygous
 *     and on the diagonal ibs0_ii = 0, hethet_ii = h_i.  KING-robust kinship is the caller's arithmetic (r_api.king_from_counts), in
 *     fp64 in exactly this order:  phi_ij = (double)(hethet_ij - 2 ibs0_ij) / (double)(h_i + h_j),  NaN when h_i + h_j = 0; a
 *     duplicate pair has phi = 0.5 exactly.
 *
 *     Hardy-Weinberg exact test (Wigginton, Cutler and Abecasis 2005) of the counts (n_AA, n_AB, n_BB):  N = their sum;  N = 0 gives
 *     p = 1.  hr = min(n_AA, n_BB), r = 2 hr + n_AB (copies of the rare allele).  The heterozygote counts h are those of the parity
 *     of r in [r mod 2, r];  mid = the one nearest to r (2N - r) / (2N), the larger of two equally near ones: in integers
 *     mid = floor(r (2N - r) / (2N)), plus 1 if its parity is not r's.  With h go the homozygote counts (r - h) / 2 (rare) and
 *     N - h - (r - h) / 2 (common).  Unnormalised probabilities start from P(mid) = 1 and follow
 *         P(h - 2) = P(h) * h (h - 1) / (4 (hr + 1) (hc + 1)),        P(h + 2) = P(h) * 4 hr hc / ((h + 2) (h + 1)),
 *     hr, hc the homozygote counts that go with h.  Each step is  P' = fl(fl(P * (double)num) / (double)den):  num and den are exact
 *     int64 products converted to fp64 once, the product and the quotient are rounded separately.  The terms are visited in ONE
 *     order: mid, then the lower leg mid - 2, mid - 4, ..., then the upper leg mid + 2, mid + 4, ..., r.  First walk:
 *     total = 1.0, then total = fl(total + P) for every further term in that order; P(n_AB) is picked up on the way.  Second walk, the
 *     same steps in the same order:  tail = (1.0 <= P(n_AB) ? 1.0 : 0.0), then tail = fl(tail + P) for every term with P <= P(n_AB).
 *     p = min(1, fl(tail / total)).  Nothing is contracted into an FMA and no array is kept per marker, so a scalar restatement in
 *     any IEEE-754 language gives the same bits.
 *
 *     Files are read as eagle_marker_counts reads them (resident image, else sidecar, else text; a VIEW alias works).  Single device:
 *     a multi-device context works on its first device.  Argument errors (EAGLE_ERR_ARG: a NULL pointer, dims <= 0, and those named
 *     below) are decided before the context is used; with ctx == NULL their text is in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */

/* counts_out[3 i .. 3 i + 2] = the numbers of '0', '1' and '2' characters of line i of M.ascii (dims = (n, L) of M: n lines of L
 * characters): the genotype counts (n0, n1, n2) of individual i, by k_marker_counts on the individual-major image. */
int eagle_sample_counts(eagle_ctx* ctx, const char* f_name_ascii_M, const long dims[2], double max_memory_in_Gbytes, int32_t* counts_out);

/* The same from a SNP-major PLINK .bed file (the format and the checks of eagle_create_ascii_from_bed; dims = (n, L)), where missing
 * genotypes are still known: counts_out[4 i .. 4 i + 3] = homozygous A1 (code 00), heterozygous (10), homozygous A2 (11), missing
 * (01) of INDIVIDUAL i over all markers (k_bed_sample_counts: the column sums of what eagle_bed_marker_counts sums along the rows).
 * The rows are staged as eagle_bed_marker_counts stages them; the windows' counts are added in HBM. */
int eagle_bed_sample_counts(eagle_ctx* ctx, const char* bed_path, const long dims[2], double max_memory_in_Gbytes, int32_t* counts_out);

/* ibs0_out, hethet_out: n x n int32 each, row-major (symmetric), as defined above, over all L markers of M.ascii (dims = (n, L)).
 * A file that is not resident, does not fit, or exceeds EAGLE_HIP_MAX_RESIDENT_GB is processed in marker windows and both integer
 * accumulators are summed across the windows: the same integers either way.  A later eagle_calculateMMt on the same resident file
 * returns the bits it returned before.  EAGLE_ERR_ARG: L >= 2^31. */
int eagle_sample_ibs(eagle_ctx* ctx, const char* f_name_ascii_M, const long dims[2], double max_memory_in_Gbytes, int32_t* ibs0_out,
                     int32_t* hethet_out);

/* p_out[i] = the exact test above on counts[i * stride .. i * stride + 2] = (n_AA, n_AB, n_BB), i < L; stride = 3 (the rows of
 * eagle_marker_counts) or 4 (those of eagle_bed_marker_counts, whose fourth column is not used).  One marker per device thread
 * (k_hwe_exact).  EAGLE_ERR_ARG: L <= 0, another stride, a negative count, a marker with more than 2^30 genotypes. */
int eagle_hwe_exact(eagle_ctx* ctx, const int32_t* counts, long L, int stride, double* p_out);

/* ---------------------------------------------------------------------------------------------
 * 1b'''i. kNN imputation of missing genotypes (no counterpart in the reference, which makes every missing genotype a heterozygote):
 *     the kNNi of TASSEL over individuals.  Neighbours are ranked genome-wide, the vote on a genotype is taken among the nearest
 *     neighbours that are called at its marker, and the result is a new SNP-major .bed file without a missing code, which
 *     eagle_create_ascii_from_bed ingests like any other.  Integer arithmetic in a fixed order: a restatement in numpy gives the same
 *     bytes (r_api.knn_rows_host, r_api.impute_knn_host).
 *
 *     2-bit codes: 0 = homozygous A1, 1 = missing, 2 = heterozygous, 3 = homozygous A2; individual 4b+q at bits 2q of byte b of a
 *     marker's row of rb = ceil(n/4) bytes.  Dosage t(0) = 0, t(2) = 1, t(3) = 2.
 *
 *     Distance, on the INGESTED panel (missing = heterozygous), from eagle_sample_ibs' matrices, with h_i = hethet_ii:
 *         d_ij = 4 ibs0_ij + h_i + h_j - 2 hethet_ij        = sum_m (g_im - g_jm)^2 for g in {-1, 0, +1},
 *     in int32 arithmetic (exact while 4 L < 2^31).
 *
 *     Neighbour table nbr[n][K], int32, 1 <= K <= EAGLE_KNN_MAX_K: row i holds the K_eff = min(K, n - 1) individuals j != i with the
 *     smallest keys (uint64)(uint32)d_ij << 32 | j, in increasing key order (ties in d go to the smaller index); the entries beyond
 *     K_eff are -1.
 *
 *     Vote for a missing genotype of individual i at marker m: walk nbr[i][0 .. K) in order, passing over entries that are -1, and
 *     take the first k (1 <= k <= K) neighbours whose code at m IN THE INPUT FILE is not 1.  With c voters (c <= k) and s the sum of
 *     their dosages:  if c >= min_votes (>= 1) the dosage written is (2 s + c) / (2 c) in integer division, the mean rounded half up.
 *     Fallback otherwise: the same formula on the marker's own called genotypes, c = n0 + n1 + n2, s = n1 + 2 n2 (the counts of
 *     eagle_bed_marker_counts); a marker without any call becomes heterozygous, the ingestion's rule.
 *
 *     Votes read original codes only, so the result does not depend on the order in which genotypes are filled.  Called genotypes are
 *     copied; the unused bit pairs of a row's last byte are written as 00.
 *
 *     Single device: a multi-device context works on its first device.  Argument errors (EAGLE_ERR_ARG: a NULL pointer, dims <= 0,
 *     and those named below) are decided before the context is used; with ctx == NULL their text is in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */

#define EAGLE_KNN_MAX_K 256
/* k_knn_rows keeps a row of d in LDS, one dword per individual (128 KiB at most); the two n x n int32 matrices take 8 GiB there. */
#define EAGLE_KNN_MAX_N 32768L
/* k_bed_impute stages whole marker rows in LDS, 60 KiB per block (two blocks per CU): a row of more individuals is refused. */
#define EAGLE_IMPUTE_MAX_N 245760L

/* nbr_out: n x K int32 as defined above, from ibs0 and hethet (n x n int32, row-major: eagle_sample_ibs' outputs), one block per
 * individual (k_knn_rows).  EAGLE_ERR_ARG: n > EAGLE_KNN_MAX_N, K outside [1, EAGLE_KNN_MAX_K]. */
int eagle_knn_rows(eagle_ctx* ctx, const int32_t* ibs0, const int32_t* hethet, long n, int K, int32_t* nbr_out);

/* Writes out_bed_path: the SNP-major .bed file bed_path (the format, the checks and the error codes of eagle_create_ascii_from_bed;
 * dims = (n, L)) with every missing genotype filled as defined above from nbr (n x K int32, host memory) -- the three header bytes,
 * then the L patched rows.  counts_out (may be NULL): L x 2 int32, the genotypes of marker i imputed by vote and by fallback; their sum
 * is the marker's missing count.  The rows are staged through pinned memory in the windows of eagle_bed_marker_counts; each window
 * is counted by that call's kernel (the fallback genotypes), patched by k_bed_impute, copied back and written while the next window
 * is on the device.  The result does not depend on the window size.
 * EAGLE_ERR_ARG: n > EAGLE_IMPUTE_MAX_N, K outside [1, EAGLE_KNN_MAX_K], k outside [1, K], min_votes < 1, an nbr entry outside
 * [-1, n), out_bed_path equal to bed_path -- nothing has been written then.  A failed call leaves no output file of the full size. */
int eagle_bed_impute_knn(eagle_ctx* ctx, const char* bed_path, const long dims[2], const int32_t* nbr, int K, int k, int min_votes,
                         const char* out_bed_path, double max_memory_in_Gbytes, int32_t* counts_out);

/* ---------------------------------------------------------------------------------------------
 * 1b'''ii. Pairwise-complete IBS counts, KING kinship and kNN distances from the .bed file (no counterpart in the reference).  The
 *     ingested panel has made every missing genotype a heterozygote, so section 1b''' counts a pair's missing calls as shared or
 *     unshared heterozygotes.  Here a marker counts for a pair only where BOTH individuals are called, as in PLINK --make-king and
 *     KING: the .bed file is read itself, where the missing code is still known.
 *
 *     Codes as in 1b'''i: 0 = homozygous A1, 1 = missing, 2 = heterozygous, 3 = homozygous A2.  Per individual i and marker m:
 *         g = -1, 0, 0, +1 for the codes 0, 1, 2, 3;    u = |g|;    h = [code == 2];    c = [code != 1].
 *     An optional include[m] (one byte per marker; zero = excluded) zeroes all four at the excluded markers.  The unused bit pairs of
 *     a row's last byte belong to nobody, whatever bits they hold.
 *
 *     Four Gram products over the included markers, int32 and symmetric, each one exact product on the fp4 MFMA (k_syrk_f4*):
 *         D = g g^T,    Q = u u^T,    H = h h^T,    N = c c^T.
 *     Results, n x n int32 each, row-major:
 *         ncalled_ij = N_ij                    markers where both are called (diagonal: i's called genotypes)
 *         ibs0_ij    = (Q_ij - D_ij) / 2       both called, opposite homozygotes (diagonal 0)
 *         hethet_ij  = H_ij                    both heterozygous (diagonal h_i)
 *         hetsum_ij  = H_ij + N_ij - Q_ij      heterozygous genotypes of i where j is called plus those of j where i is called
 *                                              (N - Q counts the both-called markers with at least one heterozygote; diagonal 2 h_i)
 *
 *     Kinship is the caller's fp64 arithmetic (r_api.king_from_pair_counts):
 *         phi_ij = (double)(hethet_ij - 2 ibs0_ij) / (double)hetsum_ij,   NaN where hetsum_ij == 0;
 *     two copies of one individual have phi = 0.5 exactly, whatever their missing patterns.
 *
 *     Distance for the neighbour table:  d_ij = 4 ibs0_ij + hetsum_ij - 2 hethet_ij = the sum of (g_i - g_j)^2 over the both-called
 *     markers, normalised to the panel length:
 *         dist_ij = (uint32)((int64)d_ij * Linc / N_ij)   (integer division; Linc = the number of included markers)
 *         dist_ij = 0xFFFFFFFE                            where N_ij < min_overlap (min_overlap >= 1)
 *     The diagonal is written by the same rule and not used.  L < 2^29 keeps every term in range.
 *
 *     Single device: a multi-device context works on its first device.  Argument errors (EAGLE_ERR_ARG: a NULL pointer, dims <= 0,
 *     and those named below) are decided before the context is used; with ctx == NULL their text is in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */

/* ncalled_out, ibs0_out, hethet_out, hetsum_out: n x n int32 each; dist_out: n x n uint32 or NULL; as defined above, from the
 * SNP-major .bed file bed_path (the format, the checks and the error codes of eagle_create_ascii_from_bed; dims = (n, L)).  include:
 * L bytes or NULL (every marker).  The rows go through the pinned staging ring in the windows of eagle_bed_marker_counts (cut further
 * only where padding n to 256 rows would make one operand plane pass 128 MiB); per window k_bed_pack_fp4 writes the four
 * individual-major fp4 operand images from one read of the rows (the window's marker count padded to a multiple of 256 with zero
 * nibbles) and four SYRKs add to four int32 accumulators, so the result does not depend on the window size; k_bed_ibs_finish makes
 * the results.  EAGLE_ERR_ARG: L >= 2^29, min_overlap < 1. */
int eagle_bed_sample_ibs(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, int min_overlap,
                         double max_memory_in_Gbytes, int32_t* ncalled_out, int32_t* ibs0_out, int32_t* hethet_out, int32_t* hetsum_out,
                         uint32_t* dist_out);

/* eagle_knn_rows with the key's high dword read from dist (n x n uint32, row-major: eagle_bed_sample_ibs' dist_out): row i of nbr_out
 * holds the min(K, n - 1) individuals j != i with the smallest keys (uint64)dist_ij << 32 | j in increasing order, then -1.  A pair
 * below min_overlap (0xFFFFFFFE) comes after every other.  A dist of 0xFFFFFFFF is not a distance (the kernel's own mark): -1 is
 * written in its place at the end of the row.  EAGLE_ERR_ARG: n > EAGLE_KNN_MAX_N, K outside [1, EAGLE_KNN_MAX_K]. */
int eagle_knn_rows_dist(eagle_ctx* ctx, const uint32_t* dist, long n, int K, int32_t* nbr_out);

/* ---------------------------------------------------------------------------------------------
 * 1b'''iii. LD-kNNi: imputation from neighbours ranked in local LD (no counterpart in the reference; Money et al. 2015, the successor
 *     of the kNNi of 1b'''i).  1b'''i ranks an individual's neighbours once, genome-wide.  In a panel whose members are all about
 *     equally related genome-wide (MAGIC, NAM, diversity panels) the close relative changes from one segment to the next: here the
 *     neighbours of a missing genotype are ranked per marker, over the marker's partners in local LD.  Integer arithmetic, or fp64 in
 *     a fixed order with no FMA contraction: a restatement in numpy gives the same bytes (r_api.ld_partners_host,
 *     r_api.impute_ldknn_host).
 *
 *     LD partners.  Notation of 1b'' (s, q, d, c, v from the ingested marker-major image; missing genotypes are heterozygotes there).
 *     For markers i != j with v_i > 0 and v_j > 0, in fp64 in exactly this order (two products, one quotient, each correctly rounded):
 *         r2_ij = fl( fl((double)c * (double)c) / fl((double)v_i * (double)v_j) )
 *     Marker j is a CANDIDATE for i when 1 <= |j - i| <= window, 0 <= j < L, r2_ij >= min_r2, and chrom[j] == chrom[i] when chrom is
 *     given.  partners[i][0 .. l) holds the l_i = min(l, #candidates) candidates by decreasing r2, ties to the smaller |j - i|, then to
 *     the smaller j; then -1.  A monomorphic marker has a row of -1.  1 <= window <= 256 (the band of eagle_ld_window),
 *     1 <= l <= EAGLE_LDKNN_MAX_PARTNERS, 0 <= min_r2 <= 1.
 *
 *     Local distance.  Codes and dosages are those of 1b'''i, read from the INPUT .bed file, where the missing code is still known.  For
 *     target marker m with partner set P = partners[m] (entries -1 passed over) and individuals i != j, over the p in P where both are
 *     called:
 *         ov_ij = #{p},    d_ij = sum_p (g_ip - g_jp)^2 with g = -1, 0, +1,    dist_ij = (d_ij * 4096) / ov_ij in integer division.
 *     d <= 128 and ov <= 32: two different ratios d / ov differ by at least 1/1024, so the floor keeps their order.  j is ELIGIBLE for
 *     (i, m) when j != i, j is called at m, and ov_ij >= min_overlap (1 <= min_overlap <= 32).
 *
 *     Vote for a missing (i, m): the k eligible j with the smallest keys (uint64)dist_ij << 32 | j, 1 <= k <= EAGLE_LDKNN_MAX_K.  With c
 *     voters of dosage sum s and c >= min_votes (>= 1) the dosage written is (2 s + c) / (2 c), the rule of 1b'''i; otherwise 1b'''i's
 *     fallback: the same formula on the marker's own calls, a heterozygote when the marker has no call.
 *
 *     Votes read original codes only, so the result does not depend on the order in which genotypes are filled.  Called genotypes are
 *     copied; the unused bit pairs of a row's last byte are written as 00.
 *
 *     Single device: a multi-device context works on its first device.  Argument errors (EAGLE_ERR_ARG: a NULL pointer, dims <= 0,
 *     and those named below) are decided before the context is used; with ctx == NULL their text is in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */

#define EAGLE_LDKNN_MAX_PARTNERS 32
#define EAGLE_LDKNN_MAX_K 64
/* k_bed_impute_ldknn keeps three 32-bit words per individual (bit p = partner p) and two copies of the target row in the 160 KiB of
 * LDS of a compute unit: 12.5 bytes per individual, 150 KiB at this n, the rest left to the kernel's own arrays. */
#define EAGLE_LDKNN_MAX_N 12288L

/* partners_out: L x l int32 as defined above, row-major; r2_out (may be NULL): L x l fp64, the r2 of every partner, 0.0 beside -1.
 * f_name_ascii_Mt is read as eagle_ld_window reads it (dims = (n, L); resident image, else sidecar, else text; a VIEW alias works).
 * The dot products are those of eagle_ld_window's band, on the same tile of the int8 MFMA, kept as fp64 r2 values (k_ld_tile's r2
 * mode); k_ld_partners ranks, per marker, its forward entries and the backward entries of the `window` markers before it.  chrom: L
 * int32 (any coding) or NULL.  Row windows -- a file that is not resident, and a resident one whose band would pass 256 MiB -- overlap
 * by `window` rows on each side: the result does not depend on the window size.
 * EAGLE_ERR_ARG: L >= 2^31, window outside [1, 256], l outside [1, EAGLE_LDKNN_MAX_PARTNERS], min_r2 outside [0, 1] or NaN. */
int eagle_ld_partners(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], long window, int l, double min_r2, const int32_t* chrom,
                      double max_memory_in_Gbytes, int32_t* partners_out, double* r2_out);

/* Writes out_bed_path: the SNP-major .bed file bed_path (the format, the checks and the error codes of eagle_create_ascii_from_bed;
 * dims = (n, L)) with every missing genotype filled as defined above from partners (L x l int32, host memory: eagle_ld_partners'
 * output, or any table within the limits below).  counts_out (may be NULL): L x 2 int32, the genotypes of marker i imputed by vote and
 * by fallback.  The staging ring and the write-behind of eagle_bed_impute_knn; a staged window carries a halo of up to 256 marker rows
 * on each side, because a marker's partners can lie in the neighbouring window.  The result does not depend on the window size.
 * EAGLE_ERR_ARG: n > EAGLE_LDKNN_MAX_N, l outside [1, EAGLE_LDKNN_MAX_PARTNERS], k outside [1, EAGLE_LDKNN_MAX_K], min_votes < 1,
 * min_overlap outside [1, 32], a partners entry outside [-1, L) or more than 256 rows from its marker, out_bed_path equal to bed_path
 * -- nothing has been written then.  A failed call leaves no output file of the full size. */
int eagle_bed_impute_ldknn(eagle_ctx* ctx, const char* bed_path, const long dims[2], const int32_t* partners, int l, int k, int min_votes,
                           int min_overlap, const char* out_bed_path, double max_memory_in_Gbytes, int32_t* counts_out);

/* ---------------------------------------------------------------------------------------------
 * 1b'''iv. Pairwise-complete LD between markers from the .bed file (no counterpart in the reference).  The ingested panel has made
 *     every missing genotype a heterozygote, so 1b'' and the partner lists of 1b'''iii pull r2 towards the heterozygote: two markers in
 *     perfect LD on inbred lines (x = +-1, p = 1/2) with a share m of each marker's calls missing at random have r2 = (1 - m)^2 there.
 *     Here a pair of markers is counted over the individuals called at BOTH, as PLINK --indep-pairwise and --r2 count it: the .bed
 *     file is read itself, where the missing code is still known.
 *
 *     Codes as in 1b'''i: 0 = homozygous A1, 1 = missing, 2 = heterozygous, 3 = homozygous A2; individual 4b+q at bits 2q of byte b.
 *     The unused bit pairs of a row's last byte belong to nobody, whatever bits they hold.  Per marker m and individual a:
 *         x = -1, 0, 0, +1 for the codes 0, 1, 2, 3;    c = [code != 1];    u = |x|.
 *     An optional include (L bytes; zero = excluded) selects the PANEL: the Linc included markers in file order.  Every index below
 *     (i, j, the outputs, chrom) is a panel index, and `window` counts panel markers.  include == NULL is the whole file.
 *
 *     For panel markers i != j, six sums over the n individuals, each an exact int32 (k_bedld_tile on the int8 MFMA):
 *         N  = sum c_i c_j      D  = sum x_i x_j
 *         Si = sum x_i c_j      Sj = sum c_i x_j
 *         Qi = sum u_i c_j      Qj = sum c_i u_j
 *     then in int64:   cov = N D - Si Sj,    vi = N Qi - Si^2,    vj = N Qj - Sj^2.
 *     The pair is COMPARABLE iff N >= min_overlap, vi > 0 and vj > 0.  vi and vj belong to the PAIR: a marker that is polymorphic over
 *     everybody can be monomorphic over the individuals it shares with j.  For a comparable pair, in fp64 in exactly the order of 1b''
 *     and 1b'''iii (correctly rounded products and one quotient, no sum, so nothing contracts into an FMA):
 *         IN LD AT t  iff  (double)cov * (double)cov > t * ((double)vi * (double)vj)
 *         r2 = fl( fl(dc * dc) / fl(dvi * dvj) ),   dc = (double)cov, dvi = (double)vi, dvj = (double)vj.
 *     A pair that is not comparable is in LD with nothing, and its r2 entry is -1.0.
 *
 *     When the file holds no missing code, N = n, Si = s_i and Qi = q_i of 1b'': mask and r2 are then bit for bit those of
 *     eagle_ld_window and eagle_ld_partners on the ingested panel (with min_overlap <= n).
 *
 *     Limits: n <= 0x3fffffff (every int64 term then stays below 2^61), window in [1, 256], min_overlap >= 1, Linc >= 1, and
 *     Linc < 2^31 for the partners call.
 *
 *     Windows.  The rows go through the pinned staging ring of eagle_bed_marker_counts.  With rb = ceil(n / 4) bytes per row and
 *     ld = 16 ceil(n / 16):
 *         S    = max(1, floor(min(64 MiB, max_memory_in_Gbytes * 1e9 / 4) / rb))   file rows the staging budget holds
 *         Wmax = max(1024, floor(2^27 / ld))                                        so that one operand image stays under 128 MiB
 *                (the partners call: also at most max(1024, floor(2^28 / (8 window))) markers, the band cap of eagle_ld_partners)
 *     A window that starts at panel marker lo ends at the largest hi <= Linc with hi - lo <= Wmax whose file rows span at most S rows
 *     (file row of marker hi - 1, minus that of marker lo, plus 1) -- but it holds at least `need` markers (or the rest of the panel),
 *     need = window + 1 for eagle_bed_ld_window and 2 window + 1 for eagle_bed_ld_partners; the staging buffer grows to the widest such
 *     span when include is sparse.  The window is staged as that span of file rows, and k_bed_ld_pack writes three marker-major int8
 *     operand images X, C, U of its panel markers alone.  The next window starts at hi - window (eagle_bed_ld_window: it writes the
 *     mask rows of the last `window` markers again, now with all their partners) or at hi - 2 window (eagle_bed_ld_partners: partner
 *     rows are written for the markers that have `window` held markers, or the panel's end, on both sides); the last window is the one
 *     with hi = Linc.  Consecutive windows thus overlap as those of eagle_ld_window and eagle_ld_partners do, and the result does
 *     not depend on the window size.
 *
 *     Single device: a multi-device context works on its first device.  Argument errors (EAGLE_ERR_ARG: a NULL pointer, dims <= 0,
 *     and those named below) are decided before the context is used; with ctx == NULL their text is in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */

/* mask_out (Linc x W uint64, W = ceil(window / 64)) and *npairs_out as those of eagle_ld_window, by panel marker, under the rule
 * above, from the SNP-major .bed file bed_path (the format, the checks and the error codes of eagle_create_ascii_from_bed;
 * dims = (n, L)).  include: L bytes or NULL (may be NULL; every other pointer may not).
 * EAGLE_ERR_ARG: n > 0x3fffffff, window outside [1, 256], r2 outside [0, 1] or NaN, min_overlap < 1, an include that selects no marker. */
int eagle_bed_ld_window(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, long window, double r2,
                        int min_overlap, double max_memory_in_Gbytes, uint64_t* mask_out, long* npairs_out);

/* partners_out (Linc x l int32) and r2_out (Linc x l fp64, may be NULL) as those of eagle_ld_partners, by panel marker: the candidates of
 * i are the panel markers j, 1 <= |j - i| <= window, whose pair with i is comparable with r2 >= min_r2, on i's chromosome when chrom
 * (Linc int32, by panel marker; may be NULL) is given; ranked by k_ld_partners under the rule of 1b'''iii on the fp64 band of
 * k_bedld_tile's r2 mode.
 * EAGLE_ERR_ARG: n > 0x3fffffff, window outside [1, 256], l outside [1, EAGLE_LDKNN_MAX_PARTNERS], min_r2 outside [0, 1] or NaN,
 * min_overlap < 1, an include that selects no marker, Linc >= 2^31. */
int eagle_bed_ld_partners(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, long window, int l, double min_r2,
                          int min_overlap, const int32_t* chrom, double max_memory_in_Gbytes, int32_t* partners_out, double* r2_out);

/* ---------------------------------------------------------------------------------------------
 * 1b'''v. LD scores and the LD decay curve (no counterpart in the reference): the sums of the r2 band that 1b'''iii ranks, per marker
 *     and per distance bin, as exact integers.  What LDPrune(window, r2, kb), ImputeBed(local, window) and tag_markers(r2) ask the user
 *     to choose is read off these two statistics.
 *
 *     1. r2.  r2_ij is the fp64 number of 1b'''iii (the ingested panel: eagle_ld_stats) or of 1b'''iv (the .bed file with include and
 *        min_overlap: eagle_bed_ld_stats), unchanged; -1.0 where there is no pair (a monomorphic marker; a pair that is not comparable).
 *        0 <= r2_ij <= 1 holds in fp64: c^2 <= v_i v_j in integers (Cauchy-Schwarz on the centred rows), the conversions to fp64 are
 *        exact while n^2 <= 2^53 (|c| and v are at most n^2), rounding is monotone -- a <= b gives fl(a) <= fl(b), so fl(c c) <=
 *        fl(v_i v_j) and the quotient of x <= y rounds to at most 1 -- and equal products round equally, so two identical markers
 *        have r2 = 1.0 exactly.
 *     2. Quantised r2.  u_ij = (uint64)(r2_ij * 1073741824.0), 2^30: the multiplication by a power of two is exact and the conversion
 *        truncates, 0 <= u_ij <= 2^30.  Integer sums of u do not depend on the order of summation: the device, whatever its
 *        reduction tree and the order of its atomic adds, and numpy (r_api.ld_stats_host) agree bit for bit.
 *     3. Eligible pair (i, j):  1 <= |j - i| <= window <= 256;  r2_ij >= 0;  chrom[i] == chrom[j] when chrom (int32 per panel marker,
 *        any coding) is given;  |pos[j] - pos[i]| <= max_dist when pos (int64 per panel marker, base pairs, need not be sorted) is given
 *        and max_dist > 0.  The distance d_ij is |pos[j] - pos[i]| with pos and |j - i| without.
 *     4. Per marker.  U_i = sum of u_ij over the eligible j (uint64) and cnt_i = their number (int32), over both sides.  The LD score is
 *        1.0 + (double)U_i * 2^-30, the caller's arithmetic: the leading 1 is the marker with itself.  A monomorphic or isolated
 *        marker has U = 0, cnt = 0 and score 1.0.
 *     5. Decay.  Bin edges edges[0] < edges[1] < ... < edges[B], int64, 1 <= B <= 512.  Every eligible pair with i < j is counted
 *        once, in bin b iff edges[b] <= d_ij < edges[b + 1]; a pair outside [edges[0], edges[B]) is in no bin but still counts in the
 *        scores.  pairs[b] (int64) is the number of pairs of the bin and sum[b] (uint64) the sum of their u_ij; the mean r2 of a bin,
 *        (double)sum / (double)pairs * 2^-30, is the caller's arithmetic.
 *     6. Limit.  markers * window <= 2^33 (markers = L, or Linc for the .bed file), so that no bin sum can pass 2^63: at most
 *        markers * window pairs of at most 2^30 each.
 *
 *     k_ld_reduce works in the place of k_ld_partners, on the same band, in the same cores of markers with a halo of `window` rows on
 *     both sides (resident, sidecar or text source, a VIEW alias; the .bed file's windows of 1b'''iv): a pair is binned with its smaller
 *     marker and every marker belongs to one core, so the result does not depend on the window size.
 *
 *     Single device: a multi-device context works on its first device.  Argument errors (EAGLE_ERR_ARG: a NULL pointer, dims <= 0,
 *     and those named below) are decided before the context is used; with ctx == NULL their text is in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */

/* U_out (L uint64) and cnt_out (L int32) of definition 4; bin_sum_out (nbins uint64) and bin_pairs_out (nbins int64) of definition 5,
 * B = nbins.  chrom (L int32), pos (L int64) and edges (nbins + 1 int64) may be NULL; edges == NULL or nbins == 0 means no decay, and
 * the two bin outputs may then be NULL.  f_name_ascii_Mt is read as eagle_ld_partners reads it (dims = (n, L)).
 * EAGLE_ERR_ARG: window outside [1, 256], L >= 2^31, L * window > 2^33, max_dist > 0 without pos, nbins outside [0, 512], edges not
 * strictly increasing, edges given without the bin outputs. */
int eagle_ld_stats(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], long window, const int32_t* chrom, const int64_t* pos,
                   long max_dist, const int64_t* edges, long nbins, double max_memory_in_Gbytes, uint64_t* U_out, int32_t* cnt_out,
                   uint64_t* bin_sum_out, int64_t* bin_pairs_out);

/* The same four outputs by PANEL marker (Linc entries; chrom and pos by panel marker too) from the SNP-major .bed file bed_path, r2 under
 * the rule of 1b'''iv (include: L bytes or NULL; min_overlap), in the windows of eagle_bed_ld_partners.
 * EAGLE_ERR_ARG: those of eagle_ld_stats with Linc in the place of L, and n > 0x3fffffff, min_overlap < 1, an include that selects no
 * marker. */
int eagle_bed_ld_stats(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, long window, int min_overlap,
                       const int32_t* chrom, const int64_t* pos, long max_dist, const int64_t* edges, long nbins, double max_memory_in_Gbytes,
                       uint64_t* U_out, int32_t* cnt_out, uint64_t* bin_sum_out, int64_t* bin_pairs_out);

/* ---------------------------------------------------------------------------------------------
 * 1b'''vi. Runs of homozygosity (no counterpart in the reference): where the autozygous segments of every individual lie, the numbers
 *     F_ROH and the per-marker ROH incidence are made of.  The rule follows PLINK --homozyg AS DOCUMENTED -- a window scan, a per-SNP
 *     threshold, then segment filters.  Agreement with the PLINK program itself is neither claimed nor tested.  Everything is integers,
 *     so the device and numpy (r_api.roh_host) agree with ==.
 *
 *     1. Class of individual i at panel marker m.  hom: image value +-1, .bed codes 00 and 11.  het: image value 0, .bed code 10.
 *        miss: .bed code 01 only -- on the ingested image a missing call of the original data is a het, as for the counts of 1b'.
 *     2. Blocks.  A block [a, e) is a maximal run of panel markers with equal chrom[m] (int32 by panel marker; NULL: one block).  pos is
 *        int64 by panel marker (NULL: pos[m] = m) and must be non-decreasing inside every block, else EAGLE_ERR_ARG.
 *     3. Window.  1 <= w <= 64.  The window that starts at s is VALID iff a <= s and s + w <= e for the block of s, and HOMOZYGOUS iff
 *        its het count is <= win_het and its miss count is <= win_miss.
 *     4. Marker flag.  cover = the number of valid windows that contain m, hom = the number of those that are homozygous; m is FLAGGED
 *        iff hom >= 1 and hom * 65536 >= thr16 * cover, 0 <= thr16 <= 65536.  A block shorter than w has no flagged marker.
 *     5. Run.  A maximal sequence s .. e of consecutive flagged markers of one block; with max_gap > 0 it is also broken between m and
 *        m + 1 where pos[m + 1] - pos[m] > max_gap.
 *     6. Reported segment.  A run with  nsnp = e - s + 1 >= min_snp,  len = pos[e] - pos[s] >= min_len,  max_density == 0 or
 *        len <= max_density * nsnp (max_density <= 2^31: the product stays in int64),  max_het < 0 or nhet <= max_het.  nhet and nmiss
 *        are the individual's het and miss markers in s .. e.
 *     7. Outputs.  ind_out: n x 4 int64 = (number of segments, sum of nsnp, sum of len, longest len) per individual.  seg_out: rows of
 *        six int32 (individual, s, e, nhet, nmiss, block ordinal), sorted by (individual, s); s and e are panel marker indices.
 *        *nseg_out is always the total.  seg_out has room for seg_cap rows (it may be NULL when seg_cap is 0); it is written iff the
 *        total is <= seg_cap and untouched otherwise.  The call returns EAGLE_OK either way.
 *     8. Limits.  Panel markers < 2^31; n <= 0x3fffffff for the .bed file.  The three bit planes below (3 x markers x ceil(n / 64) x 8
 *        bytes) stay on the device for the whole call: where they do not fit the memory budget (EAGLE_HIP_MAX_RESIDENT_GB when it is set,
 *        else the free HBM less 1 GiB) the call returns EAGLE_ERR_NOMEM, decided before any kernel runs.
 *
 *     k_roh_flags walks chunks of EAGLE_ROH_CHUNK markers with a halo of w - 1 rows on either side, one lane per four individuals,
 *     three 64-bit shift registers per individual, every row of a chunk read once, and writes three marker-major bit planes (flagged,
 *     het, miss).  k_roh_segments walks the planes, one lane per individual and one wave per 64 individuals x block: a count pass, an
 *     exclusive scan of the counts by (individual, block) on the host, and a fill pass that is skipped when the total exceeds seg_cap.
 *     The ingested panel is read as eagle_marker_counts reads it (the resident image, else row windows of the streamed size from the
 *     sidecar, the text or a VIEW alias's source; a VIEW alias gives the kept individuals), the .bed file through the pinned ring as
 *     eagle_bed_marker_counts reads it, with the panel selection of 1b'''iv.  Windows are cores of markers held with w - 1 markers of
 *     overlap on both sides: every plane word is written once and the result does not depend on the window size.
 *
 *     Single device: a multi-device context works on its first device.  Argument errors (EAGLE_ERR_ARG: a NULL pointer, dims <= 0,
 *     and those named below) are decided before the context is used; with ctx == NULL their text is in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */
#define EAGLE_ROH_CHUNK 1024L
#define EAGLE_ROH_MAX_WINDOW 64L

typedef struct eagle_roh_params {
    int64_t w, win_het, win_miss, thr16, min_snp, min_len, max_gap, max_density, max_het;
} eagle_roh_params;

/* Rules 1 to 7 on the ingested panel Mt.ascii (dims = (n, L) of M); chrom (L int32) and pos (L int64) may be NULL.
 * EAGLE_ERR_ARG: w outside [1, 64], win_het / win_miss / min_len / max_gap < 0, thr16 outside [0, 65536], min_snp < 1, max_density
 * outside [0, 2^31], L >= 2^31, seg_cap < 0, seg_out NULL with seg_cap > 0, pos decreasing inside a block. */
int eagle_roh(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const int32_t* chrom, const int64_t* pos,
              const eagle_roh_params* params, double max_memory_in_Gbytes, int64_t* ind_out, int32_t* seg_out, long seg_cap, long* nseg_out);

/* The same by PANEL marker (the Linc markers include selects, L bytes or NULL; chrom and pos by panel marker) from the SNP-major .bed
 * file bed_path (dims = (n, L) of the file), which still knows its missing calls.
 * EAGLE_ERR_ARG: those of eagle_roh with Linc in the place of L, and n > 0x3fffffff, an include that selects no marker. */
int eagle_bed_roh(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, const int32_t* chrom, const int64_t* pos,
                  const eagle_roh_params* params, double max_memory_in_Gbytes, int64_t* ind_out, int32_t* seg_out, long seg_cap, long* nseg_out);

/* ---------------------------------------------------------------------------------------------
 * 1b'''vii. Pairwise IBD-type segments (no counterpart in the reference): where two individuals share their genome.  On unphased
 *     genotypes a pair can share one haplotype only where it has no opposite homozygotes, and both only where its genotypes are equal
 *     -- the observation IBIS and TRUFFLE build on.  The runs below are IBS runs: they bound IBD from above.  Agreement with the IBIS or
 *     TRUFFLE programs is neither claimed nor tested.  Everything is integers, so the device and numpy (r_api.ibd_host) agree with ==.
 *
 *     1. Genotype and called.  Image value -1 / 0 / +1 is hom A1 / het / hom A2, always called: a missing call of the original data is
 *        a het by now.  .bed codes 00 / 10 / 11 are hom A1 / het / hom A2; code 01 is not called.
 *     2. Break marker of the pair (i, j).  Both are called at m, and  mode = 1 ("ibs1"): g_i * g_j = -1, opposite homozygotes;
 *        mode = 2 ("ibs2"): g_i != g_j.  A marker where either is not called is never a break.
 *     3. Blocks and pieces.  Blocks are those of ROH rule 2 (chrom, int32 by panel marker; NULL: one block).  pos is int64 by panel
 *        marker (NULL: pos[m] = m) and must be non-decreasing inside every block, else EAGLE_ERR_ARG.  With max_gap > 0 a block is cut
 *        further between m and m + 1 where pos[m + 1] - pos[m] > max_gap.  The results are PIECES.
 *     4. Pure run.  A maximal sequence of consecutive non-break markers inside one piece.
 *     5. Merging.  With merge_min = 0 every pure run is a candidate on its own.  With merge_min >= 1 a pure run is ELIGIBLE iff it has
 *        at least merge_min markers, and a candidate is a maximal chain R_1 .. R_k of pure runs of one piece in which, whenever k >= 2,
 *        every run is eligible and consecutive runs are separated by exactly one marker (a single break).  An ineligible run is a
 *        chain of its own; two breaks in a row, or a cut, end a chain.  The condition is on each pure run alone, so the chains do not
 *        depend on the walking order.
 *     6. Reported segment.  A candidate s .. e (the break markers inside included) with  nsnp = e - s + 1 >= min_snp  and
 *        len = pos[e] - pos[s] >= min_len.  nbreak = k - 1.
 *     7. Pairs.  pairs is P x 2 int32 with 0 <= i < j < n, duplicates allowed; NULL: all pairs in row-major upper-triangle order,
 *        k = i n - i (i + 1) / 2 + (j - i - 1), and npairs is ignored.  P <= EAGLE_IBD_MAX_PAIRS = 2^27.
 *     8. Outputs.  pair_out: P x 4 int64 = (number of segments, sum of nsnp, sum of len, longest len) by pair ordinal.  seg_out: rows of
 *        six int32 (i, j, s, e, nbreak, block ordinal), sorted by (pair ordinal, s); s and e are panel marker indices.  *nseg_out is
 *        always the total.  seg_out has room for seg_cap rows (it may be NULL when seg_cap is 0); it is written iff the total is
 *        <= seg_cap and untouched otherwise.  The call returns EAGLE_OK either way (eagle_roh's semantics, rule 7 there).
 *     9. Limits.  Panel markers < 2^31; n <= 0x3fffffff for the .bed file.  The bit planes below (2, from the .bed file 3, x
 *        ceil(markers / 64) x n rounded up to 64 x 8 bytes) and the per-pair arrays (40 bytes a pair) stay on the device for the whole
 *        call: where they do not fit the memory budget (ROH rule 8) the call returns EAGLE_ERR_NOMEM, decided before any kernel runs.
 *
 *     The planes are individual-major words, one uint64 per individual per 64 markers, stored word-major so that 64 individuals' words
 *     of one index are consecutive.  Bits past the last marker and words of padding individuals are zero.  eagle_ibd reads M.ascii as
 *     eagle_sample_counts reads it (the resident image, else bands of whole lines of the streamed size from the sidecar, the text or a
 *     VIEW alias's source; a VIEW alias gives the kept individuals): a band writes the words of its own individuals.  eagle_bed_ibd
 *     reads the .bed rows through the pinned ring in windows of panel markers that end on multiples of 64: a window writes whole words.
 *     Either way every plane word is written once and the result does not depend on the window size.  k_ibd_walk has one lane per
 *     pair -- a wave takes one i and 64 consecutive j, or 64 list entries -- and walks the words in order; events are taken by
 *     find-first-set over the bits of break | cut, the cut plane (a bit where a piece starts) being shared by all pairs.  A count pass, an
 *     exclusive scan of the per-pair counts on the host, and a fill pass that is skipped when the total exceeds seg_cap; no array of
 *     pairs x markers exists.
 *
 *     Single device: a multi-device context works on its first device.  Argument errors (EAGLE_ERR_ARG: a NULL pointer, dims <= 0,
 *     and those named below) are decided before the context is used; with ctx == NULL their text is in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */
#define EAGLE_IBD_MAX_PAIRS 134217728L

typedef struct eagle_ibd_params { int64_t mode, min_snp, min_len, max_gap, merge_min; } eagle_ibd_params;

/* Rules 1 to 8 on the ingested panel M.ascii (dims = (n, L) of M); pairs (npairs x 2 int32), chrom (L int32) and pos (L int64) may be
 * NULL.  EAGLE_ERR_ARG: mode not 1 or 2, min_snp < 1, min_len / max_gap / merge_min < 0, L >= 2^31, npairs outside [1, 2^27] (a list) or
 * n < 2 or n (n - 1) / 2 > 2^27 (all pairs), a pair outside 0 <= i < j < n, seg_cap < 0, seg_out NULL with seg_cap > 0, pos decreasing
 * inside a block. */
int eagle_ibd(eagle_ctx* ctx, const char* f_name_ascii_M, const long dims[2], const int32_t* pairs, long npairs, const int32_t* chrom,
              const int64_t* pos, const eagle_ibd_params* params, double max_memory_in_Gbytes, int64_t* pair_out, int32_t* seg_out, long seg_cap,
              long* nseg_out);

/* The same by PANEL marker (the Linc markers include selects, L bytes or NULL; chrom and pos by panel marker) from the SNP-major .bed
 * file bed_path (dims = (n, L) of the file), which still knows its missing calls.
 * EAGLE_ERR_ARG: those of eagle_ibd with Linc in the place of L, and n > 0x3fffffff, an include that selects no marker. */
int eagle_bed_ibd(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, const int32_t* pairs, long npairs,
                  const int32_t* chrom, const int64_t* pos, const eagle_ibd_params* params, double max_memory_in_Gbytes, int64_t* pair_out,
                  int32_t* seg_out, long seg_cap, long* nseg_out);

/* ---------------------------------------------------------------------------------------------
 * 1b'''viii. Mendel errors and parentage assignment (no counterpart in the reference): is the recorded pedigree right, and if not, who
 *     are the parents?  The checks PLINK runs as --mendel / --me and the opposing-homozygote parentage assignment of SNP-chip panels, on
 *     the bit planes of 1b'''vii.  Agreement with the PLINK program is neither claimed nor tested.  Sex chromosomes are not handled:
 *     every marker is autosomal.  Setting erroneous genotypes to missing is out of scope.  Everything is integers, so the device and
 *     numpy (r_api.mendel_host, r_api.parentage_host) agree with ==.
 *
 *     1. Genotype and called.  As rule 1 of 1b'''vii: image value -1 / 0 / +1 is hom A1 / het / hom A2, always called (a missing call
 *        of the original data is a het by now); .bed codes 00 / 10 / 11 are hom A1 / het / hom A2 and code 01 is not called.
 *     2. Trio.  (c, f, m) = child, father, mother as individual indices.  A parent index -1 is an unknown parent and behaves as an
 *        individual that is called nowhere; a trio with both parents -1 is legal and has no errors.  0 <= c < n, -1 <= f, m < n,
 *        c != f, c != m, and f != m unless both are -1 (selfing exists in rule 6 alone); else EAGLE_ERR_ARG.  Trios may repeat, and an
 *        individual may be a child in one trio and a parent in another.
 *     3. Mendel error at marker x.  The child is called, and no choice of one allele from each parent gives the child's genotype; a
 *        not-called or unknown parent can pass either allele.  Of the 64 code triples (hom A1, het, hom A2, not called)^3 exactly 16
 *        are errors.  On the planes A (hom A1), B (hom A2), C (called), with H_c = C_c & ~A_c & ~B_c:
 *            X = A_c B_f | B_c A_f      U = A_c | H_c B_f      V = B_c | H_c A_f      E = X | U B_m | V A_m
 *        which equals the definition on all 64 triples (tests/test_mendel_host.py enumerates them).  A and B imply called, so C is
 *        needed for H_c and the overlap counts alone.  On the image C is implicit: every bit of a panel marker; the bits of the last
 *        word past the last marker are masked, so they never become hets.
 *     4. Per-trio output.  trio_out: ntrios x 6 int32 = (n_cf, e_cf, n_cm, e_cm, n_trio, e).  n_cf = markers where c and f are both
 *        called, e_cf = opposite homozygotes of c and f; the same for m; n_trio = markers where all three are called; e =
 *        popcount(E) over the panel.  An unknown parent is called nowhere: on the image n_* = L for known parents and 0 otherwise.
 *     5. Per-marker output.  marker_out (may be NULL): int32 by panel marker, the number of trios OF THE LIST with an error there
 *        (PLINK's .lmendel; a trio listed twice counts twice).  Integer sums: any order gives the same result.
 *     6. Assignment.  offspring (n_o), sires (n_s) and dams (n_d) are lists of individual indices in [0, n); a duplicate inside a list
 *        is EAGLE_ERR_ARG (an individual may be in several lists).  An empty dam list (n_d = 0, dams may be NULL) means one unknown dam:
 *        single-parent assignment; likewise an empty sire list; both empty is EAGLE_ERR_ARG.  For the offspring c the admissible
 *        candidates are the (s, d) with s != c, d != c, overlap >= min_overlap, and s != d unless allow_self.  overlap = n_trio of
 *        (c, s, d); for single-parent assignment it is n_cf of the child and the one known parent (the unknown parent would make n_trio
 *        0).  Candidates are ranked by the key (e, ordinal), ordinal = s_idx * max(n_d, 1) + d_idx with s_idx, d_idx the positions in
 *        the lists; the smaller key wins, so ties in e go to the earlier candidate.  THE RANK IS BY ERROR COUNT, NOT BY ERROR RATE: a
 *        candidate with few called markers is not penalised beyond min_overlap.  best_out: n_o x 2 x 4 int32, per offspring the best
 *        and the runner-up as (sire, dam, e, overlap) with sire and dam as individual indices (-1 for the unknown parent); all four
 *        are -1 where there is no such candidate.
 *     7. Limits.  ntrios and n_o in [1, EAGLE_MENDEL_MAX_TRIOS = 2^27]; max(n_s, 1) * max(n_d, 1) < 2^31; 0 <= min_overlap < 2^31;
 *        allow_self 0 or 1; panel markers < 2^31; n <= 0x3fffffff for the .bed file.  The planes (1b'''vii: 2, from the .bed file 3)
 *        stay on the device for the call, with the per-trio and per-marker arrays or the gathered planes of the three lists and the
 *        partial minima of a chunk of offspring (under 256 MiB): where they do not fit the memory budget (rule 9 of 1b'''vii) the call
 *        returns EAGLE_ERR_NOMEM, decided before any kernel runs.
 *
 *     The planes are built as for eagle_ibd / eagle_bed_ibd (one helper serves all six entry points): the resident image, a streamed
 *     panel, a VIEW alias, or the .bed windows that end on multiples of 64.  k_mendel_trios has one lane per trio; the per-marker
 *     totals of a wave's 64 error words come from one ballot and one popcount per bit and reach the marker array through 32-bit
 *     integer atomics.  k_plane_gather packs the words of each list word-major; k_parentage gives a wave one offspring, 64
 *     consecutive dams and four sires a lane, keeps the two smallest keys (e << 32 | ordinal) with their overlaps per lane and
 *     reduces them over the wave and the workgroup; k_parentage_finish merges the workgroups' partials.  No atomics on that path.
 *
 *     Single device: a multi-device context works on its first device.  Argument errors (EAGLE_ERR_ARG: a NULL pointer, dims <= 0,
 *     and those named above) are decided before the context is used; with ctx == NULL their text is in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */
#define EAGLE_MENDEL_MAX_TRIOS 134217728L

/* Rules 1 to 5 on the ingested panel M.ascii (dims = (n, L) of M): trios is ntrios x 3 int32, trio_out ntrios x 6 int32, marker_out L
 * int32 or NULL. */
int eagle_mendel(eagle_ctx* ctx, const char* f_name_ascii_M, const long dims[2], const int32_t* trios, long ntrios,
                 double max_memory_in_Gbytes, int32_t* trio_out, int32_t* marker_out);

/* The same by PANEL marker (the Linc markers include selects, L bytes or NULL) from the SNP-major .bed file bed_path (dims = (n, L) of the
 * file), which still knows its missing calls.  EAGLE_ERR_ARG also for n > 0x3fffffff and an include that selects no marker. */
int eagle_bed_mendel(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, const int32_t* trios, long ntrios,
                     double max_memory_in_Gbytes, int32_t* trio_out, int32_t* marker_out);

/* Rule 6 on the ingested panel M.ascii: every overlap is L there.  best_out: n_o x 8 int32. */
int eagle_parentage(eagle_ctx* ctx, const char* f_name_ascii_M, const long dims[2], const int32_t* offspring, long n_o, const int32_t* sires,
                    long n_s, const int32_t* dams, long n_d, long min_overlap, int allow_self, double max_memory_in_Gbytes, int32_t* best_out);

/* Rule 6 by panel marker from the .bed file, as eagle_bed_mendel reads it. */
int eagle_bed_parentage(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, const int32_t* offspring, long n_o,
                        const int32_t* sires, long n_s, const int32_t* dams, long n_d, long min_overlap, int allow_self,
                        double max_memory_in_Gbytes, int32_t* best_out);

/* ---------------------------------------------------------------------------------------------
 * 1b''''. Genomic relationship matrix (no counterpart that the reference calls: its VanRaden G, E/R/GenomicRel.R, is unused): the one
 *     Gram product the matrices of EIGENSTRAT / PLINK / GCTA and their principal components need, with a weight per marker.  With
 *     g in {-1, 0, +1} = AA, AB, BB as everywhere in this library and integer weights q_m < 2^21,
 *         Q_ij = sum_m q_m g_im g_jm                       (int64, exact, |Q_ij| < 2^52, symmetric).
 *     q_m = d0 + 128 d1 + 128^2 d2 with digits d in [0, 127]; each digit plane is one exact int8 x int8 product on the int8 MFMA,
 *     C^(p)_ij = sum_m g_im (d^(p)_m g_jm): the second operand is written per marker window and plane into a buffer of the context
 *     (k_scale_cols_i8, at most about 1 GiB; never an n x L temporary), the product is k_syrk_i8's tile engine with two operand images
 *     (k_gram_i8ab, upper-triangular tile pairs only: the result is symmetric), and Q = C^(0) + 128 C^(1) + 128^2 C^(2) in int64
 *     (k_wgram_finish).  A plane whose digits are all zero costs nothing: weights in {0, 1} (the Gram product of a marker subset) are
 *     one product, q = 0 everywhere is none.  The cached int8 and fp4 images of a resident file are only read: a later
 *     eagle_calculateMMt on the same file returns the bits it returned before.
 *
 *     What a relationship matrix is made of from Q is the caller's fp64 arithmetic (r_api.grm_weights, r_api.grm_from_gram).
 *     Centring needs no second pass over the genotypes: with mu_m the mean of g_.m over a set R of individuals,
 *         sum_m q_m (g_im - mu_m)(g_jm - mu_m) = Q_ij - r_i - r_j + kappa,   r_i = (1/|R|) sum_{j in R} Q_ij,   kappa = (1/|R|) sum_{i in R} r_i,
 *     because sum_m q_m mu_m g_im = r_i: centring every marker at its mean over R is double-centring Q over R.
 *
 *     The file is read as eagle_sample_ibs reads it (resident image when it fits, else marker windows from the sidecar or the text;
 *     a VIEW alias works) and streamed and resident runs give the same integers.  Single device: a multi-device context works on its
 *     first device.  Argument errors (EAGLE_ERR_ARG: a NULL pointer, dims <= 0, and those named below) are decided before the context
 *     is used; with ctx == NULL their text is in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */

/* The int32 accumulator of a digit plane holds |sum| <= 127 L.  The accumulators are NOT folded into the int64 result between
 * windows: a panel with more markers than this, floor((2^31 - 1) / 127), is refused, so that nothing can wrap. */
#define EAGLE_WGRAM_MAX_MARKERS 16909320L

/* Q_out: n x n int64, row-major, as defined above, over all L markers of M.ascii (dims = (n, L)); q[m] < 2^21 for every marker m.
 * EAGLE_ERR_ARG: L >= 2^31, L > EAGLE_WGRAM_MAX_MARKERS, a q[m] >= 2^21. */
int eagle_weighted_gram(eagle_ctx* ctx, const char* f_name_ascii_M, const long dims[2], const uint32_t* q, double max_memory_in_Gbytes,
                        int64_t* Q_out);

/* ---------------------------------------------------------------------------------------------
 * 1b''''i. Line scores (no counterpart in the reference, which stops at the fitted model): the two products that use a model on a panel,
 *     as one exact integer pass over either genotype file.  For a file of R lines of C characters and T columns of integer weights,
 *         out[r * T + t] = sum_c w[t * C + c] * g[r][c]          (int64, exact, |out| <= 2^30 * C < 2^61).
 *     On M.ascii a line is an individual and the weights are per marker: the result is M w, a polygenic or genomic score per
 *     individual (eagle_sample_scores).  On Mt.ascii a line is a marker and the weights are per individual: the result is M^T V, one
 *     number per marker from one number per individual, for T vectors at once (eagle_marker_scores) -- marker BLUPs, PCA loadings.
 *
 *     1. Genotypes and weights.  g in {-1, 0, +1} = AA, AB, BB as everywhere in this library; a missing genotype of the source is a
 *        heterozygote by now.  Weights are int32 with |w| <= 2^30 = EAGLE_SCORES_MAX_WEIGHT; 1 <= T <= 64 = EAGLE_SCORES_MAX_COLUMNS.
 *     2. Digits.  w = d0 + 256 d1 + 256^2 d2 + 256^3 d3 with balanced digits d in [-128, 127]:  d_p = ((w_p + 128) & 255) - 128 and
 *        w_{p+1} = (w_p - d_p) >> 8, from w_0 = w.  Four digits hold every |w| <= 2^30.  Each digit plane of each column is one int8
 *        operand row, d * g is an int8 x int8 product accumulated in int32, and out = sum_p 256^p C^(p) in int64.  A plane whose
 *        digits are all zero over the call costs nothing: weights with |w| <= 127 are one plane, w = 0 everywhere is no product.
 *     3. Line length.  C <= EAGLE_SCORES_MAX_LINE = 8,388,480, the largest multiple of 128 below 2^23 (the addressing contract of the
 *        tile engine, ld * 256 < 2^31).  A plane's int32 accumulator holds at most 128 C < 2^31: nothing wraps and no fold is needed.
 *     4. Order.  Integer sums do not depend on the order of summation: the device, whatever its K splits and the order of its atomic
 *        adds, and numpy's int64 product (r_api.line_scores_host) agree bit for bit.
 *
 *     k_score_digits writes the digit image (at most 256 live rows of the line's padded length; T <= 64 is 256 rows at four planes),
 *     k_line_scores_i8 is the stage loop of k_syrk_i8's tile engine over a rectangular work list (row tile, 0) x K splits -- one pass
 *     over the image per call, no temporary of image size -- and k_scores_finish sums the planes.  The cached int8 and fp4 images of a
 *     resident file are only read: a later eagle_calculateMMt on the same file returns the bits it returned before.
 *
 *     The file is read as eagle_marker_counts reads it: the resident image where it lies, otherwise bands of whole lines from the
 *     sidecar, the text or a VIEW alias's source.  Rows are independent, so bands need no accumulation across windows, and streamed and
 *     resident runs give the same integers.  With a VIEW alias of eagle_reshape_m the M file has the kept individuals as lines and the
 *     Mt file has them as columns (v then has dims[0] = kept entries per column).  Single device: a multi-device context works on
 *     its first device.  Argument errors (EAGLE_ERR_ARG: a NULL pointer, dims <= 0, T outside [1, 64], a line longer than
 *     EAGLE_SCORES_MAX_LINE, more than 2^31 - 1 lines, a weight beyond +-2^30) are decided before the context is used; with ctx == NULL
 *     their text is in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */
#define EAGLE_SCORES_MAX_COLUMNS 64L
#define EAGLE_SCORES_MAX_WEIGHT 1073741824L
#define EAGLE_SCORES_MAX_LINE 8388480L

/* out: n x T int64, row-major: the scores of the n lines of M.ascii (dims = (n, L)) under the T x L weights w (row-major, one row per
 * column of the result). */
int eagle_sample_scores(eagle_ctx* ctx, const char* f_name_ascii_M, const long dims[2], const int32_t* w, long T, double max_memory_in_Gbytes,
                        int64_t* out);
/* out: L x T int64, row-major: M^T V for the L lines of Mt.ascii (dims = (n, L) of M) and the T x n weights v (row-major). */
int eagle_marker_scores(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const int32_t* v, long T, double max_memory_in_Gbytes,
                        int64_t* out);

/* ---------------------------------------------------------------------------------------------
 * 1b''''ii. Epistasis (no counterpart in the reference, whose model is additive): the exact pairwise marker-interaction scan.  For two
 *     markers i, j and an integer trait y the model is
 *         y = b0 + b1 g_i + b2 g_j + b3 g_i g_j + e,
 *     the additive x additive test of PLINK --epistasis for a quantitative trait (GLIDE and epiGPU ran this regression on GPUs), and the
 *     statistic is the F(1, n - 4) of b3 = 0.  Every sufficient statistic is an exact integer, so the device (k_epi_tile, eagle_epi.hip)
 *     and the numpy restatement (r_api.epistasis_host) agree bit for bit.
 *
 *     1. Inputs.  Genotypes g in {-1, 0, +1} = AA, AB, BB over the n individuals of Mt.ascii (a VIEW alias of eagle_reshape_m: its kept
 *        individuals); a missing call of the source is a heterozygote by now, as everywhere on the image.  The trait is int32 with
 *        |y_k| <= EAGLE_EPI_YMAX = 1000000, and n <= EAGLE_EPI_MAX_N = 65535.  (r_api.quantise_trait maps a real trait onto this grid; F
 *        does not change under a shift or a scale of y.)
 *     2. Sums, all exact integers.  Per trait: Y = sum y, T = sum y^2.  Per marker: s = sum g, q = sum g^2, u = sum y g.  Per pair:
 *        d = sum g_i g_j, e = sum g_i^2 g_j, f = sum g_i g_j^2, h = sum g_i^2 g_j^2, z = sum y g_i g_j.  On the device y = d0 + 128 d1 +
 *        128^2 d2 with balanced digits in [-64, 63] (d_p = ((y_p + 64) & 127) - 64, y_{p+1} = (y_p - d_p) >> 7), so that digit * g
 *        stays int8, and z = z0 + 128 z1 + 128^2 z2 in int64.
 *     3. The rule.  B = [[n, s_i, s_j], [s_i, q_i, d], [s_j, d, q_j]], Delta = det B, A = adj B, c = (d, e, f), u = (Y, u_i, u_j), and
 *            Sxx = Delta h - c^T A c,   Sxy = Delta z - c^T A u,   Syy = Delta T - u^T A u
 *        in 128-bit integers (no term exceeds 2^110).  Delta Sxx, Delta Sxy, Delta Syy are Delta^2 times the residual sums of squares and
 *        products of g_i g_j and y after the regression on (1, g_i, g_j).
 *     4. The pair is UNDEFINED (stat = NaN) unless n > 4, Delta > 0 and Sxx > 0.  That makes i = j, a monomorphic marker, a duplicate
 *        marker and a product that lies in the span of its factors undefined, with no special case.
 *     5. Otherwise, with t53(x) = x truncated toward zero to its top 53 bits, as a double, and every fp64 operation one correctly rounded
 *        operation in this order (nothing contracts into an FMA),
 *            r2   = (t53(Sxy) / t53(Sxx)) * (t53(Sxy) / t53(Syy))
 *            stat = ((double)(n - 4) * r2) / (1.0 - r2),          stat = +inf when !(r2 < 1.0).
 *        A zero Syy (the trait lies in the span of 1, g_i, g_j: nothing is left to explain) has Sxy = 0 too, so r2 = 0 * (0 / 0) = NaN
 *        and the pair lands in +inf, not in NaN: it is defined, and it is a hit at every min_stat.  A constant trait does this for every
 *        defined pair; r_api.Epistasis refuses one.
 *     6. A hit is stat >= min_stat.  NaN is never a hit; min_stat = -inf makes every defined pair a hit.
 *
 *     What is not claimed.  Agreement with the PLINK or GLIDE programs is neither claimed nor tested, because neither is available: the
 *     tests hold the statistic to exact rational arithmetic instead.  Sex chromosomes, dominance terms and case/control traits are out
 *     of scope.  No p-value is computed here (r_api.Epistasis adds scipy's fdtrc).
 *
 *     eagle_epistasis_loci tests every marker against each of 1 <= nloci <= 64 listed loci (repeats allowed); the output is dense:
 *     stat_out[i * nloci + k] for marker i and locus loci[k], mom_out (or NULL) the five pair sums (d, e, f, h, z) at
 *     [(i * nloci + k) * 5 ..], with marker i as g_i and the locus as g_j.  The file is read as eagle_ld_dots reads it: the loci's rows
 *     are gathered first, then the resident image where it lies, else row windows from the sidecar, the text or a VIEW alias's source;
 *     both give the same bits.
 *
 *     eagle_epistasis_pairs tests all pairs i < j except those with j - i <= gap on the same chromosome (chrom NULL: one chromosome;
 *     gap = 0 skips nothing).  *ntested_out = the defined pairs among those not skipped; *max_out = the largest defined stat and its
 *     pair, ties to the smallest (i, j), or (-1, -1, NaN) if none is defined.  *nhits_out is always the total number of hits; the
 *     tables hit_ij (hit_cap x 2), hit_stat (hit_cap), hit_mom (hit_cap x 5: d, e, f, h, z) are written, sorted by (i, j), iff the total
 *     is <= hit_cap and untouched otherwise.  The call returns EAGLE_OK either way (eagle_roh's seg_cap semantics).  Two deterministic
 *     passes without global atomics: per tile pair the counts and the maximum, then the tile pairs that have hits once more into their
 *     slots.  The image must be resident or fit max_memory_in_Gbytes: otherwise EAGLE_ERR_ARG with a message that says to prune or
 *     filter first -- a streamed all-pairs pass does not exist.
 *
 *     Single device: a multi-device context works on its first device.  Argument errors (EAGLE_ERR_ARG: a NULL pointer, dims <= 0,
 *     n > EAGLE_EPI_MAX_N, |y| > EAGLE_EPI_YMAX, nloci outside [1, 64], a locus outside [0, L), gap < 0, min_stat NaN, hit_cap < 0, NULL
 *     tables with hit_cap > 0) are decided before the context is used; with ctx == NULL their text is in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */
#define EAGLE_EPI_MAX_N 65535L
#define EAGLE_EPI_YMAX 1000000
typedef struct eagle_epi_max { int64_t i, j; double stat; } eagle_epi_max;

int eagle_epistasis_loci(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const int32_t* y, const long* loci, long nloci,
                         double max_memory_in_Gbytes, double* stat_out, int64_t* mom_out);
int eagle_epistasis_pairs(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const int32_t* y, const int32_t* chrom, long gap,
                          double min_stat, double max_memory_in_Gbytes, int32_t* hit_ij, double* hit_stat, int64_t* hit_mom, long hit_cap,
                          long* nhits_out, long* ntested_out, eagle_epi_max* max_out);

/* ---------------------------------------------------------------------------------------------
 * 1b''''iii. Per-group genotype counts and Fisher's exact test (no counterpart in the reference, whose panel is one population with one
 *     quantitative trait): the genotype counts of every marker WITHIN each group of individuals, the one primitive under per-population
 *     allele frequencies, Fst, the Hardy-Weinberg test among controls only and the case/control association tests.  The counts are exact
 *     integers, so the device and a numpy restatement (r_api.group_counts_host, r_api.bed_group_counts_host) agree with ==; every
 *     statistic is the caller's fp64 arithmetic on them (r_api.GroupCounts, r_api.Fst, r_api.CaseControl).
 *
 *     1. Inputs.  labels[i] in {-1, 0, ..., K - 1}, one int32 per individual; -1 = in no group.  1 <= K <= EAGLE_GROUPS_MAX = 64.  With a
 *        VIEW alias of eagle_reshape_m, labels has dims[0] entries: one per kept individual.  size_k = the number of individuals with
 *        label k.
 *     2. Image route (eagle_group_counts).  g in {-1, 0, +1} over the individuals of Mt.ascii; a missing call of the source is a
 *        heterozygote by now.  s_mk = sum_{i in k} g_im and q_mk = sum_{i in k} g_im^2, then n2 = (q + s) / 2, n0 = (q - s) / 2,
 *        n1 = size_k - q:  counts_out[(m K + k) 3 + c], c = 0, 1, 2, is int32 of shape L x K x 3, the numbers of '0', '1', '2'
 *        characters of line m among group k.  On the device s and q are two products of the int8 image with the one-hot label operand on
 *        v_mfma_i32_32x32x32_i8 (k_group_tile, csrc/eagle_groups.hip); the image is read once.
 *     3. .bed route (eagle_bed_group_counts).  counts_out[(m K + k) 4 + c] = (homozygous A1, code 00; heterozygous, 10; homozygous A2,
 *        11; missing, 01) of marker m among group k, int32 of shape L x K x 4, by popcounts of the two bit planes against K bit-mask
 *        planes (k_bed_group_counts).  The unused bit pairs of a row's last byte are not counted.
 *     4. Invariants.  Summed over k with every individual labelled, the counts are those of eagle_marker_counts /
 *        eagle_bed_marker_counts exactly; K = 1 with all labels 0 IS those calls.  A group without an individual has zero counts.
 *     5. Fisher's exact test of a 2 x 2 table (a, b; c, d), two-sided (eagle_fisher_2x2).  r1 = a + b, r2 = c + d, c1 = a + c,
 *        N = r1 + r2;  N = 0 gives p = 1.  x runs over lo = max(0, c1 - r2) .. hi = min(r1, c1), the values the first cell can take
 *        under the margins.  Unnormalised probabilities start from the mode x0 = clamp(floor((r1 + 1) (c1 + 1) / (N + 2)), lo, hi) with
 *        P(x0) = 1 and follow
 *            P(x - 1) = P(x) * x (r2 - c1 + x) / ((r1 - x + 1) (c1 - x + 1)),      P(x + 1) = P(x) * (r1 - x) (c1 - x) / ((x + 1) (r2 - c1 + x + 1)).
 *        Each step is  P' = fl(fl(P * (double)num) / (double)den):  num and den are exact int64 products converted to fp64 once, the
 *        product and the quotient are rounded separately.  The terms are visited in ONE order: x0, then the lower leg x0 - 1, ..., lo,
 *        then the upper leg x0 + 1, ..., hi; a leg ends at its first term that is exactly 0.0 (adding zeros changes no bit).  First walk:
 *        total = 1.0, then total = fl(total + P) for every further term in that order; P(a) is picked up on the way (0.0 if a leg ended
 *        before it).  cut = fl(P(a) * 1.0000001).  Second walk, the same steps in the same order:  tail = (1.0 <= cut ? 1.0 : 0.0),
 *        then tail = fl(tail + P) for every term with P <= cut.  p = min(1, fl(tail / total)).  The factor 1.0000001 is the rule of R's
 *        fisher.test: without it the balanced designs that are the common case (r1 = r2) have mathematically tied terms x and c1 - x
 *        that the two legs round differently, and the p-value would hang on the last bit.  Nothing is contracted into an FMA and no
 *        array is kept per table, so a scalar restatement in any IEEE-754 language gives the same bits (r_api.fisher_2x2_host).
 *
 *     What is not claimed.  Agreement with the PLINK program is neither claimed nor tested, because it is not available: the tests hold
 *     the counts to loops over individuals and the statistics to exact rational arithmetic.  Logistic regression with covariates is
 *     section 1b''''iv; stratified (Cochran-Mantel-Haenszel) tests and sex chromosomes are out of scope.
 *
 *     The image route reads the file as eagle_marker_counts reads it: the resident image where it lies (it is never modified), else row
 *     windows from the sidecar, the text or a VIEW alias's source; rows are independent and the label operand is built once per call, so
 *     every route gives the same integers.  The .bed route stages the rows as eagle_bed_marker_counts does.  Single device: a
 *     multi-device context works on its first device.  Argument errors (EAGLE_ERR_ARG: a NULL pointer, dims <= 0, K outside [1, 64],
 *     a label outside [-1, K), n > 2^30 - 1, a negative table entry, a table sum above 2^30) are decided before the context is used;
 *     with ctx == NULL their text is in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */
#define EAGLE_GROUPS_MAX 64

int eagle_group_counts(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const int32_t* labels, int K,
                       double max_memory_in_Gbytes, int32_t* counts_out);
int eagle_bed_group_counts(eagle_ctx* ctx, const char* bed_path, const long dims[2], const int32_t* labels, int K,
                           double max_memory_in_Gbytes, int32_t* counts_out);
/* p_out[i] = the test above on tables[4 i .. 4 i + 3] = (a, b, c, d), i < L; one table per device thread (k_fisher_2x2).
 * EAGLE_ERR_ARG also for L <= 0. */
int eagle_fisher_2x2(eagle_ctx* ctx, const int32_t* tables, long L, double* p_out);

/* ---------------------------------------------------------------------------------------------
 * 1b''''iv. Logistic regression of a binary trait on covariates and one marker at a time (no counterpart in the reference): what
 *     eagle_group_counts' case/control tests cannot do, take covariates (the principal components of section 1b'''', sex, age).  For
 *     marker m over the used individuals i (status[i] in {0, 1}; -1 = not used)
 *            logit P(y_i = 1) = x_i' beta + g_im gamma,
 *     X is n x c column-major fp64 as R holds it, and the caller supplies the intercept column;  1 <= c <= 15, so p = c + 1 <= 16
 *     parameters;  g in {0, 1, 2} counts the '2' character of line m (the image value plus one): the allele whose odds ratio
 *     CaseControl reports.  x~_i = (x_i, g_im), gamma is the LAST parameter.  A missing call of the source is a heterozygote by now.
 *     r_api.logistic_host is a scalar restatement of the rule below.
 *
 *     1. Start.  Every fit starts at (beta0, 0), beta0 = the covariates-only fit over the used individuals, computed once by the
 *        caller (r_api.logistic_null_host: fp64 Newton with the stop rule of 4) and passed in.
 *     2. One evaluation at beta.  eta_i = x~_i' beta, mu_i = 1 / (1 + e^-eta_i), w_i = mu_i (1 - mu_i), U = sum (y_i - mu_i) x~_i,
 *        I = sum w_i x~_i x~_i', l = sum [y_i eta_i - log(1 + e^eta_i)], all over the used individuals.  With e = exp(-|eta|):
 *        mu = 1 / (1 + e) for eta >= 0 and e / (1 + e) else, w = e / (1 + e)^2, log(1 + e^eta) = max(eta, 0) + log1p(e), and y - mu is 1 - mu = e / (1 + e) for eta >= 0, 1 / (1 + e) else, or -mu: no overflow
 *        and no cancellation, so U does not round to zero on a separated marker before code 3 is met.
 *        The Cholesky factor I = L L' is taken column by column; a pivot must be finite and above 2^-40 of its diagonal entry of I
 *        (a column that the columns before it explain to the resolution of fp64 is not positive), else code 2.  gamma is last, so
 *        (I^-1)_gg = 1 / L_gg^2.
 *     3. Score test.  The first evaluation gives it: score = U_g^2 (I^-1)_gg, the test of gamma = 0 with 1 degree of freedom.  With
 *        c = 1 (intercept only) this is the Cochran-Armitage trend statistic of case_control_from_counts, N num^2 / (R S tvar).
 *     4. Maximum likelihood.  Solve I delta = U by the factor; scale delta so that max |delta_j| <= 5; beta <- beta + delta; stop when
 *        max_j |delta_j| <= tol; at most max_iter evaluations.  Order inside an evaluation: factor (code 2), the score if it is the
 *        first, max_i |eta_i| > 40 (code 3), the step, the stop.
 *     5. Firth (Heinze and Schemper 2002).  h_i = w_i x~_i' I^-1 x~_i, U*_j = sum [y_i - mu_i + h_i (1/2 - mu_i)] x~_ij, I delta = U*
 *        with the same cap and stop as ML and no step halving.  I^-1 is needed before h, so a Firth evaluation takes two passes over
 *        the individuals.  Inference is Wald from I(beta)^-1 as PLINK 2 does; the penalised likelihood-ratio test is not reported.
 *        Code 3 is not raised.
 *     6. Per-marker result.  stat_out[4 m ..] = (gamma, se = sqrt((I^-1)_gg), score, l) and info_out[2 m ..] = (code, evaluations of
 *        the fit reported).  gamma is beta_g after the last step; se and l are those of the last evaluation, whose point lies within
 *        that step (at most tol) of it.  Codes: 0 converged; 1 max_iter reached; 2 a Cholesky pivot of I was not positive or not
 *        finite (a marker that is monomorphic among the used individuals makes gamma's column the intercept's at the first
 *        evaluation; later on, a separated marker whose weights vanish everywhere but on one genotype does the same); 3 separation (ML
 *        only): some evaluation had max_i |eta_i| > 40, that individual's weight is below the resolution of fp64; + 256 the value
 *        reported is the Firth fit.  gamma, se and l are NaN unless the code's low byte is 0; score is NaN only under code 2 at the
 *        first evaluation.
 *     7. firth = 0: ML only.  1: Firth for every marker (every code carries + 256).  2 (fallback): ML first; a marker whose ML fit ends
 *        with code 1, 2 or 3 after the first evaluation (a code 2 AT the first evaluation stays: Firth meets the same matrix) is
 *        restarted from (beta0, 0) with Firth, in the same kernel and by the same wave; the score stays the first evaluation's.
 *
 *     On the device (k_logit_irls<firth>, csrc/eagle_logit.hip) one wave owns one marker; I is the 16 x 16 x n product
 *     (diag(w) X~)' X~ accumulated on v_mfma_f64_16x16x4_f64 with p padded to 16, four individuals an instruction; eta, mu, w and the
 *     likelihood term are evaluated once per individual; the factor, the solves and I^-1 are the wave's own fp64 work in LDS.  X~ is
 *     staged once per call as an n x 16 padded image with the status as one byte per individual; an unused individual contributes
 *     w = 0 and residual 0 (nothing is gathered), and the genotype column is read from the image row.  No atomics; a marker's result
 *     depends on its row, X, status and beta0 alone, so it does not depend on how markers fall into row windows or workgroups.
 *
 *     What is not claimed.  Agreement with the PLINK or logistf programs is neither claimed nor tested, because neither is available:
 *     the tests hold the fits to 40-digit roots of the same equations.  Bit equality with the host restatement is not claimed either:
 *     exp, log1p and the matrix pipe's summation order are not fixed by IEEE 754.  Stratified tests and sex chromosomes stay out of
 *     scope; so does a .bed route, where a missing call would change the used individuals, and with them the null fit, per marker.
 *
 *     The file is read as eagle_group_counts reads it: the resident image where it lies, else row windows from the sidecar, the text
 *     or a VIEW alias's source; with a VIEW alias status and X have one entry per kept individual.  Single device: a multi-device
 *     context works on its first device.  Argument errors (EAGLE_ERR_ARG: a NULL pointer, dims <= 0, n > 2^30 - 1, c outside [1, 15],
 *     a status outside {-1, 0, 1}, a non-finite X entry of a used individual or beta0 entry, firth outside {0, 1, 2}, tol not in
 *     (0, 1), max_iter outside [1, 1000], no case or no control among the used individuals) are decided before the context is used;
 *     with ctx == NULL their text is in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */
int eagle_logistic(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const int32_t* status, const double* X, int c,
                   const double* beta0, int firth, double tol, int max_iter, double max_memory_in_Gbytes, double* stat_out,
                   int32_t* info_out);

/* ---------------------------------------------------------------------------------------------
 * 1b''''v. Admixture: model-based ancestry proportions (no counterpart in the reference, whose panel is one population): for K
 *     ancestral populations the fractions Q (n x K, rows sum to 1) of every individual and the allele frequencies F of every
 *     population, by EM on the likelihood of FRAPPE (Tang et al. 2005), ADMIXTURE (Alexander et al. 2009) and STRUCTURE.  The groups
 *     that eagle_group_counts, Fst and the case/control tests take from the caller come from here (argmax_k Q), and the columns of Q
 *     are covariates for the association models as the principal components of section 1b'''' are.
 *
 *     1. Model.  g in {-1, 0, +1} over the individuals of line m of Mt.ascii, d = g + 1 copies of the allele that the character '2'
 *        stands for; a missing call of the source is a heterozygote by now.  For individual i and marker m
 *            p_im = sum_k q_ik f_km,      pbar_im = sum_k q_ik (1 - f_km):
 *        p-bar is its own sum, never 1 - p, so every sum of the rule has non-negative terms and is well conditioned in any order.
 *            l(Q, F) = sum_m sum_i [ d ln p + (2 - d) ln pbar ],   a term with a zero factor (d = 0, or d = 2) being 0.
 *     2. One EM step (Q, F) -> (Q', F').  With A_im = d_im / p_im and B_im = (2 - d_im) / pbar_im:
 *            sa_km = f_km sum_i q_ik A_im,      sb_km = (1 - f_km) sum_i q_ik B_im,
 *            f'_km = clamp(sa / (sa + sb), eps, 1 - eps),   and f'_km = f_km where sa + sb = 0 (no individual has a part in k);
 *            t_ik = q_ik sum_m (f_km A_im + (1 - f_km) B_im),
 *            q'_ik = max(t_ik / (2 L), eps), then every row of Q' is divided by its sum.
 *        eps = EAGLE_ADMIX_EPS = 1e-6 and 1 <= K <= EAGLE_ADMIX_KMAX = 16.  Both halves use the OLD (Q, F).  The likelihood never
 *        falls under a step, up to the floors.  With K = 1 one step gives f' = clamp(mean(d) / 2).
 *     3. Storage.  Q is n x K row-major, F is L x K row-major (the frequencies of a window of markers are contiguous), both in and out.
 *        loglik_out has steps + 1 entries: entry t is l at the parameters entering step t, the last entry is l at the returned
 *        parameters, from a likelihood-only pass of the same kernel.  steps = 0 computes loglik_out[0] and returns Q and F untouched.
 *     4. Individuals with index >= n do not exist: the kernels mask them and do not rely on the image's padding (a zero byte would be
 *        a heterozygote).
 *
 *     On the device (csrc/eagle_admix.hip) a step is two tile kernels over the image, both on v_mfma_f64_16x16x4_f64 with K padded to
 *     16.  k_admix_f: a wave owns 16 markers and walks the individuals 16 at a time; the tile of p and of pbar is ceil(K / 4)
 *     instructions each, a lane turns its four entries into A and B, and the C/D registers are, as they lie, the B operand of the
 *     sums over individuals; the lane then writes f'.  The likelihood's terms ride in one register per lane, one partial per 16-marker
 *     tile, added by k_admix_ll_finish in a fixed order.  k_admix_q is the transposed tile (16 individuals per wave), with the markers
 *     cut into S ranges whose number and boundaries (multiples of 16) are a function of (n, L) alone (admix_range_plan,
 *     csrc/eagle_host.h); a range's accumulator lives in the partials buffer part[S][n16][16], and k_admix_q_finish adds the ranges
 *     in order, applies q / (2 L), the floor and the normalisation.  No atomics.  The whole loop of `steps` stays on the device: Q, F
 *     and l cross the bus once per call and direction.
 *
 *     The same words on every route.  f'_m depends on line m alone; q' depends on the order of the markers and the range plan, never on
 *     how the lines fall into row windows: a streamed window holds a multiple of 16 lines, and a window that ends inside a range
 *     leaves the accumulator in the partials buffer in fp64, where the next window takes it up.  So the resident image, the sidecar,
 *     row windows, the text and a VIEW alias return the same words, and so do steps = 5 and five calls with steps = 1.  Bit equality
 *     with the host restatement (r_api.admixture_host) is not claimed: the matrix pipe's summation order and log are not fixed by
 *     IEEE 754; the tests hold both to 40-digit arithmetic within bounds derived from the number of non-negative terms.
 *
 *     Out of scope: a .bed route that skips missing calls, supervised mode (known ancestries held fixed), cross-validation of K,
 *     device-held state between calls, sex chromosomes.  Agreement with the ADMIXTURE or STRUCTURE programs is neither claimed nor
 *     tested, because neither is available.  The accelerated driver (SQUAREM), the start and the ordering of the components are
 *     r_api.Admixture's.
 *
 *     The file is read as eagle_group_counts reads it; with a VIEW alias Q has one row per kept individual.  Single device: a
 *     multi-device context works on its first device.  Argument errors (EAGLE_ERR_ARG: a NULL pointer, dims <= 0, n > 2^30 - 1, K
 *     outside [1, 16], steps outside [0, 10000], a non-finite Q or F entry, an F entry outside [eps, 1 - eps], a negative Q entry, a Q
 *     row whose sum is off 1 by more than 1e-9) are decided before the context is used; with ctx == NULL their text is in
 *     eagle_open_error().
 * ------------------------------------------------------------------------------------------- */
#define EAGLE_ADMIX_EPS 1e-6
#define EAGLE_ADMIX_KMAX 16

int eagle_admixture_em(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], int K, int steps, double* Q, double* F,
                       double max_memory_in_Gbytes, double* loglik_out);

/* ---------------------------------------------------------------------------------------------
 * 1b''''vi. max(T) permutation p-values of every marker against one trait (no counterpart in the reference; PLINK's --assoc --mperm /
 *     --model trend --mperm): per marker how often a permuted trait's statistic reaches the observed one (EMP1's count), and per
 *     permutation the largest statistic over all markers (EMP2's reference distribution, Westfall and Young), which respects the LD
 *     between the markers.  All sums are integers, so the device and a numpy restatement (r_api.maxt_host) agree with == on every output.
 *
 *     1. Inputs.  g in {-1, 0, +1} over the individuals of line m of Mt.ascii, dims = (n, L); a missing call of the source is a
 *        heterozygote by now.  t[n] int32 with |t_i| <= EAGLE_MAXT_TMAX = 10^6.  used[n] bytes (non-zero = used) or NULL = everybody;
 *        the used individuals are u_0 < ... < u_{N-1}.  strata[n] int32 in [0, 2^16) or NULL; only the entries of used individuals are
 *        read.  seed uint64.  first >= 1 and R >= 1: this call makes the permutations with the ordinals first, ..., first + R - 1.
 *        perm, optional: int32 [R][N], every row a permutation of 0 .. N - 1.  Limits: n <= EAGLE_MAXT_MAX_N = 65,535; 3 <= N;
 *        R <= EAGLE_MAXT_RMAX = 1024 per call; first + R <= 2^31.  With a VIEW alias t, used and strata have one entry per kept
 *        individual.
 *     2. Integers, over the used individuals only.  S_m = sum g, Q_m = sum g^2, V_m = N Q_m - S_m^2;  T = sum t, W = N sum t^2 - T^2;
 *        W = 0 (a constant trait) is an argument error.  For an arrangement t' of the trait c_m(t') = sum_k g_{u_k, m} t'_{u_k} and
 *        d_m(t') = N c_m - S_m T.  Bounds: |c| <= N 10^6, so |N c| <= 65535^2 10^6 < 4.3 10^15, |S_m T| <= N . N 10^6 likewise, and
 *        |d| < 8.6 10^15 < 2^53 = 9.007 10^15;  0 <= V_m <= N^2 < 2^32 (Cauchy-Schwarz below, Q <= N above).  Both convert to fp64
 *        exactly.
 *     3. Key.  key_m(t') = fl(fl(d d) / V_m) in fp64: the product and the quotient are rounded separately, nothing is contracted into
 *        an FMA; key = 0 where V_m = 0 (a monomorphic marker).  r^2 = key / W;  the Cochran-Armitage trend chi-square of a 0/1 trait
 *        is N r^2 and the F(1, N - 2) of the regression slope is (N - 2) r^2 / (1 - r^2): both increase with key, so the largest key is
 *        the largest statistic.
 *     4. Seeded permutation r >= 1.  For j < N, with counter = r 2^16 + j + 1 (all arithmetic mod 2^64):
 *            z = seed + counter 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) 0x94D049BB133111EB;
 *            z ^= z >> 31;  h = z >> 32
 *        (the splitmix64 finaliser; h has 32 bits).  key64(r, j) = (strata[u_j] << 48) | (h << 16) | j, with stratum 0 when strata is
 *        NULL: the keys of one r are distinct, and two equal hashes fall back to j -- about N^2 / 2^33 pairs per permutation, half a
 *        pair at N = 65,535.  pi_r[k] = the j of the k-th smallest key64(r, .);  sigma[k] = the j of the k-th smallest (strata[u_j], j),
 *        the identity without strata.  t^(r)[u_sigma[k]] = t[u_pi_r[k]].  Trait values never leave their stratum; with every individual
 *        in its own stratum every permutation is the identity.  With perm given t^(r)[u_k] = t[u_perm[r - first][k]], and seed and strata
 *        are ignored.  The rule fixes the result, not the sort: the device runs a bitonic network (csrc/eagle_maxt.hip).
 *     5. Outputs.  d_obs[L] int64 = d_m(t), V[L] int64, key_obs[L] fp64 = key_m(t);  count1[L] int32 = #{r : |d_m(t^(r))| >= |d_obs,m|},
 *        compared in int64;  maxkey[R] fp64 = max_m key_m(t^(r)) and argmax[R] int32 = the lowest m that attains it.  count1 depends on
 *        (seed, first, R) alone: calls over [1, a] and [a + 1, R] add up to one call over [1, R], and their maxkey and argmax
 *        concatenate.  Nothing depends on tiles, windows or the route: integer sums and an fp64 maximum are free of order.
 *     6. Operand.  The device multiplies the int8 image with an int8 operand [P][R][ld] on v_mfma_i32_32x32x32_i8 (k_maxt_tile): plane p
 *        of arrangement r holds digit p of t^(r) in sign-magnitude base 128, t = sign(t) (m_0 + 128 m_1 + 16384 m_2), m in [0, 127],
 *        digit = sign(t) m_p in [-127, 127];  P = 1 for max |t| <= 127 (a 0/1 case indicator), 2 up to 16,383, else 3 (up to
 *        2,097,151).  c = c_0 + 128 c_1 + 16384 c_2 in int64 in the tile's epilogue, which forms d, the count1 contributions and the
 *        tile's largest key per permutation; no L x R array is stored.  S and Q come from eagle_group_counts' kernel with `used` as one
 *        group; the observed pass is the same tile on the trait itself.
 *
 *     What is not claimed.  Agreement with the PLINK program is neither claimed nor tested, because it is not available: the tests hold
 *     the outputs to loops over individuals on exact integers and fractions.  Out of scope: covariates (pass a residual as the trait), a
 *     .bed route (N would differ per marker), adaptive early stopping (--perm), step-down corrections, permutation of the Logistic and
 *     GWAS fits, several devices, sex chromosomes.
 *
 *     The file is read as eagle_group_counts reads it: the resident image where it lies, else row windows from the sidecar, the text or a
 *     VIEW alias's source.  Single device: a multi-device context works on its first device.  Argument errors (EAGLE_ERR_ARG: a NULL
 *     pointer, dims <= 0, n > 65,535, N < 3, |t| > 10^6, W = 0, a stratum outside [0, 2^16), first < 1, R outside [1, 1024],
 *     first + R > 2^31, a perm row that is no permutation) are decided before the context is used; with ctx == NULL their text is in
 *     eagle_open_error().
 * ------------------------------------------------------------------------------------------- */
#define EAGLE_MAXT_MAX_N 65535L
#define EAGLE_MAXT_TMAX 1000000
#define EAGLE_MAXT_RMAX 1024L

int eagle_maxt(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const int32_t* t, const uint8_t* used, const int32_t* strata,
               uint64_t seed, long first, long R, const int32_t* perm, double max_memory_in_Gbytes, int64_t* d_obs, int64_t* V,
               double* key_obs, int32_t* count1, double* maxkey, int32_t* argmax);

/* ---------------------------------------------------------------------------------------------
 * 1b''''vii. Pairwise haplotype frequencies, Lewontin's D' and the verdicts haplotype blocks are cut from (no counterpart in the
 *     reference; PLINK's --r2 dprime and --blocks, Haploview): for every pair of markers at most `window` <= 256 apart the four
 *     haplotype frequencies estimated from the unphased genotypes by EM, D', the haplotype r2, and two bits.  The genotype r2 of
 *     1b'' cannot give them: the phase of the double heterozygotes is unknown, and D' needs the haplotype frequencies.  Integers until
 *     a short fp64 epilogue whose order of operations is fixed, so the device and a numpy restatement (r_api.hap_ld_host) agree with ==
 *     on every output.
 *
 *     1. Genotypes and marginals.  g in {-1, 0, +1} over the individuals of line m of Mt.ascii, dims = (n, L); a missing call is a het,
 *        as everywhere on this route.  Allele B is the allele of '2'.  Per marker s = sum g and q = sum g^2 (k_marker_counts);
 *        b_i = n + s_i is the number of B alleles out of 2n;  a marker is polymorphic iff 0 < b_i < 2n.
 *     2. Pair sums and the 3 x 3 table.  For markers i < j four int32 sums over the individuals:  d = sum g_i g_j,  e = sum g_i^2 g_j^2,
 *        f = sum g_i^2 g_j,  h = sum g_i g_j^2.  The nine cells N_ab (a, b = the number of B alleles at i and at j) are exact integers:
 *            N22 = (e + f + h + d) / 4    N00 = (e - f - h + d) / 4    N20 = (e - f + h - d) / 4    N02 = (e + f - h - d) / 4
 *            N12 = (q_j + s_j - e - f) / 2    N10 = (q_j - s_j - e + f) / 2    N21 = (q_i + s_i - e - h) / 2    N01 = (q_i - s_i - e + h) / 2
 *            N11 = x = n - q_i - q_j + e      (the double heterozygotes, whose phase is unknown)
 *     3. Known haplotype counts.  k_BB = 2 N22 + N21 + N12,  k_BA = 2 N20 + N21 + N10,  k_AB = 2 N02 + N01 + N12,
 *        k_AA = 2 N00 + N01 + N10  (first letter: marker i);  k_BB + k_BA + k_AB + k_AA + 2x = 2n.
 *     4. The EM, in fp64.  Every operation is a single correctly rounded multiplication, addition, subtraction or division
 *        (the device code is compiled with contraction switched off), so nothing contracts into an FMA.  T = (double)(2n);  p_i = (double)b_i / T,
 *        q_i = (double)(2n - b_i) / T, formed from the integer and never as 1 - p_i.  Start at equilibrium: pBB = p_i p_j, pBA = p_i q_j,
 *        pAB = q_i p_j, pAA = q_i q_j.  With x = 0 there is no iteration: every p is k / T.  Otherwise repeat
 *            u = pBB pAA;  v = pBA pAB;  den = u + v;  t = den > 0 ? u / den : 0.5;  xt = x t;  xo = x - xt;
 *            the new pBB, pAA, pBA, pAB = (k_BB + xt) / T, (k_AA + xt) / T, (k_BA + xo) / T, (k_AB + xo) / T;
 *            delta = |pBB_new - pBB|;  iterations += 1;
 *            stop with code 0 when delta <= tol, else stop with code 1 when iterations = max_iter.
 *        Defaults tol = 1e-10 and max_iter = 1000.  This is the local optimum reached from the equilibrium start, which is Haploview's
 *        EM.  It is not PLINK's cubic solver, which compares all roots of the likelihood equation: where the likelihood has two
 *        maxima the two can differ.
 *     5. Statistics.  D = pBB - p_i p_j;  Dmax = min(p_i q_j, q_i p_j) when D >= 0, else min(p_i p_j, q_i q_j);  D' = D / Dmax, clamped to
 *        [-1, 1];  r2_h = (D D) / ((p_i q_i)(p_j q_j));  pmin = the smallest of the four haplotype frequencies.
 *     6. Verdicts.  RECOMBINANT: all four gametes are seen, iff pmin > fg_cut, strictly (default 0.01, Haploview's four-gamete
 *        cutoff).  STRONG: iff |D'| >= dprime_cut (default 0.8).
 *     7. Undefined pairs.  A pair with i + o >= L, or with a monomorphic member, is undefined: neither bit is set, D' is reported as
 *        -2.0 and r2_h as -1.0.  With n = 1 no pair is defined: one individual says nothing about association.
 *     8. Outputs.  recomb_mask_out and strong_mask_out have eagle_ld_window's shape, L x ceil(window / 64) uint64: bit o - 1 of row i
 *        is the pair (i, i + o).  dprime_out and r2_out are L x window fp64, entry (i, o - 1).  Each of the four may be NULL (the two
 *        bands are held whole on the device while the call runs: 16 L window bytes).  counts_out[4] = the defined pairs, the pairs
 *        that stopped with code 1, the recombinant bits, the strong bits.  Every output word is written by one workgroup of one
 *        launch that held all partners of its marker, and the totals are integers: nothing depends on tiles, windows or the route.
 *
 *     The kernel (k_hapld_tile, csrc/eagle_hapld.hip) has k_ld_tile's geometry on v_mfma_i32_32x32x32_i8 with four products per block
 *     pair, g.g, g^2.g^2, g^2.g and g.g^2; only the genotype image is staged, g^2 is made in registers.
 *
 *     What is not claimed.  Agreement with the PLINK or Haploview programs is neither claimed nor tested, because neither is
 *     available: the tests hold the outputs to counting loops, a scalar loop of this rule and the same EM at 40 digits.  Out of
 *     scope: Gabriel's confidence-interval blocks (their likelihood grid needs log, which IEEE 754 does not fix), a .bed route with
 *     pairwise-complete tables (nine products), a picks mode against listed loci, multi-marker haplotype frequencies inside a block,
 *     several devices, sex chromosomes.
 *
 *     The file is read as eagle_ld_window reads it: the resident image where it lies, else row windows that overlap by `window` rows
 *     from the sidecar, the text or a VIEW alias's source.  Single device: a multi-device context works on its first device.
 *     Argument errors (EAGLE_ERR_ARG: a NULL path, dims or counts_out, dims <= 0, n > 2^30 - 1, window outside [1, 256], tol not in
 *     (0, 1), max_iter outside [1, 100000], a cut outside [0, 1]) are decided before the context is used; with ctx == NULL their text is
 *     in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */
int eagle_hap_ld(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], long window, double tol, int max_iter, double fg_cut,
                 double dprime_cut, double max_memory_in_Gbytes, uint64_t* recomb_mask_out, uint64_t* strong_mask_out, double* dprime_out,
                 double* r2_out, int64_t* counts_out);

/* ---------------------------------------------------------------------------------------------
 * 1b''''viii. Transmission disequilibrium test of parent-offspring trios (no counterpart in the reference; Spielman 1993; PLINK's
 *     --tdt, --tdt poo and --tdt mperm): among heterozygous parents of affected children, is the '2' allele passed on more often than
 *     not?  The test is immune to population stratification, which the case/control tests of 1b''''iii are not.  On the bit planes of
 *     1b'''vii with the trios of 1b'''viii.  All outputs are integers or two correctly rounded fp64 operations on exact operands, so
 *     the device and a numpy restatement (r_api.tdt_host) agree with == on every output.
 *
 *     Genotypes, called, trios and their argument errors are rules 1 and 2 of 1b'''viii (Mendel).  H = C & ~A & ~B is the het plane.  A trio
 *     with an unknown parent is legal and contributes nothing.
 *
 *     1. Complete.  K = C_c & C_f & C_m & ~E, with E the Mendel error word of rule 3 of 1b'''viii: all three are called and the trio
 *        has no Mendel error there.  Hf = H_f & K and Hm = H_m & K are the informative het parents.
 *     2. Transmissions of the '2' allele.  A2 is the allele of genotype +1, the one CaseControl and Logistic report.
 *            PT = Hf & (B_c | H_c & A_m)     PU = Hf & (A_c | H_c & B_m)
 *            MT = Hm & (B_c | H_c & A_f)     MU = Hm & (A_c | H_c & B_f)
 *            W  = Hf & Hm & H_c
 *        PT / PU: the father passed A2 / A1; MT / MU: the same for the mother.  W: het x het -> het, one A2 and one A1 were passed
 *        and the origin is unknown.  Of the 27 called code triples 11 are informative, and popcount(Hf) + popcount(Hm) = PT + PU + MT
 *        + MU + 2 W on every triple (tests/tdt_truth.py enumerates the allele choices of all 64).  Per trio and marker
 *        d = PT + MT - PU - MU lies in [-2, 2].
 *     3. Per-marker output.  marker_out: L x 5 int32 = (PT, PU, MT, MU, W), summed over the trios of the list; a trio listed twice
 *        counts twice.  T = PT + MT + W, U = PU + MU + W, d_obs = T - U, V = T + U.  key_obs = fl(fl(d d) / V) in fp64, two separately
 *        rounded operations, 0 where V = 0: the TDT chi-square (T - U)^2 / (T + U) as it is reported.
 *     4. Per-trio output.  trio_out: ntrios x 6 int32 = (popcount K, popcount Hf, popcount Hm, T_t, U_t, W_t) over the panel, with
 *        T_t = PT + MT + W and U_t = PU + MU + W of the trio.
 *     5. Flips.  For R >= 1 only.  The family of trio t is family[t] if given, int32 in [0, 65535]; otherwise the smallest list
 *        position k with (f_k, m_k) = (f_t, m_t), so full sibs flip together.  Flip r >= 1 gives family phi the sign -1 when bit 31
 *        of h is set, else +1, with h the 32-bit splitmix64 value of rule 4 of 1b''''vi at counter = r 2^16 + phi + 1: transmitted and
 *        untransmitted alleles change places in the whole family.  d_m^(r) = sum_t s_r(phi_t) d_{t,m}; V does not change under a flip;
 *        key^(r) is as in rule 3.  count1[m] = #{r : |d_m^(r)| >= |d_obs,m|}, compared as integers.  maxkey[R] is the largest key of
 *        flip r and argmax[R] the lowest marker that attains it.  Calls over [first, first + R) add and concatenate exactly as
 *        eagle_maxt's do.
 *     6. Limits.  ntrios in [1, 2^27] when R = 0; ntrios <= 65,535, R <= 1024 per call and first + R <= 2^31 when R >= 1; panel markers
 *        < 2^31; n <= 0x3fffffff for the .bed file.  The planes stay on the device for the call with the per-trio and per-marker
 *        arrays and, for R >= 1, the int8 image of d (marker-major, leading dimension ceil16(ntrios)), the sign operand and the
 *        tiles' partial maxima; where the image does not fit the memory budget (rule 9 of 1b'''vii) beside the planes it is built
 *        and multiplied in bands of whole 128-marker tiles; where even one band does not fit the call returns EAGLE_ERR_NOMEM,
 *        decided before any kernel runs.  Argument errors are decided before the context is used; with ctx == NULL their text is in
 *        eagle_open_error().
 *     7. Not claimed and out of scope.  Agreement with the PLINK program is neither claimed nor tested.  Every marker is autosomal.
 *        On the ingested image a missing call is a het, which invents informative parents: the .bed route is the one for un-imputed
 *        panels.  Sib-TDT / DFAM, parental discordance tests, adaptive permutation, covariates and several devices are out of scope.
 *
 *     k_tdt_trios (csrc/eagle_tdt.hip) has one lane per trio as k_mendel_trios has, and turns the wave's 64 words of each of the five
 *     kinds into per-bit totals by ballot and popcount, added to marker_out with 32-bit integer atomics; k_tdt_finish forms d_obs, V
 *     and key_obs; k_tdt_image transposes 64 markers x 64 trios of d through LDS into the int8 image; k_tdt_signs writes the +-1
 *     operand; the product, count1 and the per-flip maxima are k_maxt_tile and k_maxt_finish of 1b''''vi as they stand (N = 1, T = 0,
 *     S = 0).  Single device: a multi-device context works on its first device.
 * ------------------------------------------------------------------------------------------- */
/* Rules 1 to 5 on the ingested panel M.ascii (dims = (n, L) of M).  trios: ntrios x 3 int32; family: ntrios int32 or NULL; trio_out:
 * ntrios x 6 int32; marker_out: L x 5 int32; key_obs: L fp64; R = 0 means counts only: count1 (L int32), maxkey (R fp64) and argmax (R
 * int32) may then be NULL and seed, first and family are not read. */
int eagle_tdt(eagle_ctx* ctx, const char* f_name_ascii_M, const long dims[2], const int32_t* trios, long ntrios, const int32_t* family,
              uint64_t seed, long first, long R, double max_memory_in_Gbytes, int32_t* trio_out, int32_t* marker_out, double* key_obs,
              int32_t* count1, double* maxkey, int32_t* argmax);

/* The same by PANEL marker (the Linc markers include selects, L bytes or NULL) from the SNP-major .bed file bed_path (dims = (n, L) of the
 * file), which still knows its missing calls: a trio with a missing call at a marker is not complete there. */
int eagle_bed_tdt(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, const int32_t* trios, long ntrios,
                  const int32_t* family, uint64_t seed, long first, long R, double max_memory_in_Gbytes, int32_t* trio_out,
                  int32_t* marker_out, double* key_obs, int32_t* count1, double* maxkey, int32_t* argmax);

/* ---------------------------------------------------------------------------------------------
 * 1c. Dense n x n model algebra on the device (OPT-IN: north_star keeps calculateH / calculateP / emma.* on
 *     host LAPACK, and nothing above calls these).  Once the scan takes tens of milliseconds the ~10-15 O(n^3) base-R calls
 *     of a find_qtl iteration are the whole run time (the author's note MyPackage/MyREADME:1 names eigen(); his MAGMA
 *     attempt is E/R/emma_eigen_R_wo_Z.R:9-15).  Column-major host matrices in and out, as R holds them.  The
 *     factorisations are rocSOLVER library calls (dlopen()ed on first use), the products this library's fp64 MFMA GEMM.
 * ------------------------------------------------------------------------------------------- */
/* eigen(A, symmetric = TRUE): values in DEcreasing order as R returns them, the matching eigenvectors in the columns of
 * vectors_out (NULL: only.values = TRUE).  Used by E/R/emma_eigen_L_wo_Z.R:3, emma_eigen_R_wo_Z.R:17, calculateMMt_sqrt_and_sqrtinv.R:25.
 * Only the LOWER triangle of the column-major matrix is read (as R's eigen(symmetric = TRUE) and LAPACK uplo 'L' do): for an input
 * that is symmetric only to rounding, a row-major buffer handed over as its transpose has its UPPER triangle read instead and the
 * result differs at rounding level.  Must not run under `rocprofv3 --pmc` (rocSOLVER aborts under counter collection,
 * profiles/r02_eigh_under_pmc.log). */
int eagle_sym_eig(eagle_ctx* ctx, const double* A, long n, double* values_out, double* vectors_out);
/* chol2inv(chol(A)) (calculateMMt_sqrt_and_sqrtinv.R:30, calculateP.R:27, calculate_reduced_vara.R:27).  Returns
 * EAGLE_SOFT_SENTINEL when A is not positive definite (R's chol() error text in eagle_last_error).  Only the UPPER triangle of
 * the column-major matrix is read (as R's chol() does); a row-major buffer handed over as its transpose has its lower triangle read. */
int eagle_chol2inv(eagle_ctx* ctx, const double* A, long n, double* Ainv_out);
/* solve(A) (calculate_reduced_vara.R:31-33, calculateP.R:28).  EAGLE_SOFT_SENTINEL for a singular matrix. */
int eagle_inverse(eagle_ctx* ctx, const double* A, long n, double* Ainv_out);
/* C (m x n) = A (m x k) %*% B (k x n) on the fp64 MFMA GEMM of the scan operands (v_mfma_f64_16x16x4_f64). */
int eagle_matmul(eagle_ctx* ctx, const double* A, const double* B, long m, long k, long n, double* C);
/* E/R/calculateMMt_sqrt_and_sqrtinv.R:15-47 in one call: EAGLE_SOFT_SENTINEL if MMt is not positive definite by
 * matrixcalc::is.positive.definite's rule (:15; eigenvalues below 1e-8 in magnitude count as 0); sqrt_out = U sqrt(L) U^T
 * (:25-27), invsqrt_out = chol2inv(chol(sqrt)) (:30), *trace_out = sum(diag(sqrt %*% invsqrt)), whose truncation the R code
 * compares with nrow(MMt) (:35-46; may be NULL). */
int eagle_mmt_sqrt_and_sqrtinv(eagle_ctx* ctx, const double* MMt, long n, double* sqrt_out, double* invsqrt_out, double* trace_out);

/* Optional shortcut (NOT one of the reference's .Call symbols; a maintainer who edits find_qtl.R may use it): the scan of
 * eagle_calculate_a_and_vara with W = S V S (n x n) and v = S a_hat (n) handed over ready-made.  Inside AM() neither needs an
 * n^3 product: dim_reduced_vara = varG I - C22 = varG^2 Ze P Ze with Ze = MMt^1/2 (E/R/calculate_reduced_vara.R:21-35),
 * inv_MMt_sqrt = Ze^-1, hence W = varG^2 P and v = varG P y, and .find_qtl holds P (E/R/find_qtl.R:9, calculateP.R:27-28).
 * Same outputs, sentinel-free (no availmemGb branch rules: those belong to the reference-shaped call). */
int eagle_scan_with_W(eagle_ctx* ctx, const char* f_name_ascii, const double* selected_loci, long n_selected, const double* W,
                      const double* v, double max_memory_in_Gbytes, const long dims[2], int quiet, double* a_out, double* vara_out);

/* ---------------------------------------------------------------------------------------------
 * 1d. The scan in the eigenbasis of MM^T (OPT-IN; not symbols of the reference -- a maintainer who edits find_qtl.R may use
 *     them; the reference-shaped eagle_calculate_a_and_vara above stays the drop-in).
 *     Per iteration the reference evaluates a_i = varG m_i^T P y and vara_i = varG^2 m_i^T P m_i (W = S V S = varG^2 P, see
 *     eagle_scan_with_W) with P = H^-1 - H^-1 X (X^T H^-1 X)^-1 X^T H^-1, H = varE I + varG K, K = the normalised MM^T of
 *     calcMMt.R:13 -- an n x n quadratic form per marker.  K does not change during an AM() run (only varE, varG, X do), so with
 *     K = U diag(lambda) U^T (emma.REMLE computes it anyway, E/R/emma_eigen_R_wo_Z.R:17) and Z = Mt U made ONCE,
 *     every scan is one streaming pass over Z: 8 n bytes and (p + 2) n multiply-adds per marker, HBM-bound.
 * ------------------------------------------------------------------------------------------- */
/* Once per AM() run: Z = Mt U (L x n fp64, 8 bytes per genotype, kept in HBM by the ctx) from the resident int8 image of
 * Mt.ascii (dims = (L, n)) and the eigenvectors U of K (n x n column-major, any order, the same order as lambda below). */
int eagle_spectral_prepare(eagle_ctx* ctx, const char* f_name_ascii, const long dims[2], const double* U, double max_memory_in_Gbytes);
/* Per iteration: lambda (n eigenvalues of K), UtX = U^T X (n x p column-major, p = columns of the fixed-effects design,
 * 1 <= p <= 31), Uty = U^T y (n), the variance components.  a_out, vara_out: L doubles, the values
 * eagle_calculate_a_and_vara returns for the S, V, a_hat that find_qtl.R:5-49 builds from the same K, X, y, varE, varG.
 * selected_loci: the reference's masking rule (element 0 NA: none). */
int eagle_spectral_scan(eagle_ctx* ctx, const double* lambda, const double* UtX, const double* Uty, long p, double varE, double varG,
                        const double* selected_loci, long n_selected, double* a_out, double* vara_out);
/* The same pass with the operands made by the caller: a_i = varG (z_i . Gy - q_i . c1), vara_i = varG^2 (sum_k z_ik^2 d_k -
 * q_i^T C q_i), q_i = z_i^T GX, z_i the row of the resident Z.  d, Gy: n; GX: n x p column-major (1 <= p <= 31); C: p x p
 * symmetric; c1: p.  eagle_spectral_scan is this call with d = 1/(varE + varG lambda), Gy = d o Uty, GX = d o UtX,
 * C = (UtX^T D UtX)^-1, c1 = C UtX^T D Uty.  For a model whose C and c1 hold terms that lambda and UtX alone do not give: the
 * repeated-measures design y = X b + Z g + e of am.AM(Zmat=), where Z is made from the scaled eigenvectors of D^1/2 K D^1/2 and
 * X^T H^-1 X carries the within-individual remainder.  Masking and errors as eagle_spectral_scan. */
int eagle_spectral_scan_weights(eagle_ctx* ctx, const double* d, const double* Gy, const double* GX, long p, const double* C, const double* c1,
                                double varG, const double* selected_loci, long n_selected, double* a_out, double* vara_out);
/* T traits over the Z of the last eagle_spectral_prepare, in as few passes over Z as the column groups allow (whole traits packed
 * into at most 128 MFMA columns: p[t] + 1 per trait plus one per trait for sum_k z_ik^2 d_t[k]; eagle_spectral_traits_passes).
 * UtX[t]: n x p[t] column-major (1 <= p[t] <= 31), Uty: n x T column-major, varE/varG: T each.  a_out, vara_out: L x T
 * column-major, the values T eagle_spectral_scan calls return (no selected_loci masking), or both NULL (then only the arg-max
 * crosses PCIe).  index_out: T 1-based arg-max indices of tsq = a^2/vara, first index of the maximum, NaN skipped (0 = every
 * tsq NaN); tsqmax_out: T values (may be NULL).  EAGLE_ERR_ARG with a message: no prepare, T < 1, p[t] outside 1..31,
 * varE + varG lambda <= 0, X^T H^-1 X not positive definite. */
int eagle_spectral_scan_traits(eagle_ctx* ctx, long T, const double* lambda, const double* const* UtX, const long* p, const double* Uty,
                               const double* varE, const double* varG, double* a_out, double* vara_out, long* index_out, double* tsqmax_out);
/* Passes over Z eagle_spectral_scan_traits makes for these p[0..T-1] (EAGLE_ERR_ARG for T < 1 or a p[t] outside 1..31). */
int eagle_spectral_traits_passes(long T, const long* p);
/* U^T m_j for k markers (0-based idx): the rows of the resident Z, n x k column-major -- the U^T X column a pick adds. */
int eagle_spectral_rows(eagle_ctx* ctx, const long* idx, long k, double* out);

/* ---------------------------------------------------------------------------------------------
 * 1d'. The exact per-marker mixed-model test (no counterpart in the reference, which reports the loci its multi-locus model picks):
 *     for every marker i the fit of  y = X beta + m_i gamma + g + e,  g ~ N(0, sg2 K), e ~ N(0, se2 I),  with delta = se2 / sg2
 *     RE-ESTIMATED for that marker, as GEMMA and FaST-LMM do -- not the score statistic a^2 / vara of eagle_spectral_scan, which keeps
 *     the null model's variance components (EMMAX / P3D).  csrc/eagle_lmm.hip, k_lmm_exact; restated in numpy by r_api.lmm_host.
 *
 *     Notation.  K = U diag(lambda) U^T is the kinship AM() uses; yt = U^T y, Xt = U^T X, X n x c WITH the intercept column,
 *     1 <= c <= 14; z = row i of the resident Z (U^T m_i); D = [Xt z], p = c + 1; B = [D yt], c + 2 <= 16 columns;
 *     w_k(delta) = 1 / (lambda_k + delta);  S_r(delta) = B^T W^r B for r = 1, 2, 3, with blocks A_r (p x p), b_r (p), y_r.
 *
 *     One evaluation at theta = ln delta, in this order:
 *       delta = e^theta; w_k, S_1, S_2, S_3 and s_r = sum_k w_k^r;
 *       the Cholesky factor of A_1, a pivot tested against LMM_PIVOT_REL times its diagonal entry of A_1;
 *       beta = A_1^-1 b_1;  R = y_1 - b_1^T beta  (= yt^T P yt), tested against LMM_PIVOT_REL y_1 like a pivot;
 *       Q = y_2 - 2 beta^T b_2 + beta^T A_2 beta  (= yt^T P^2 yt);
 *       C = y_3 - 2 beta^T b_3 + beta^T A_3 beta - u^T A_1^-1 u,  u = b_2 - A_2 beta  (= yt^T P^3 yt: with r = yt - D beta,
 *           r^T W^3 r - (D^T W^2 r)^T A_1^-1 (D^T W^2 r));
 *       REML:  m = n - p,  T = s_1 - tr(A_1^-1 A_2)  (= tr P),  T2 = s_2 - 2 tr(A_1^-1 A_3) + tr((A_1^-1 A_2)^2)  (= tr P^2);
 *       ML:    m = n,      T = s_1,                          T2 = s_2;
 *       l'(delta) = 1/2 [m Q / R - T],   l''(delta) = 1/2 [m (Q^2 / R^2 - 2 C / R) + T2];
 *       g(theta) = delta l',   g'(theta) = delta l' + delta^2 l''.
 *     The likelihoods these differentiate:  REML  l = 1/2 [(n - p)(log((n - p) / 2 pi) - 1 - log R) + sum log w - log det A_1],
 *     ML  l = 1/2 [n (log(n / 2 pi) - 1 - log R) + sum log w].  The log terms enter no g: they are formed once, for the reported l.
 *
 *     The iteration seeks the root of g.  theta starts at theta0 = ln delta of the null fit (X alone), clipped to [LMM_THETA_MIN,
 *     LMM_THETA_MAX] = [-10, 10] (emma.py's llim, ulim); lo = LMM_THETA_MIN and hi = LMM_THETA_MAX, neither evaluated yet.  Then:
 *       1. evaluate g, g' at theta.  g > 0: lo = theta, an evaluated point; g < 0: hi = theta, an evaluated point;
 *       2. g > 0 at theta = LMM_THETA_MAX: stop, code 4;  g < 0 at theta = LMM_THETA_MIN: stop, code 3  (a limit at which g still
 *          points outward is a boundary optimum);
 *       3. the proposal t: Newton's theta - g / g' when g' < 0, lo < t < hi and |t - theta| <= LMM_STEP_MAX; otherwise (lo + hi) / 2
 *          when the end on the other side of theta is an evaluated point (one of opposite sign exists); otherwise theta + sign(g)
 *          LMM_STEP_MAX clipped to the limit (g = 0: t = theta);
 *       4. |t - theta| <= tol: stop, code 0;  `iterations` = max_iter: stop, code 1;  else theta = t, iterations += 1, back to 1.
 *     So a call makes iterations + 1 evaluations and max_iter = 0 returns the values at theta0.  Every stop but code 2 reports the
 *     LAST EVALUATED theta:  gamma = beta_p,  sg2 = R / m,  se2 = delta sg2,  se = sqrt(sg2 (A_1^-1)_pp),  l(theta).
 *     This is the local optimum reached from the null fit, as GEMMA's Newton stage gives it -- NOT emma.REMLE's search over a grid of
 *     100 intervals, which compares every local optimum.
 *
 *     stat_out[5 o ..] = (gamma, se, delta, sg2 (vg), l), info_out[2 o ..] = (code, iterations) for output position o.  Codes:
 *     0 converged; 1 max_iter reached; 2 singular: a Cholesky pivot of A_1 was not above LMM_PIVOT_REL of its diagonal entry (a
 *     monomorphic marker, a marker in the span of X), or R was not above LMM_PIVOT_REL y_1, or g or g' was not finite -- the five
 *     statistics are NaN; 3 optimum at the lower limit; 4 optimum at the upper limit.
 *
 *     eagle_spectral_lmm runs on the Z of the last eagle_spectral_prepare.  lambda: n; UtX: n x c column-major; Uty: n; reml: 1 = REML,
 *     0 = ML.  idx == NULL: every marker, in order (nidx is not read); else idx holds nidx 0-based markers and the outputs are in list
 *     order.  A marker's result depends on its row of Z, the operands and theta0 alone: the same bits for all markers, for an index list
 *     and in any order.  Bit equality with the host restatement is not claimed.  The reduction over the n eigen-directions runs on
 *     v_mfma_f64_16x16x4_f64 (three instructions per four directions and evaluation), one wave per marker.  Argument errors
 *     (EAGLE_ERR_ARG with a message; decided before the context is used, with ctx == NULL their text is in eagle_open_error()): a NULL
 *     pointer, c outside [1, 14], reml outside {0, 1}, theta0 not finite, tol not in (0, 1), max_iter outside [0, 1000], nidx < 0;
 *     then: no context, a multi-device context (single device only), no eagle_spectral_prepare, n <= c + 2, a marker index out of
 *     range, lambda_k + e^-10 <= 0 or not finite, a non-finite entry of UtX or Uty.
 * ------------------------------------------------------------------------------------------- */
#define LMM_THETA_MIN (-10.0)
#define LMM_THETA_MAX 10.0
#define LMM_STEP_MAX 2.0        /* the longest step in theta = ln delta: delta changes by a factor of at most e^2 per evaluation */
#define LMM_PIVOT_REL 0x1p-40   /* a Cholesky pivot must exceed this fraction of its diagonal entry of A_1 */
int eagle_spectral_lmm(eagle_ctx* ctx, const double* lambda, const double* UtX, const double* Uty, int c, int reml, double theta0, double tol,
                       int max_iter, const long* idx, long nidx, double* stat_out, int32_t* info_out);

/* ---------------------------------------------------------------------------------------------
 * 1d''. Tests of marker SETS under the mixed model (no counterpart in the reference): is a gene, a window or a candidate region as a
 *     whole associated with the trait?  The burden test and SKAT (the sequence kernel association test, Wu et al. 2011) under the null
 *     model's variance components, as EMMAX-SKAT / famSKAT define them.  eagle_spectral_scan gives each marker's score a_i and vara_i =
 *     varG^2 m_i^T P m_i; a set needs the COVARIANCES varG^2 m_i^T P m_j of its markers, which this call forms from the resident Z.
 *     csrc/eagle_settest.hip, k_settest_gram; restated in numpy by r_api.settest_host; the p-values are host work (r_api.skat_pvalue).
 *
 *     Notation as sections 1d and 1d'.  K = U diag(lambda) U^T;  d_k = 1 / (varE + varG lambda_k);  Xt = U^T X (n x c, 1 <= c <= 14, the
 *     intercept column included);  yt = U^T y;  z_j = row j of the resident Z.
 *
 *     A set S has the markers j_1 .. j_m, 1 <= m <= SETTEST_MAX_MARKERS = 64, and a weight omega_1 .. omega_m per marker, finite and
 *     >= 0.  The sets arrive in CSR form: set_ptr[nsets + 1], set_idx[] (0-based markers), omega[].  A marker may be in many sets.
 *
 *     Per set, in this order:
 *       1. the augmented weighted Gram G = A^T diag(d) A of A = [z_j1 .. z_jm | Xt | yt] (n x (m + c + 1)), with the blocks G_zz, G_zx,
 *          G_zy, G_xx, G_xy; the reduction over the n eigen-directions runs on v_mfma_f64_16x16x4_f64;
 *       2. the Cholesky factor of G_xx, a pivot tested against LMM_PIVOT_REL times its diagonal entry of G_xx: a pivot not above it is
 *          an argument error of the whole call (X^T H^-1 X is not positive definite, as eagle_spectral_scan_traits reports it; G_xx is
 *          the same for every set).  Then B = G_xx^-1 [G_xz | G_xy];
 *       3. the scores s = varG (G_zy - G_zx B_y) and their covariance Phi = varG^2 (G_zz - G_zx B_z): the a, and the matrix whose
 *          diagonal is the vara, of eagle_spectral_scan for the same operands;
 *       4. the degenerate-marker rule: a marker with Phi_jj <= LMM_PIVOT_REL varG^2 (G_zz)_jj (a monomorphic marker, a marker in the
 *          span of X) gets s_j = 0, row and column j of Phi are set to exactly 0, and it is counted in n_degenerate;
 *       5. with W = diag(omega) and Aw = W Phi W:  Q = sum_j omega_j^2 s_j^2,  Ub = sum_j omega_j s_j,  Vb = omega^T Phi omega,
 *          c_r = tr(Aw^r) for r = 1 .. 4  (c_2 = |Aw|_F^2, c_3 = tr(Aw Aw^2), c_4 = |Aw^2|_F^2);
 *       6. Phi is written symmetric bit for bit: the mirror is a copy of the lower triangle.
 *
 *     stat_out[7 o ..] = (Q, Ub, Vb, c_1, c_2, c_3, c_4), info_out[2 o ..] = (code, m - n_degenerate) for set o.  Codes: 0 ok; 2 nothing
 *     left (Vb <= 0 or c_2 <= 0: every marker degenerate or of weight 0) -- the seven statistics are NaN.  score_out (one double per CSR
 *     entry: s_j) and cov_out (the sets packed one after another, m_s^2 doubles each, row-major: Phi) may each be NULL.
 *
 *     From these the host forms (r_api.SetTest):  burden  stat = Ub^2 / Vb ~ chi^2_1, beta = varG Ub / Vb (the beta_p3d convention);
 *     SKAT  p = P(sum_i lambda_i chi^2_1,i > Q), lambda = eig(Aw), by the modified moment matching of Liu et al. (2009) on c_1 .. c_4
 *     and, for small p, by a saddlepoint approximation on the eigenvalues of a second call's cov_out.
 *
 *     A set's result depends only on its rows of Z, its weights and the staged operands: the same bits for any order of the sets, for a
 *     set listed twice and for a second call (chunk r of 64 eigen-directions belongs to wave r mod 4, the four partial Grams are added in
 *     wave order).  Bit equality under a permutation of the markers WITHIN a set is not claimed; bit equality with the host restatement
 *     is not claimed either.  Not done: sets above 64 markers, SKAT-O's rho grid, re-estimating delta per set, case/control traits, a
 *     .bed route, more than one device.
 *
 *     eagle_spectral_settest runs on the Z of the last eagle_spectral_prepare.  lambda: n; UtX: n x c column-major; Uty: n.  Argument
 *     errors (EAGLE_ERR_ARG with a message) decided before the context is used -- with ctx == NULL their text is in eagle_open_error():
 *     a NULL pointer (score_out and cov_out excepted), c outside [1, 14], nsets < 0, varE or varG not finite, set_ptr not non-decreasing
 *     from 0, an empty set, a set above 64 markers, a negative or non-finite weight, a negative marker index; then: no context, a
 *     multi-device context (single device only), no eagle_spectral_prepare, n <= c + 1; then what needs the n and L of the resident Z: a
 *     marker index >= L, varE + varG lambda_k <= 0 or not finite, a non-finite entry of UtX or Uty.  nsets == 0 returns EAGLE_OK.
 *     (A context whose Z was prepared from a marker range holds the markers [first, first + L): an index outside it is out of range.)
 * ------------------------------------------------------------------------------------------- */
#define SETTEST_MAX_MARKERS 64
int eagle_spectral_settest(eagle_ctx* ctx, const double* lambda, const double* UtX, const double* Uty, int c, double varE, double varG,
                           long nsets, const long* set_ptr, const long* set_idx, const double* omega, double* stat_out, int32_t* info_out,
                           double* score_out, double* cov_out);

/* ---------------------------------------------------------------------------------------------
 * 1d'''. Saddlepoint p-values of the score test under the logistic mixed model (no counterpart in the reference, whose trait is
 *     quantitative): case/control association with a kinship term.  The model is GMMAT's (Chen et al. 2016),
 *            logit mu_i = x_i' alpha + b_i,   b ~ N(0, tau K),
 *     fitted once per trait on the host by penalised quasi-likelihood (eagleeverything_amd/glmm.py, null_fit), and the p-value of a
 *     marker's score is SAIGE's saddlepoint approximation (SPA; Dey et al. 2017, Zhou et al. 2018), which repairs the normal
 *     approximation where it fails: unbalanced case/control ratios and rare alleles.  This call is the per-marker part.
 *     glmm.spa_host is a numpy restatement of the rule below.
 *
 *     Operands, all of the null fit: mu (n, each in (0, 1)); resid = y - mu (n); X (n x c column-major fp64 as R holds it, the caller
 *     supplies the intercept column, 1 <= c <= 15); A = (X'DX)^-1 (c x c), D = diag(mu_i (1 - mu_i)), made once by the caller; vara
 *     (one V_m = m' P m per marker, what eagle_scan_with_W returns for W = P) or NULL for V = V*.  g_i in {0, 1, 2} is the image value
 *     plus one of line m of Mt.ascii; a missing call of the source is a heterozygote by now.  At the fixed point of the null fit
 *     y - mu = P Y and X'(y - mu) = 0, so the score does not depend on whether m is the image value or the allele count.
 *
 *     1. First pass.  s = X'D g, beta = A s, G~_i = g_i - x_i' beta;  T = sum g_i resid_i;  V* = sum D_i G~_i^2;  m = sum G~_i mu_i.
 *     2. Degenerate marker: V* <= 2^-40 sum D_i g_i^2, or a V that is not finite and positive (a monomorphic marker, a marker in the
 *        span of X): code 2, z and the four values of 6 are NaN, no evaluation.
 *     3. Scaling and screen.  z = T / sqrt(V), q = z sqrt(V*) = T sqrt(V* / V).  If |z| <= cutoff the marker ends here with code 4 and
 *        0 evaluations; SAIGE's cutoff is 2.
 *     4. The cumulant generating function of sum G~_i (y_i - mu_i), y_i independent Bernoulli(mu_i):
 *            K(t) = sum log(1 - mu_i + mu_i e^(t G~_i)) - t m,
 *            K'(t) = sum mu_i G~_i / ((1 - mu_i) e^(-t G~_i) + mu_i) - m,
 *            K''(t) = sum (1 - mu_i) mu_i G~_i^2 e^(-t G~_i) / ((1 - mu_i) e^(-t G~_i) + mu_i)^2.
 *        One evaluation is one pass over the individuals.  The centring by m is taken inside the sum, individual by individual, so
 *        nothing of first order cancels between two sums and nothing overflows: with a = t G~_i, nu = 1 - mu_i for a >= 0 and mu_i
 *        else, e = exp(-|a|), u = 1 - e, den = 1 - nu u the three terms of individual i are
 *            nu |a| + log1p(-nu u),     sign(a) D_i G~_i u / den,     D_i G~_i^2 e / den^2,
 *        one exp and one log1p, as section 1b''''iv evaluates its likelihood.  K'(0) = 0 and K''(0) = V* need no evaluation.
 *     5. Tails.  There are two, with targets +|q| (zeta_up) and -|q| (zeta_lo); the one on the side of T, the observed side, is
 *        taken first.  zeta_max = 500 / max_i |G~_i|.  A target is reachable when K'(+-zeta_max) passes it by more than 2^-40 |target| (a statistic AT the edge
 *        of its support is not reachable, whatever the last bit of the sums), which is the tail's first evaluation.  An unreachable observed-side target is code 3: all carriers are cases, the statistic sits at the edge of its
 *        support.  An unreachable opposite tail contributes no probability and sets + 256 (zeta = -+zeta_max, r* = -+infinity): the
 *        usual case for a rare allele.  For a reachable target solve K'(zeta) = target by Newton from zeta = 0 inside the bracket
 *        [0, +-zeta_max]: zeta <- zeta - (K' - target) / K''; bisect when the step leaves the bracket (or is not a number); evaluate
 *        there; the bracket is updated by the sign of K' - target; stop when |delta zeta| sqrt(V*) <= tol; at most max_iter evaluations
 *        per tail, the reachability one included, code 1 otherwise.  The first code that is not 0 ends the marker.
 *     6. Per-tail deviate at the root: w = sign(zeta) sqrt(2 (zeta target - K(zeta))), v = zeta sqrt(K''(zeta)), r* = w + ln(v / w) / w;
 *        where |zeta| sqrt(V*) < 10^-4, r* = target / sqrt(V*).
 *     7. Per-marker result.  stat_out[7 m ..] = (T, V*, z, zeta_up, r*_up, zeta_lo, r*_lo) and info_out[2 m ..] = (code, evaluations
 *        of both tails).  Codes: 0 both tails solved; 1 max_iter reached; 2 degenerate; 3 observed-side target unreachable; 4 below the
 *        cutoff; + 256 the opposite tail was unreachable.  The four values of 6 are NaN unless the code's low byte is 0.  The host makes
 *        p_spa = Phi(-r*_up) + Phi(r*_lo) (scipy.special.ndtr): only this way do far tails keep their precision.
 *
 *     On the device (k_glmm_spa, csrc/eagle_glmm.hip) one wave owns one marker, four to a workgroup, no barrier between waves and no
 *     atomics; X'D g is accumulated on v_mfma_f64_16x16x4_f64 with c padded to 16; a lane owns one individual per chunk of 64 and
 *     recomputes G~_i at every evaluation (c FMAs) rather than holding it; wave reductions finish an evaluation.  X, mu, D and resid
 *     are staged once per call as padded images and the genotype is read from the int8 row.  A marker's result depends on its row
 *     and the per-call operands alone, so it does not depend on how markers fall into row windows or workgroups.
 *
 *     What is not claimed.  Agreement with the GMMAT, SAIGE or SPAtest programs is neither claimed nor tested, because none is
 *     available: the tests hold the roots and deviates to 40-digit solutions of the same equations and the rule itself to full
 *     enumeration of the 2^n outcomes at n = 18.  Bit equality with the numpy restatement is not claimed either: exp, log1p and the
 *     order of the sums are not fixed by IEEE 754.  Not done: a .bed route, repeated measures, several devices, SAIGE's variance-ratio
 *     shortcut (V here is exact), the fast SPA partial-normal split for non-carriers, sex chromosomes.
 *
 *     The file is read as eagle_logistic reads it: the resident image where it lies, else row windows from the sidecar, the text or a
 *     VIEW alias's source; with a VIEW alias the operands have one entry per kept individual.  Single device: a multi-device context
 *     works on its first device.  Argument errors (EAGLE_ERR_ARG: a NULL pointer (vara excepted), dims <= 0, n > 2^30 - 1, c outside
 *     [1, 15], a mu outside (0, 1) or not finite, a non-finite X, resid or A entry, cutoff < 0 or NaN, tol not in (0, 1), max_iter
 *     outside [1, 1000]) are decided before the context is used; with ctx == NULL their text is in eagle_open_error().
 * ------------------------------------------------------------------------------------------- */
int eagle_glmm_spa(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const double* mu, const double* resid, const double* X,
                   int c, const double* A, const double* vara_or_NULL, double cutoff, double tol, int max_iter, double max_memory_in_Gbytes,
                   double* stat_out, int32_t* info_out);

/* Replaces the R tail of .find_qtl:  tsq <- a^2/vara ; which(tsq == max(tsq, na.rm=TRUE))[1]
 *                                                E/R/find_qtl.R:71-83
 * Evaluated on the device on the a / vara of the LAST eagle_calculate_a_and_vara call of this ctx (still in
 * HBM).  index_out is 1-based (0 if every tsq is NaN).  In digit-slice mode the arrays were certified inside the scan call
 * (eagle_dev_scan_certify below: every marker that could be the arg-max carries its fp64-kernel value), so the index is
 * the one scan mode 0 returns and the one R's own which(tsq == max(tsq))[1] finds on the returned a / vara.
 * n_near_ties is informational: markers whose tsq is within a relative 1e-9 of the maximum (1 = unambiguous). */
int eagle_last_scan_argmax(eagle_ctx* ctx, long* index_out, double* tsqmax_out, long* n_near_ties);

/* MMt/max(MMt) + 0.95 I  (E/R/calcMMt.R:13) of the LAST eagle_calculateMMt result, on the device. */
int eagle_last_mmt_normalised(eagle_ctx* ctx, double* MMt_norm_out, double* max_out);

/* ---------------------------------------------------------------------------------------------
 * 2. Device-resident entry points (all pointers are HBM addresses on ctx's device; `stream` is a
 *    hipStream_t passed as void*, NULL = default stream).  Used by the marker-sharded multi-GPU driver
 *    and by bench.py, which keep genotype shards resident in HBM between calls.
 *
 *    Layout contract for genotype matrices (int8, values {-1,0,1}):
 *      Mt8: marker-major  [L_pad][ld]  ld >= n, ld % 256 == 0, L_pad % 256 == 0, padding bytes ZERO
 *      M8 : individual-major [n_pad][ld] ld >= L, ld % 256 == 0, n_pad % 256 == 0, padding bytes ZERO
 *    fp64 square operands: row-major [np][np], np = eagle_pad(n) (next multiple of 256), padding ZERO.
 * ------------------------------------------------------------------------------------------- */
long eagle_pad(long x);

/* Lines [row0,row0+nrows) x characters [col0,col0+ncols) of a no-space ASCII genotype file (M.ascii / Mt.ascii,
 * as ReadBlock reads them, E/src/ReadBlock.cpp:47-58) -> int8 at dst[r*ld + c] in HBM.  Fixed-width files are
 * pread() into pinned memory by `threads` workers, double-buffered against the H2D copy and the decode kernel;
 * max_mem_gb bounds the pinned staging.  A marker shard is a row range of Mt.ascii or a column window of M.ascii. */
int eagle_dev_load_ascii(eagle_ctx* ctx, const char* path, long row0, long nrows, long col0, long ncols, int8_t* dst,
                         long ld, double max_mem_gb, int threads);

/* raw text tile (rows of `line_stride` bytes, first `cols` bytes used) -> int8 (value char-'0'-1);
 * *bad_chars_dev (device int, caller-zeroed) counts bytes outside '0'..'2'. */
int eagle_dev_decode_ascii(eagle_ctx* ctx, const uint8_t* raw, long rows, long cols, long line_stride,
                           int8_t* out, long ld_out, int* bad_chars_dev, void* stream);
int eagle_dev_transpose_i8(eagle_ctx* ctx, const int8_t* in, long rows, long cols, long ld_in, int8_t* out,
                           long ld_out, void* stream);
/* out[r*ld_out + j] = src[r*ld_src + map[j] - base] for j < ncols, 0 for ncols <= j < ld_out (r < rows): the column subset of a
 * resident Mt image behind the VIEW aliases of eagle_reshape_m.  map: device int32, increasing; ld_src, ld_out % 4 == 0; every
 * map[j] - base in [0, ld_src). */
int eagle_dev_gather_cols_i8(eagle_ctx* ctx, const int8_t* src, long ld_src, const int32_t* map, long base, long rows, long ncols,
                             int8_t* out, long ld_out, void* stream);
/* How many windows of VIEW aliases this context (all its sub-contexts) has loaded, by source: from the source's resident HBM
 * image (k_gather_cols_i8 / row copies), its 2-bit sidecar, its fixed-width text, or the general line scanner. */
#define EAGLE_VIEW_RESIDENT 0
#define EAGLE_VIEW_SIDECAR 1
#define EAGLE_VIEW_TEXT 2
#define EAGLE_VIEW_SCANNER 3
int eagle_view_load_counts(eagle_ctx* ctx, long counts_out[4]);
int eagle_dev_i8_to_f64_colmajor(eagle_ctx* ctx, const int8_t* in, long rows, long cols, long ld_in,
                                 double* out_colmajor, void* stream);

/* C32[np][np] (int32, row-major, caller-zeroed) += M8 * M8^T over the marker columns [0, L_pad).
 * Upper-triangular tiles only; exact integers, order independent (integer atomics).  The products run on
 * v_mfma_scale_f32_32x32x64_f8f6f4 with both operands fp4 (-1, 0, +1 are exact e2m1 numbers; fp32 partial sums of a K
 * split are exact integers): eagle_dev_mmt_accumulate packs the int8 image into a ctx-owned fp4 buffer first,
 * eagle_dev_mmt_accumulate_f4 takes an image the caller made with eagle_dev_pack_fp4 (M4[n_pad][ld4 bytes], two
 * genotypes per byte).  n_pad % 256 == 0, L_pad % 256 == 0. */
int eagle_dev_mmt_accumulate(eagle_ctx* ctx, const int8_t* M8, long n_pad, long L_pad, long ld, int32_t* C32,
                             void* stream);
int eagle_dev_mmt_accumulate_f4(eagle_ctx* ctx, const void* M4, long n_pad, long L_pad, long ld4, int32_t* C32, void* stream);
/* C32 -= sum over the listed marker columns of m_c m_c^T  (the selected_loci masking of
 * calculateMMt_rcpp.cpp:88-92 applied as an exact rank-k downdate). cols_dev: device array of long. */
int eagle_dev_mmt_downdate(eagle_ctx* ctx, const int8_t* M8, long n_pad, long ld, const long* cols_dev,
                           long ncols, int32_t* C32, void* stream);
/* Mirror the upper triangle, convert to fp64 (n x n, leading dimension ld_out, symmetric so layout-free),
 * and write max(MMt) to *max_dev (device double). */
int eagle_dev_mmt_finish(eagle_ctx* ctx, const int32_t* C32, long n, long n_pad, double* MMt, long ld_out,
                         double* max_dev, void* stream);
int eagle_dev_mmt_normalise(eagle_ctx* ctx, double* MMt, long n, long ld, const double* max_dev, void* stream);

/* Scan operands from the reference's arguments (n_pad x n_pad row-major images of the COLUMN-major
 * inputs, i.e. Sa = S^T, Va = V^T):  v = S a_hat ; Wu = upper-triangular fold of W = S (V S) with
 * Wu[j][k] = W[j][k] + W[k][j] (j<k), W[k][k] (j=k), 0 (j>k), so that m^T W m = sum_k m_k sum_{j<=k} m_j Wu[j][k].
 * tmp: n_pad*n_pad doubles of scratch. */
int eagle_dev_scan_operands(eagle_ctx* ctx, const double* Sa, const double* Va, const double* ahat, long n,
                            long n_pad, double* v_out, double* Wu_out, double* tmp, void* stream);
/* Lifetime: when the int8 engine formed W (eagle_last_w_info: int8 = 1) the context remembers Sa, Va, Wu_out and tmp -- the scan
 * that follows re-evaluates single markers from m^T (S (V (S m))) and may redo the products in fp64.  All four must stay allocated and
 * unchanged until that scan has finished (or the next eagle_dev_scan_operands* call on this context).
 *
 * Keeping S between calls.  Everything the int8 engine computes from S alone (its digit image and row statistics, S 1 and S^T 1:
 * one full pass over S and a half, every call) can stay in the context's workspace.  The library cannot see an image rewritten in
 * place, so this is opt-in: eagle_dev_declare_s(ctx, Sa, n, n_pad) is the caller's promise that the image at Sa IS S and stays
 * bit for bit as it is until the next eagle_dev_declare_s or eagle_dev_forget_s on this context.  Calls of eagle_dev_scan_operands
 * with exactly that (Sa, n, n_pad), on one stream, then compute the S part once; every result is bit for bit what an undeclared call
 * returns.  A new S in the same buffer: write it, then declare again (every declaration is a new S).  Before freeing the buffer:
 * eagle_dev_forget_s.  Without a declaration nothing is kept.  eagle_drop_cache, a workspace that had to grow, and a call the engine
 * declined drop what was kept (the declaration stands: the next call computes it anew).  eagle_dev_scan_operands_rows and the fp64
 * products take no part in this.  eagle_w8_keep_stats: calls that found / had to compute the S part (summed over the devices). */
int eagle_dev_declare_s(eagle_ctx* ctx, const double* Sa, long n, long n_pad);
int eagle_dev_forget_s(eagle_ctx* ctx);
int eagle_w8_keep_stats(eagle_ctx* ctx, long* hits, long* misses);
/* Marker-sharded runs share the n^3 part: each rank computes v and the rows [row0, row1) (multiples of 128) of the W^T
 * image (full rows), the row blocks are all-gathered, and eagle_dev_fold_upper folds the complete image in place. */
int eagle_dev_scan_operands_rows(eagle_ctx* ctx, const double* Sa, const double* Va, const double* ahat, long n, long n_pad,
                                 long row0, long row1, double* v_out, double* Wt_out, double* tmp, void* stream);
int eagle_dev_fold_upper(eagle_ctx* ctx, double* W, long n_pad, void* stream);
/* a_i = scale * sum_j Mt8[i][j] v[j] for L_pad rows: calculate_a_and_vara_rcpp.cpp:91, calculate_reduced_a_rcpp.cpp:83-84.
 * HBM-bound pass on the int8 MFMA (v as 8 exact base-256 digit rows, int32 sums, one rounding per output).
 * L_pad % 16 == 0, n_pad % 256 == 0, ld % 16 == 0. */
int eagle_dev_gemv_i8(eagle_ctx* ctx, const int8_t* Mt8, long L_pad, long n_pad, long ld, const double* v,
                      double scale, double* out, void* stream);
/* vara_i = m_i^T W m_i for L_pad rows (calculate_a_and_vara_rcpp.cpp:103-112), fp64 MFMA kernel. */
int eagle_dev_vara_f64(eagle_ctx* ctx, const int8_t* Mt8, long L_pad, long n_pad, long ld, const double* Wu,
                       double* vara_out, void* stream);
/* Same result from int8 digit slices of the off-diagonal part of Wu on the int8 MFMA (exact integer partial sums)
 * plus the fp64 diagonal term.  nslices: 0 = automatic (see eagle_set_scan_slices), 1..8 = fixed.
 * ws: workspace, eagle_vara_i8_workspace_bytes(n_pad, L_pad, nslices) bytes; its first 48 bytes are written by the
 * device as { double max|offdiag|; int32 S_used; int32 pad; double bound; double sum|diag|; double R = sum_{j<k} Wu_jk }.
 * err_bound_dev (device double, may be NULL): the absolute error bound n_pad^2 * 2^(e+1-8S) of every vara_i. */
int64_t eagle_vara_i8_workspace_bytes(long n_pad, long L_pad, int nslices);
/* The same in two phases, so that one pass over the genotype bytes serves both a = Mt8 v (if v != NULL; written to
 * a_out) and the diagonal term, and so that the MFMA kernel can be timed on its own:
 *   prepare: max |off-diagonal|, slice count, diagonal vector, fused genotype pass, digit slices;
 *   mfma   : k_vara_i8 over all (marker tile, slice) workers + the S-term finish into vara_out. */
int eagle_dev_vara_i8_prepare(eagle_ctx* ctx, const int8_t* Mt8, long L_pad, long n_pad, long ld, const double* Wu,
                              int nslices, void* ws, const double* v, double* a_out, void* stream);
int eagle_dev_vara_i8_mfma(eagle_ctx* ctx, const int8_t* Mt8, long L_pad, long n_pad, long ld, int nslices, void* ws,
                           double* vara_out, double* err_bound_dev, void* stream);
/* The genotype pass of prepare from a 2-bit image.  Genotypes are {-1, 0, +1} and the same bytes in every scan of a run, and the pass
 * sits on the HBM stream: eagle_dev_pack_2bit makes, once, the image Mt2 of an int8 image -- ld / 4 bytes per marker, the codes m & 3
 * laid out so that one 16-byte load is a lane's MFMA fragments of four 64-column steps (csrc/eagle_kernels.hip) -- and
 * eagle_dev_vara_i8_prepare_packed is eagle_dev_vara_i8_prepare reading it (ld is the int8 image's): the fragments decode to the int8
 * image's bytes and the integer sums are the same, so a, the diagonal term and m^T rho come out bit for bit.  L_pad % 16 == 0,
 * n_pad % 256 == 0, ld % 256 == 0.  A value outside {-1, 0, +1} is not representable (its low two bits are kept).
 * eagle_dev_unpack_2bit: the int8 image back through the decode of the pass. */
int eagle_dev_pack_2bit(eagle_ctx* ctx, const int8_t* Mt8, long L_pad, long n_pad, long ld, void* Mt2, void* stream);
int eagle_dev_unpack_2bit(eagle_ctx* ctx, const void* Mt2, long L_pad, long n_pad, long ld, int8_t* Mt8, void* stream);
int eagle_dev_vara_i8_prepare_packed(eagle_ctx* ctx, const void* Mt2, long L_pad, long n_pad, long ld, const double* Wu,
                                     int nslices, void* ws, const double* v, double* a_out, void* stream);
/* Re-centred markers for the digit-slice kernel: Mt8s[i][j] = Mt8[i][j] - c_i for the n real individuals (padding stays
 * zero), c_i in {-1,0,+1} = the majority genotype of marker i, cshift[i] = c_i.  eagle_dev_vara_i8_mfma_shifted runs
 * the MFMA kernel on Mt8s (rare-variant markers become sparse rows, so their truncation error bound
 * (sum_j |m'_ij|)^2 / 2 * 2^(e+1-8S) shrinks with their own diagonal term) and adds c_i m_i^T rho - c_i^2 R in fp64;
 * prepare (always on the ORIGINAL image) has left rho, R and m^T rho in the workspace.
 * l1norm (may be NULL; 2 * L_pad int32): l1norm[2i] = sum_j |Mt8s[i][j]|, l1norm[2i+1] = sum_j Mt8s[i][j]^2, which
 * eagle_dev_scan_certify turns into marker i's error bound. */
int eagle_dev_marker_shift(eagle_ctx* ctx, const int8_t* Mt8, long L_pad, long n, long n_pad, long ld, int8_t* Mt8s,
                           int8_t* cshift, int32_t* l1norm, void* stream);
int eagle_dev_vara_i8_mfma_shifted(eagle_ctx* ctx, const int8_t* Mt8s, const int8_t* cshift, long L_pad, long n_pad, long ld,
                                   int nslices, void* ws, double* vara_out, double* err_bound_dev, void* stream);
/* Between eagle_dev_vara_i8_mfma_shifted and the certification (same image, cshift, l1norm, workspace), automatic digit count only:
 * when the scan ran on one digit fewer than cut (spectral bound, eagle_set_scan_budget), every marker whose own bound
 * min(specH q2_i, l1_i^2/2 * 128.5 u) exceeds 1.8 x budget of |vara_i| is given the dropped digit back: its rows are gathered, the
 * vara kernel runs once more on them with the last digit slice alone, and vara_i becomes, bit for bit, the value a scan on all the
 * cut digits gives that marker (the certificate then uses the rounding bound of that digit count for it).  Up to min(65,536, L_pad)
 * markers per call; more: nobody is extended and the certificate decides (fp64 fallback of the block).  Nothing runs when no marker
 * qualifies.  A call that skips this step is still certified correctly -- its flagged markers go to the fp64 kernel instead. */
int eagle_dev_vara_i8_extend(eagle_ctx* ctx, const int8_t* Mt8s, const int8_t* cshift, const int32_t* l1norm, long L, long L_pad, long n_pad,
                             long ld, int nslices, void* ws, double* vara, void* stream);
int eagle_dev_vara_i8(eagle_ctx* ctx, const int8_t* Mt8, long L_pad, long n_pad, long ld, const double* Wu,
                      int nslices, void* ws, double* vara_out, double* err_bound_dev, void* stream);
/* Certification of a digit-slice scan (after eagle_dev_vara_i8_mfma_shifted, before the arg-max), all on the device:
 * every vara_i carries the a-posteriori bound b_i = l1_i^2 / 2 * 2^(e+1-8S) (stochastic rounding: 8.355 q2_i 2^(e+1-8S)) + fp64
 * rounding terms; markers with
 * b_i > 1e-7 |vara_i|, and every marker that the bounds cannot exclude from being the arg-max of tsq = a^2 / vara
 * (a_i^2 / (vara_i - b_i) >= max_j a_j^2 / (vara_j + b_j)), are re-evaluated by the fp64 MFMA kernel on the ORIGINAL image
 * Mt8 -- bitwise the value eagle_dev_vara_f64 gives that marker -- and written back into vara.  The arg-max of tsq over the
 * certified arrays is then the arg-max of the fp64 scan (find_qtl.R:71-83 selects the same marker in either mode).
 * L = real markers of the block (rows beyond it are padding), L_pad / nslices / vara_ws as passed to prepare + mfma.
 * cert_ws: eagle_scan_certify_workspace_bytes(n_pad) bytes; its head is an eagle_cert_info the host may copy back.  If more
 * than 2048 markers qualify (degenerate operands) the whole block is redone in fp64 (overflow = 1).
 * Round 4: over_tight = markers whose bound exceeds 1.8 x the budget in force; with the tight budget (1e-7) in force and more than 512
 * of them (structured populations: quadratic forms that cancel against their diagonal term) the certificate enforces 1.8 x the default
 * budget (5e-7) instead -- `flagged` counts against the threshold that was enforced. */
typedef struct { double lower_bound; int32_t reevaluated; int32_t overflow; int32_t flagged; int32_t over_tight; } eagle_cert_info;
int64_t eagle_scan_certify_workspace_bytes(long n_pad);
int eagle_dev_scan_certify(eagle_ctx* ctx, const int8_t* Mt8, long L, long L_pad, long n_pad, long ld, const int8_t* cshift,
                           const int32_t* l1norm, int nslices, void* vara_ws, const double* Wu, const double* a, double* vara,
                           void* cert_ws, void* stream);
/* The same in two phases, for scans whose markers are spread over several devices / ranks: _lb leaves the lower bound of
 * this block's maximum tsq in cert_ws (eagle_cert_info.lower_bound); the caller takes the maximum over all blocks and hands
 * it to _apply as lb_override (NaN: the block's own), so that every block selects exactly the candidates a single scan of
 * all markers would. */
int eagle_dev_scan_certify_lb(eagle_ctx* ctx, long L, long L_pad, long n_pad, const int8_t* cshift, const int32_t* l1norm, int nslices,
                              void* vara_ws, const double* a, const double* vara, void* cert_ws, void* stream);
int eagle_dev_scan_certify_apply(eagle_ctx* ctx, const int8_t* Mt8, long L, long L_pad, long n_pad, long ld, const int8_t* cshift,
                                 const int32_t* l1norm, int nslices, void* vara_ws, const double* Wu, const double* a, double* vara,
                                 void* cert_ws, double lb_override, void* stream);
/* Certification counters of the LAST eagle_calculate_a_and_vara call of this ctx in digit-slice mode (summed over the
 * marker blocks of a streamed file): markers re-evaluated in fp64, of which flagged by their own error bound, and
 * whether a block fell back to the fp64 kernel entirely. */
int eagle_last_scan_certificate(eagle_ctx* ctx, long* n_reevaluated, long* n_flagged, int* fell_back);
/* Digit slices of the LAST eagle_calculate_a_and_vara call in digit-slice mode: used by the scan, cut from W (the same, or one more
 * when the spectral bound took the last one off), and that bound (|error_i| <= spectral_bound * sum_j m'_ij^2; 0 = not in use). */
int eagle_last_scan_digits(eagle_ctx* ctx, int* digits_used, int* digits_cut, double* spectral_bound);
/* Round 4.  The budget IN FORCE for the last digit-slice scan (what its certificate enforced per marker is 1.8 x this), the level of the
 * spectral bound that took the last digit off (0: none, 1, 2) and the error bound of W itself when the int8 engine formed it (0: fp64
 * products).  A context whose budget was never set tries 1e-7 first and falls back to 5e-7: the tight budget is in force whenever
 * the digits that run anyway certify a marker with q2 = n_pad to it (worst-case bound, or the spectral bound at level 1 / 2);
 * eagle_set_scan_budget(b) makes b the only budget, eagle_set_scan_budget(0) restores the default policy. */
int eagle_last_scan_budget(eagle_ctx* ctx, double* budget_used, int* bound_level, double* w_error_bound);
/* What the certificate of the last digit-slice scan ENFORCED per marker (bound <= 1.8 x budget_enforced x |vara_i|, else fp64): the
 * budget in force, or the default behind a tight one when more than 512 markers of the whole scan (all blocks, all devices) missed the
 * tight threshold (n_over_tight; see eagle_cert_info). */
int eagle_last_scan_enforced(eagle_ctx* ctx, double* budget_enforced, long* n_over_tight);
/* Round 4.  The first eagle_calculate_a_and_vara of a context allocates its device arena (four n x n fp64 images + the digit-slice and
 * certification workspaces: 100 GB at 50,000 individuals, 3-6 s of hipMalloc).  This call starts that allocation on a background
 * thread and returns at once; the scan collects it.  eagle_calculateMMt calls it by itself (AM() calls calcMMt once and then works
 * on the host for seconds); EAGLE_HIP_ARENA_GB=<GB> does the same at eagle_open.  dims as R has them: n individuals, L markers. */
int eagle_prepare_scan(eagle_ctx* ctx, long n, long L);
/* Out-of-core bookkeeping of the LAST call of this ctx that streamed its file through HBM in marker chunks (a file larger than
 * free HBM or than EAGLE_HIP_MAX_RESIDENT_GB; the lead device's share in a multi-device context): what SURVEY 8(d) asks to be
 * reported for the streamed configurations.  The loader of chunk k+1 (pread -> pinned -> H2D -> decode / 2-bit unpack) runs
 * under the kernels of chunk k.  Fraction of the load time hidden = 1 - starved_s / (load_s - load_first_s). */
typedef struct eagle_stream_stats {
    long chunks;         /* marker chunks */
    long file_bytes;     /* bytes read from the genotype file (text, or its 2-bit sidecar) */
    double pread_s;      /* host seconds inside the parallel preads (file_bytes / pread_s = storage rate) */
    double load_s;       /* host seconds in the chunk loaders (read + H2D + decode, synchronised per chunk) */
    double wait_s;       /* host seconds waiting for a free chunk buffer (kernels of chunk k-2 still running) */
    double kernel_s;     /* device seconds of the chunks' kernels (HIP events on the compute stream) */
    double wall_s;       /* first load to last kernel (includes whatever the compute stream had queued before chunk 0, e.g. W = S V S) */
    double load_first_s; /* the first chunk's load: nothing of this call's chunk kernels to hide under */
    double starved_s;    /* device seconds the compute stream sat idle between chunks because the next one was not loaded yet */
} eagle_stream_stats;
int eagle_last_stream_stats(eagle_ctx* ctx, eagle_stream_stats* out);
/* Where the LAST eagle_calculate_a_and_vara / eagle_scan_with_W call spent its time on device `device_index` of the context
 * (0 = the lead, which works on the calling thread): the accounting between the device-resident step bench.py times and what
 * the .Call-shaped entry point costs (E/R/calculate_a_and_vara.R:20-31 is the caller).  The *_ms fields are HIP-event intervals
 * on that device's compute stream, summed over the marker blocks of a streamed file. */
typedef struct eagle_scan_timing {
    double call_wall_s;   /* the whole call on the calling thread (argument checks, all devices, joins) */
    double device_wall_s; /* this device's worker: resident lookup / file load, uploads, kernels, results back */
    double host_setup_s;  /* of it: host seconds until the operand uploads were enqueued (resident lookup or file load, arena,
                             staging of V, a_hat -- and S when it is not the cached one -- out of pageable memory) */
    double upload_ms;     /* stream time from the first upload to the last (V, a_hat, S on a cache miss) */
    double w_ms;          /* v = S a_hat, W = S (V S): symmetry check, two products, fold (+ all-gather of W's rows) */
    double load_wait_ms;  /* streamed files: compute stream waiting for a marker block to be loaded */
    double prepare_ms;    /* digits of W, rho, ONE genotype pass (a = Mt v, diagonal term of vara) */
    double vara_ms;       /* the vara kernel (int8 digit slices + finish, or the fp64 kernel) */
    double certify_ms;    /* error bounds, candidate selection, fp64 re-evaluation */
    double d2h_ms;        /* row masking + a, vara back into the caller's arrays */
    long blocks;          /* marker blocks (1 = resident) */
    long markers;         /* markers of this device's shard */
} eagle_scan_timing;
int eagle_last_scan_timing(eagle_ctx* ctx, int device_index, eagle_scan_timing* out);
/* eagle_calculate_a_and_vara keeps the last call's S = inv_MMt_sqrt on the device (MMt^-1/2 is the same matrix in every find_qtl
 * call of an AM() run; n_pad <= 16,384, 2 x 8 n_pad^2 bytes): the next call starts its n^3 products on that copy and meanwhile
 * uploads the caller's matrix and compares the two bit for bit; a difference starts the products over with the new matrix, so the
 * result never depends on the cache.  hits: calls whose S was the cached one (its PCIe upload hidden under the product);
 * misses: calls that started over.  EAGLE_HIP_NO_SCACHE=1 disables the mechanism. */
int eagle_scan_operand_cache_stats(eagle_ctx* ctx, long* hits, long* misses);
/* The same quadratic form on the block-scaled matrix path (v_mfma_scale_f32_32x32x64_f8f6f4): genotypes as fp4, balanced
 * base-33 digits of Wu as fp6 (every integer in [-16,16] is an e2m3 number / 8), exact fp32 sums, twice the MAC rate of
 * the int8 instruction.  Mt4: [L_pad][n_pad/2] bytes made once per genotype matrix by eagle_dev_pack_fp4 (two genotypes
 * per byte).  nslices: 0 = automatic (same 1e-7 worst-case criterion), 1..12 = fixed; absolute error bound n_pad^2 * 2^(e-5S).
 * The workspace head has the layout of the int8 one ({max|offdiag|; S; f; bound; sum|diag|}). */
int64_t eagle_vara_f6_workspace_bytes(long n_pad, long L_pad, int nslices);
int eagle_dev_pack_fp4(eagle_ctx* ctx, const int8_t* Mt8, long L_pad, long n_pad, long ld, void* Mt4, void* stream);
/* The operand image of eagle_dev_mmt_accumulate_f4 straight from the MARKER-major genotypes, in one pass: M4[n_pad][ld4 bytes],
 * byte b of row j = markers 2b (low nibble) and 2b+1 (high nibble) of individual j as e2m1 codes, from Mt8[L_pad][ld].  The same
 * bytes as eagle_dev_transpose_i8 followed by eagle_dev_pack_fp4, without the individual-major int8 image in between.
 * L_pad % 256 == 0, n_pad % 128 == 0, ld % 16 == 0, ld4 % 16 == 0, ld4 >= L_pad / 2. */
int eagle_dev_transpose_pack_fp4(eagle_ctx* ctx, const int8_t* Mt8, long L_pad, long n_pad, long ld, void* M4, long ld4, void* stream);
int eagle_dev_vara_f6_prepare(eagle_ctx* ctx, const int8_t* Mt8, long L_pad, long n_pad, long ld, const double* Wu,
                              int nslices, void* ws, const double* v, double* a_out, void* stream);
int eagle_dev_vara_f6_mfma(eagle_ctx* ctx, const int8_t* Mt8, const void* Mt4, long L_pad, long n_pad, long ld, int nslices,
                           void* ws, double* vara_out, double* err_bound_dev, void* stream);
/* The spectral scan (section 1d) on device-resident data: Z[L_pad][n_pad] = Mt8 * Ur with Ur = U row-major [n_pad][n_pad]
 * (Ur[j][k] = U[j][k], zero padded); one pass over Z: lin[L_pad][NC] = Z G and quad[i] = sum_k Z_ik^2 d_k with G [n_pad][NC]
 * row-major, NC = 16 or 32 (column 0 = d o U^T y, columns 1..p = d o U^T X, the rest zero); the finish:
 * a_i = varG (lin_i0 - q_i . c1), vara_i = varG^2 (quad_i - q_i^T C q_i), q_i = lin_i[1..p], C p x p row-major, c1 p. */
int eagle_dev_spectral_zbuild(eagle_ctx* ctx, const int8_t* Mt8, long L_pad, long n_pad, long ld, const double* Ur, double* Z, void* stream);
/* The same Z from S exact int8 digit slices of U on the int8 MFMA (the tile engine of the digit-slice scan, dense K loop, store
 * epilogue): |Z_ik - (Mt U)_ik| <= (sum_j |m_ij|) 2^(e+1-8S), max|U| < 2^e <= 1.  ws: eagle_spectral_zbuild_i8_workspace_bytes bytes.
 * eagle_spectral_prepare uses S = 6 (error <= n 2^-47) unless eagle_set_scan_mode(ctx, 0) asks for the fp64 form. */
int64_t eagle_spectral_zbuild_i8_workspace_bytes(long n_pad, int nslices);
int eagle_dev_spectral_zbuild_i8(eagle_ctx* ctx, const int8_t* Mt8, long L_pad, long n_pad, long ld, const double* Ur, double* Z, void* ws,
                                 int nslices, void* stream);
int eagle_dev_spectral_pass(eagle_ctx* ctx, const double* Z, long L_pad, long n_pad, const double* G, int NC, const double* d, double* lin,
                            double* quad, void* stream);
/* The pass of eagle_spectral_scan_traits for one column group: out[L_pad][16 nt] = Z G with the A operand z_i in the first ntl
 * tiles of 16 columns and z_i o z_i in the rest (2 <= nt <= 8, 1 <= ntl < nt); G [n_pad][16 nt] row-major. */
int eagle_dev_spectral_pass_traits(eagle_ctx* ctx, const double* Z, long L_pad, long n_pad, const double* G, int nt, int ntl, double* out,
                                   void* stream);
int eagle_dev_spectral_finish(eagle_ctx* ctx, const double* lin, int NC, const double* quad, long L, long p, const double* Cm, const double* c1,
                              double varG, double* a, double* vara, void* stream);
/* zero a[i], vara[i] at the listed rows (row masking of calculate_a_and_vara_rcpp.cpp:79-84: a zeroed
 * marker row yields exactly a = 0, vara = 0). rows_dev: device array of long, entries outside [0,L) ignored. */
int eagle_dev_zero_rows(eagle_ctx* ctx, double* a, double* vara, long L, const long* rows_dev, long nrows,
                        long row_offset, void* stream);
/* tsq = a^2/vara, first index of the maximum ignoring NaN (find_qtl.R:71-83).
 * best_dev: device struct {double tsqmax; long index0; long near_ties;} index0 = -1 if all NaN.
 * tsq_out may be NULL. block_scratch: 3*1024 doubles. */
typedef struct { double tsqmax; long index0; long near_ties; } eagle_best;
int eagle_dev_tsq_argmax(eagle_ctx* ctx, const double* a, const double* vara, long L, double* tsq_out,
                         eagle_best* best_dev, double* block_scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EAGLE_HIP_H */
