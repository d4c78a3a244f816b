// eagle_internal.h -- shared between eagle_api.cpp and eagle_kernels.hip (not part of the public ABI)
#ifndef EAGLE_INTERNAL_H
#define EAGLE_INTERNAL_H
#include <hip/hip_runtime.h>

#include "../../include/eagle_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
int eagle_fail(eagle_ctx* ctx, int code, const char* msg);
int eagle_fail_hip(eagle_ctx* ctx, hipError_t e, const char* where);
// C = A * B, all row-major np x np fp64, np % 128 == 0
int eagle_dev_gemm_f64(eagle_ctx* ctx, const double* A, const double* B, double* C, long np, void* stream);
// eagle_dev_scan_operands in three steps (eagle_kernels.hip): the caller may upload V in row blocks under the first product
#define EAGLE_VROWS_BLOCK 1024  /* rows of V's image per upload + product step (a multiple of 256) */
int eagle_dev_scan_operands_begin(eagle_ctx* ctx, const double* Sa, const double* ahat, long n, long n_pad, double* v_out, double* tmp, void* stream);
int eagle_dev_scan_operands_vrows(eagle_ctx* ctx, const double* Sa, const double* Va, long n_pad, long row0, long row1, double* tmp, void* stream);
int eagle_dev_scan_operands_finish(eagle_ctx* ctx, const double* Sa, const double* Va, long n_pad, double* Wu_out, double* tmp, void* stream);
// the two n^3 products alone (v is made by _begin): W's folded image from resident operands on the fp64 GEMM
int eagle_dev_scan_operands_w_f64(eagle_ctx* ctx, const double* Sa, const double* Va, long n_pad, double* Wu_out, double* tmp, void* stream);
// W = S (V S) from int8 digit slices (eagle_w8.hip): EAGLE_OK, 1 = declined (run the fp64 products), < 0 error
int eagle_dev_scan_operands_w8(eagle_ctx* ctx, const double* Sa, const double* Va, const double* ahat, long n, long n_pad, double* v_out, double* Wu_out,
                               double* tmp, void* stream);
int eagle_dev_colgemv_parts(eagle_ctx* ctx, const double* At, long n, long n_pad, const double* x, double* out, double* part, void* stream);
// the same in three steps (eagle_w8.hip): V may arrive in row blocks of eagle_w8_vrows_block() rows under the first product
int eagle_w8_begin(eagle_ctx* ctx, const double* Sa, const double* Va, const double* ahat, long n, long n_pad, double* v_out, double* Wu_out, double* tmp,
                   int allow_guess, unsigned long s_gen, void* stream);
int eagle_w8_vrows(eagle_ctx* ctx, long r0, long r1, void* stream);
int eagle_w8_finish(eagle_ctx* ctx, void* stream);
int eagle_w8_vrows_block(void);
int eagle_w8_rho(eagle_ctx* ctx, const double* Wu, long n_pad, double* rho, void* stream);
int eagle_w8_true_vara(eagle_ctx* ctx, const int8_t* rows8, long count, long n_pad, long ld, const long* dst_dev, double* out, void* stream);
int eagle_w8_redo_f64(eagle_ctx* ctx, long n_pad, void* stream);
// out = A x where At is the row-major image of A^T (i.e. the column-major R matrix), n_pad % 64 == 0
int eagle_dev_colgemv(eagle_ctx* ctx, const double* At, long n, long n_pad, const double* x, double* out, void* stream);
// 4 KiB of ctx-owned device scratch (flags, small reductions); stream-ordered use only
void* eagle_ctx_scratch(eagle_ctx* ctx);
// grow-only ctx-owned device buffer for the fp4 image of a genotype tile (NULL + last_error on failure)
void* eagle_ctx_f4_buffer(eagle_ctx* ctx, size_t bytes);
int eagle_dev_gemv2_i8(eagle_ctx* ctx, const int8_t* Mt8, long L_pad, long n_pad, long ld, const double* v, const double* w,
                       double scale, double* out_a, double* out_d, void* stream);
int eagle_dev_gemv3_i8(eagle_ctx* ctx, const int8_t* Mt8, long L_pad, long n_pad, long ld, const double* v, const double* w,
                       const double* x, double scale, double* out_a, double* out_d, double* out_x, void* stream);
int eagle_dev_gemv3_2bit(eagle_ctx* ctx, const void* Mt2, long L_pad, long n_pad, long ld, const double* v, const double* w, const double* x,
                         double scale, double* out_a, double* out_d, double* out_x, void* stream);
int eagle_dev_vara_f64_gated(eagle_ctx* ctx, const int8_t* Mt8, long L_pad, long n_pad, long ld, const double* Wu, double* vara_out,
                             const int* run_if, void* stream);
long eagle_vara_f64_split_partial_doubles(long rows_cap, long n_pad);
int eagle_dev_vara_f64_split(eagle_ctx* ctx, const int8_t* rows8, long rows_cap, long n_pad, long ld, const double* Wu,
                             const int* count_dev, const long* dst_dev, double* partial, double* out, void* stream);
long eagle_upper_tiles_count(long n_pad);  // int32 elements of the packed upper 256-tiles of an n_pad x n_pad matrix
int eagle_dev_tiles_pack(eagle_ctx* ctx, int32_t* C32, long n_pad, int32_t* packed, int unpack, void* stream);
int eagle_dev_add_i32(eagle_ctx* ctx, int32_t* dst, const int32_t* src, long count, void* stream);
// eagle_dev_vara_i8_prepare in parts: 0 = all of it, 1 = the W-dependent part only (once per scan), 2 = the block part only
int eagle_dev_vara_i8_prepare_part(eagle_ctx* ctx, const int8_t* Mt8, long L_pad, long n_pad, long ld, const double* Wu, int nslices, void* ws,
                                   const double* v, double* a_out, void* stream, int part);
int eagle_dev_cert_accumulate(eagle_ctx* ctx, const void* cert_ws, long* totals_dev, void* stream);
// certification of a scan cut into marker blocks / device shards against ONE lower bound (eagle_i8mfma.hip, "The same certification ...")
int eagle_dev_cert_bounds(eagle_ctx* ctx, long L, long L_pad, long n_pad, const int8_t* cshift, const int32_t* l1norm, int nslices,
                          const void* vara_ws, const double* vara, double* bound, void* stream);
int eagle_dev_cert_lb_b(eagle_ctx* ctx, long L, const double* a, const double* vara, const double* bound, void* cert_ws, const void* vara_ws,
                        void* stream);
int eagle_cert_tight_max(void);
int eagle_dev_cert_select_b(eagle_ctx* ctx, long L, const double* a, const double* vara, const double* bound, void* cert_ws, double lb,
                            long over_tight, const void* vara_ws, void* stream);
int8_t* eagle_cert_rows(void* cert_ws);
long* eagle_cert_indices(void* cert_ws);
int eagle_dev_cert_reevaluate(eagle_ctx* ctx, const int8_t* Mt8, long ld, long n_pad, const double* Wu, double* vara, void* cert_ws, void* stream);
int eagle_dev_symmetrize(eagle_ctx* ctx, double* A, long n, long ld, void* stream);
int eagle_dev_symmetrize_mean(eagle_ctx* ctx, double* A, long n, long ld, void* stream);
int eagle_dev_scale_rows_pow(eagle_ctx* ctx, double* R, long n, long ld, const double* w, double p, void* stream);
int eagle_dev_transpose_f64(eagle_ctx* ctx, const double* in, double* out, long N, void* stream);
int eagle_dev_dot_matrices(eagle_ctx* ctx, const double* A, long lda, const double* B, long ldb, long n, double* out, void* stream);
void eagle_linalg_release(eagle_ctx* ctx);
void eagle_spectral_release(eagle_ctx* ctx);
int eagle_spectral_prepare_range(eagle_ctx* ctx, const char* f_name_ascii, long L, long n, long m0, long m1, const double* U, double max_memory_in_Gbytes);
int eagle_spectral_host_operands(eagle_ctx* ctx, long n, const double* lambda, const double* UtX, const double* Uty, long p, double varE, double varG,
                                 int NC, double* d, double* G, double* Cm, double* c1);
int eagle_spectral_scan_range(eagle_ctx* ctx, const double* d, const double* G, int NC, const double* Cm, const double* c1, long p, double varG,
                              const long* sel, long nsel, double* a_out, double* vara_out);
int eagle_dev_extract_col(eagle_ctx* ctx, const int8_t* M8, long n, long ld, long col, int* out, void* stream);
// Linkage disequilibrium (eagle_ld.hip) on an int8 Mt tile of `rows` markers x n individuals (ld % 16 == 0, zero from n on).
// sq[r] = (sum g, sum g^2) of marker r from counts[r] = (n0, n1, n2) of eagle_dev_marker_counts.
int eagle_dev_ld_sq(eagle_ctx* ctx, const int32_t* counts, long rows, int32_t* sq, void* stream);
// bit o - 1 of mask[i] (words_per_row = ceil(window / 64) uint64 words per marker, every word of the rows [0, rows) written) is set iff
// markers i and i + o, 1 <= o <= window <= 256, i + o < rows, are in LD at threshold t in [0, 1] (the rule at the head of eagle_ld.hip).
int eagle_dev_ld_band(eagle_ctx* ctx, const int8_t* Mt8, long rows, long n, long ld, const int32_t* sq, long window, double t, uint64_t* mask,
                      long words_per_row, void* stream);
// dots[i * k + j] = sum over the individuals of marker i times row j of B8 (64 rows x ld, rows k .. 63 zero), 1 <= k <= 64
int eagle_dev_ld_dots(eagle_ctx* ctx, const int8_t* Mt8, long rows, long n, long ld, const int8_t* B8, long k, int32_t* dots, void* stream);
// band[i * window + o - 1] (rows x window fp64, every entry written) = r^2 between markers i and i + o of the tile in the fp64 order of
// the header's LD-kNNi section, -1.0 where i + o >= rows or one of the two is monomorphic.
int eagle_dev_ld_r2band(eagle_ctx* ctx, const int8_t* Mt8, long rows, long n, long ld, const int32_t* sq, long window, double* band, void* stream);
// The ranked partner rows of the markers g0 + [c_lo, c_hi) of the panel from a band whose row 0 is marker g0 (a marker's candidates on
// both sides must lie among the band's rows, or beyond the panel's ends).  partners / r2: L x l by the panel's marker; chrom: L or null.
int eagle_dev_ld_partners(eagle_ctx* ctx, const double* band, long rows, long window, long c_lo, long c_hi, long g0, const int32_t* chrom,
                          double min_r2, int l, int32_t* partners, double* r2, void* stream);
// LD scores and the decay histogram of the markers g0 + [c_lo, c_hi) from the same band (include/eagle_hip.h section 1b'''v): U / cnt by
// the panel's marker, written; bin_sum / bin_pairs (nbins words) ADDED to -- zero them before the first core.  Forward pairs are binned
// with their smaller marker, so cores that partition the panel count every pair once.  chrom / pos: L or null; edges: nbins + 1 int64 on
// the device, strictly increasing, 0 <= nbins <= 512 (0: no histogram, the three pointers unused).
int eagle_dev_ld_reduce(eagle_ctx* ctx, const double* band, long rows, long window, long c_lo, long c_hi, long g0, const int32_t* chrom,
                        const int64_t* pos, long max_dist, const int64_t* edges, int nbins, uint64_t* U, int32_t* cnt, uint64_t* bin_sum,
                        int64_t* bin_pairs, void* stream);
// Pairwise haplotype EM (eagle_hapld.hip; include/eagle_hip.h section 1b''''vii).  Mt8 / sq: the first of the `crows` markers the launch
// OWNS, out of `rows` >= crows it holds (the markers behind the owned ones are the partners of the last of them).  recomb / strong (crows x
// words_per_row uint64) and dprime / r2 (crows x window fp64) start at that marker's row, every word of the owned rows is written, each
// may be null; counts: four uint64 totals on the device, ADDED to -- zero them before the first launch.
int eagle_dev_hap_ld(eagle_ctx* ctx, const int8_t* Mt8, long rows, long crows, long n, long ld, const int32_t* sq, long window, double tol,
                     int max_iter, double fg_cut, double dprime_cut, uint64_t* recomb, uint64_t* strong, long words_per_row, double* dprime,
                     double* r2, uint64_t* counts, void* stream);
// The exact line-score pass (eagle_score.hip; include/eagle_hip.h section 1b''''i), device pointers throughout.  B = the int8 digit image of
// the T x cols int32 weights w: eagle_score_b_rows(T, plane_mask) rows of ld bytes (ld % 128 == 0), row rank(p) T + t = digit plane p of
// column t for the planes p of plane_mask in increasing order, zero elsewhere.  out[r T + t] = sum_c w[t cols + c] img[r ld + c] for the
// lines [0, rows) of an image whose rows up to the next multiple of 256 are allocated (pad128(cols) <= ld, ld * 256 < 2^31); c32:
// eagle_line_scores_ws_bytes(rows, T, plane_mask) bytes of workspace.  The image is only read.
long eagle_score_b_rows(long T, int plane_mask);
size_t eagle_line_scores_ws_bytes(long rows, long T, int plane_mask);
int eagle_dev_score_digits(eagle_ctx* ctx, const int32_t* w, long T, long cols, long ld, int plane_mask, int8_t* B, void* stream);
int eagle_dev_line_scores(eagle_ctx* ctx, const int8_t* img, long rows, long cols, long ld, const int8_t* B, long T, int plane_mask,
                          int32_t* c32, int64_t* out, void* stream);
#ifdef __cplusplus
}
#include "eagle_host.h"
// Head of the digit workspace of the int8 scan (eagle_i8mfma.hip): written on the device, copied back by scan_publish for the figures of
// eagle_last_scan_digits / _budget / _enforced.
struct VaraHdr {
    double maxabs_off;  // max |Wu[j][k]|, j != k
    int S;              // digit slices in use
    int pad;
    double bound;       // n_pad^2 * 2^(e+1-8S): absolute error bound of every vara_i
    double sumdiag;     // sum_k |Wu[k][k]|
    double R;           // sum_{j<k} Wu[j][k] (the off-diagonal quadratic form of the all-ones vector)
    double specH;       // > 0: the scan runs on S = S_sliced - 1 digits and |digit error of marker i| <= specH * sum_j m'_ij^2 (k_spectral_decide)
    int S_sliced;       // digits k_slice_w cut (the scale of the integers Q); S_sliced - S is 0 or 1
    int pad2;
    double budget;      // the digit budget of this scan (eagle_set_scan_budget)
    int e;              // the scale exponent w_scale_exp(maxabs_off): the digits are those of round(Wu * 2^(8 S_sliced - e - 2))
    int pad3;
    // second level of the spectral bound (k_gram_hi_i8): sum of squares of the low part of offdiag(Ds Ds), its largest diagonal entry,
    // whether a high part left int8, whether level 1 declined and level 2 is to run, and the level that took the digit off (0: none)
    unsigned long long lo_sumsq;
    int maxdiag, hi_overflow, spec_try2, level;
    // W itself came from int8 digit slices (eagle_w8.hip): || Wu - truth ||_F <= wErr, i.e. |error of marker i| <= wErr sum_j m'_ij^2 on top
    // of the digit terms (0: the fp64 products)
    double wErr;
    // round 4: the budget is tried TIGHT first (1e-7 unless eagle_set_scan_budget fixed one): `budget` above is the one in force for this
    // scan -- the tight one if the digits that run certify a marker with q2 = n_pad to it, else the default; specH1 = level 1's bound while
    // level 2 is being tried
    double specH1;
    // the default budget behind a tight one in force (= budget otherwise): what the certificate ENFORCES per marker falls back to it when
    // more than CERT_TIGHT_MAX markers of the scan miss the tight threshold (see k_cert_select)
    double budget_loose;
};
static_assert(sizeof(VaraHdr) == 120, "VaraHdr: the device kernels and the host copy agree on this layout");
struct eagle_ctx;
bool eagle_w8_wanted(const eagle_ctx* ctx, long n_pad);
void eagle_w8_release(eagle_ctx* ctx);
int eagle_spectral_traits_range(eagle_ctx* ctx, long T, const std::vector<SpectralGroup>& groups, const std::vector<std::vector<double>>& G,
                                const SpectralTraitDesc* desc, const double* par, long npar, long L_total, double* a_out, double* vara_out,
                                eagle_best* best);
int eagle_spectral_rows_range(eagle_ctx* ctx, const long* idx, long k, double* out);
#endif
#endif
