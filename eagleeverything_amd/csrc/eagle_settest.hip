// eagle_settest.hip -- burden and SKAT statistics of marker sets under the mixed model (include/eagle_hip.h section 1d''): for every
// set S of up to SETTEST_MAX_MARKERS = 64 rows of the resident Z = Mt U the augmented weighted Gram G = A' diag(d) A of
// A = [z_j1 .. z_jm | U^T X | U^T y], the Schur complement on the U^T X block -- the scores s and their covariance Phi, the a and the
// matrix whose diagonal is the vara of eagle_spectral_scan -- and the seven statistics (Q, Ub, Vb, tr Aw .. tr Aw^4), Aw = W Phi W.
//
//   k_settest_gram<T> ... one 256-thread workgroup per set of T = ceil(m / 16) marker tiles.  Columns are padded to 16: T marker
//                         tiles (a padded column is a zero column) plus one operand tile from the staged image O16 (n64 x 16 fp64, one
//                         128-byte row per eigen-direction k: U^T X in columns 0..c-1, U^T y in column c, zeros after).  d64 holds
//                         n64 fp64, d_k = 1 / (varE + varG lambda_k) and 0 from k = n on, so a padded direction needs no mask.
//
// The pass.  The eigen-directions are cut into chunks of 64; chunk number r belongs to wave r mod 4, so the partition depends on n
// alone.  A lane (i = lane & 15, q = lane >> 4) loads the 32 contiguous bytes Z[row_i][k0 + 4 q .. 4 q + 3] of each marker tile (a
// row's 128-byte line is one request of its four lanes), the same four directions of d64 and of its column i of O16, and uses them in
// four successive v_mfma_f64_16x16x4_f64 steps: in step s the instruction's slot q holds direction k0 + 4 q + s, for the A operand
// (d_k x) and the B operand (x) alike.  Each wave keeps the (T + 1)(T + 2) / 2 <= 15 lower-triangle 16 x 16 tiles of G (C/D: col =
// lane & 15, row = (lane >> 4) + 4 reg).  The four partial Grams are added in LDS in wave order; the upper triangle is a copy of the
// lower.  No atomics, no inline assembly, no LDS staging of Z.
//
// The epilogue is the workgroup's own fp64 work in LDS, every verdict formed from words that all 256 threads read alike: the Cholesky
// factor of G_xx (one thread per entry of the 16 x 16 block), G_xx^-1 (sixteen solves, one per 16-lane group), B = G_xx^-1 [G_xz | G_xy],
// the lower triangle of Phi and its mirror, the degenerate-marker rule, Aw in place of Phi, Aw^2 entry by entry (never stored) and the
// traces, summed per thread in index order, per wave by a butterfly and over the waves in wave order.  Thread 0 owns the output words.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"

typedef double st_f64x4 __attribute__((ext_vector_type(4)));

#define ST_P 16            /* columns of the operand tile */
#define ST_CMAX 14         /* the most columns of X */
#define ST_CHUNK 64        /* eigen-directions per wave chunk */
#define ST_CODE_XX 1       /* internal: G_xx failed its pivot rule (turned into the call's argument error) */

template <int T>
struct StShared {
    static constexpr int NP = 16 * (T + 1), LD = NP + 1, NC = 16 * T;
    double G[NP * LD];                   // the Gram; then L of G_xx in its X block, Phi and Aw in its marker block
    double Bm[ST_CMAX * (NC + 1)];       // B = G_xx^-1 [G_xz | G_xy], row a, column j < m: marker j, column m: y
    double Inv[ST_P * ST_P];             // G_xx^-1, zero outside c x c
    double xd[ST_P];                     // the diagonal of G_xx before the factorisation
    double gd[NC], s[NC], w[NC];         // diag G_zz, the scores, the weights (0 from m on)
    double red[4 * 5];
    int deg[NC];
};

__device__ __forceinline__ double st_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int T>
__global__ __launch_bounds__(256) void k_settest_gram(const double* __restrict__ Z, long ldz, const double* __restrict__ O16,
                                                      const double* __restrict__ d64, long n64, int c, double varG,
                                                      const long* __restrict__ set_ptr, const long* __restrict__ set_idx,
                                                      const double* __restrict__ omega, const long* __restrict__ order,
                                                      const long* __restrict__ cov_off, double* __restrict__ stat, int32_t* __restrict__ info,
                                                      double* __restrict__ score, double* __restrict__ cov) {
    typedef StShared<T> Sh;
    constexpr int NT = T + 1, NP = Sh::NP, LD = Sh::LD, NC = Sh::NC;
    __shared__ Sh S;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, i = lane & 15, q = lane >> 4;
    const long o = order[blockIdx.x], base = set_ptr[o];
    const int m = (int)(set_ptr[o + 1] - base);                                  // 16 (T - 1) < m <= 16 T: the host sorted the sets by T

    // ---- the pass over the eigen-directions: this wave's chunks
    const double* zp[T];
    bool live[T];
#pragma unroll
    for (int t = 0; t < T; t++) {
        live[t] = 16 * t + i < m;
        zp[t] = Z + set_idx[base + (live[t] ? 16 * t + i : 0)] * ldz;
    }
    const st_f64x4 zero = {0.0, 0.0, 0.0, 0.0};
    st_f64x4 acc[NT * (NT + 1) / 2];
#pragma unroll
    for (int e = 0; e < NT * (NT + 1) / 2; e++) acc[e] = zero;
    const long nch = n64 / ST_CHUNK;
    for (long ch = wv; ch < nch; ch += 4) {
#pragma unroll
        for (int sb = 0; sb < ST_CHUNK / 16; sb++) {
            const long kb = ch * ST_CHUNK + 16 * sb + 4 * q;                     // kb + 3 < n64 <= ldz
            const st_f64x4 dv = *(const st_f64x4*)(d64 + kb);
            st_f64x4 x[NT];
#pragma unroll
            for (int t = 0; t < T; t++) x[t] = live[t] ? *(const st_f64x4*)(zp[t] + kb) : zero;
#pragma unroll
            for (int s = 0; s < 4; s++) x[T][s] = O16[(kb + s) * ST_P + i];
#pragma unroll
            for (int s = 0; s < 4; s++) {
#pragma unroll
                for (int a = 0; a < NT; a++) {
                    const double av = dv[s] * x[a][s];
#pragma unroll
                    for (int b = 0; b <= a; b++)
                        acc[a * (a + 1) / 2 + b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, x[b][s], acc[a * (a + 1) / 2 + b], 0, 0, 0);
                }
            }
        }
    }
    // ---- the four partial Grams, added in wave order
#pragma unroll 1
    for (int w = 0; w < 4; w++) {
        if (wv == w) {
#pragma unroll
            for (int a = 0; a < NT; a++)
#pragma unroll
                for (int b = 0; b <= a; b++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int e = (16 * a + q + 4 * r) * LD + 16 * b + i;
                        const double v = acc[a * (a + 1) / 2 + b][r];
                        S.G[e] = w == 0 ? v : S.G[e] + v;
                    }
        }
        __syncthreads();
    }
    for (int e = tid; e < NP * NP; e += 256) {                                   // the upper triangle is a copy of the lower
        const int r = e / NP, cc = e % NP;
        if (cc > r) S.G[r * LD + cc] = S.G[cc * LD + r];
    }
    if (tid < NC) {
        S.gd[tid] = tid < m ? S.G[tid * LD + tid] : 0.0;
        S.w[tid] = tid < m ? omega[base + tid] : 0.0;
        S.deg[tid] = 0;
    }
    if (tid < ST_P) S.xd[tid] = S.G[(NC + tid) * LD + NC + tid];
    __syncthreads();

    // ---- G_xx = L L' in place, one thread per entry of the 16 x 16 block
    double* X = S.G + NC * LD + NC;
    const double nan = __builtin_nan("");
    {
        const int r = tid >> 4, k = tid & 15;
        bool ok = true;
        for (int j = 0; j < c; j++) {
            const double dj = X[j * LD + j];
            if (!(dj > S.xd[j] * LMM_PIVOT_REL) || !(dj < __builtin_inf())) { ok = false; break; }
            const double l = sqrt(dj);
            __syncthreads();
            if (k == j && r == j) X[j * LD + j] = l;
            else if (k == j && r > j && r < c) X[r * LD + j] = X[r * LD + j] / l;
            __syncthreads();
            if (k > j && r >= k && r < c) X[r * LD + k] -= X[r * LD + j] * X[k * LD + j];
            __syncthreads();
        }
        if (!ok) {                                                               // the same verdict in all 256 threads
            if (tid == 0) {
                for (int k2 = 0; k2 < 7; k2++) stat[7 * o + k2] = nan;
                info[2 * o] = ST_CODE_XX;
                info[2 * o + 1] = 0;
            }
            return;
        }
    }
    {   // G_xx^-1: the 16-lane group g solves L L' x = e_g
        const int g = tid >> 4, r = tid & 15, gb = lane & 48;
        double b = r == g ? 1.0 : 0.0;
        for (int j = 0; j < c; j++) {
            const double y = __shfl(b, gb | j) / X[j * LD + j];
            if (r == j) b = y;
            else if (r > j && r < c) b -= X[r * LD + j] * y;
        }
        for (int j = c - 1; j >= 0; j--) {
            const double x = __shfl(b, gb | j) / X[j * LD + j];
            if (r == j) b = x;
            else if (r < j) b -= X[j * LD + r] * x;
        }
        S.Inv[r * ST_P + g] = (r < c && g < c) ? b : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < c * (m + 1); e += 256) {                               // B = G_xx^-1 [G_xz | G_xy]
        const int a = e / (m + 1), j = e % (m + 1), gc = j < m ? j : NC + c;
        double v = 0.0;
        for (int b = 0; b < c; b++) v = fma(S.Inv[a * ST_P + b], S.G[(NC + b) * LD + gc], v);
        S.Bm[a * (NC + 1) + j] = v;
    }
    __syncthreads();
    // ---- s = varG (G_zy - G_zx B_y), Phi = varG^2 (G_zz - G_zx B_z): the lower triangle, then its mirror
    const double vg2 = varG * varG;
    for (int e = tid; e < m * m; e += 256) {
        const int r = e / m, cc = e % m;
        if (cc <= r) {
            double t = 0.0;
            for (int a = 0; a < c; a++) t = fma(S.G[r * LD + NC + a], S.Bm[a * (NC + 1) + cc], t);
            S.G[r * LD + cc] = vg2 * (S.G[r * LD + cc] - t);
        }
    }
    if (tid < m) {
        double t = 0.0;
        for (int a = 0; a < c; a++) t = fma(S.G[tid * LD + NC + a], S.Bm[a * (NC + 1) + m], t);
        S.s[tid] = varG * (S.G[tid * LD + NC + c] - t);
    }
    __syncthreads();
    if (tid < m && !(S.G[tid * LD + tid] > LMM_PIVOT_REL * vg2 * S.gd[tid])) {   // the degenerate-marker rule
        S.deg[tid] = 1;
        S.s[tid] = 0.0;
    }
    __syncthreads();
    int ndeg = 0;
    double Q = 0.0, Ub = 0.0;
    for (int j = 0; j < m; j++) {
        const double t = S.w[j] * S.s[j];
        ndeg += S.deg[j];
        Q = fma(t, t, Q);
        Ub += t;
    }
    for (int e = tid; e < m * m; e += 256) {                                     // rows and columns of degenerate markers: exactly 0
        const int r = e / m, cc = e % m;
        if (cc <= r && (S.deg[r] | S.deg[cc])) S.G[r * LD + cc] = 0.0;
    }
    __syncthreads();
    for (int e = tid; e < m * m; e += 256) {                                     // the mirror: a copy, so Phi is symmetric bit for bit
        const int r = e / m, cc = e % m;
        if (cc > r) S.G[r * LD + cc] = S.G[cc * LD + r];
    }
    __syncthreads();
    for (int e = tid; e < m * m; e += 256) {                                     // Phi goes out; Aw = W Phi W takes its place (own entry only)
        const int r = e / m, cc = e % m;
        const double v = S.G[r * LD + cc];
        if (cov) cov[cov_off[o] + e] = v;
        S.G[r * LD + cc] = v * (S.w[r] * S.w[cc]);                               // w_r w_cc == w_cc w_r: Aw is symmetric bit for bit too
    }
    if (score && tid < m) score[base + tid] = S.s[tid];
    __syncthreads();
    // ---- Vb = sum Aw, c_1 = tr Aw, c_2 = |Aw|_F^2, c_3 = sum Aw o Aw^2, c_4 = |Aw^2|_F^2
    double p[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int e = tid; e < m * m; e += 256) {
        const int r = e / m, cc = e % m;
        const double v = S.G[r * LD + cc];
        double v2 = 0.0;
        for (int k = 0; k < m; k++) v2 = fma(S.G[r * LD + k], S.G[k * LD + cc], v2);
        p[0] += v;
        if (r == cc) p[1] += v;
        p[2] = fma(v, v, p[2]);
        p[3] = fma(v, v2, p[3]);
        p[4] = fma(v2, v2, p[4]);
    }
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const double v = st_wave_sum(p[k]);
        if (lane == 0) S.red[wv * 5 + k] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double r[5];
#pragma unroll
        for (int k = 0; k < 5; k++) r[k] = ((S.red[k] + S.red[5 + k]) + S.red[10 + k]) + S.red[15 + k];
        const bool none = !(r[0] > 0.0) || !(r[2] > 0.0);                        // nothing left: Vb <= 0 or c_2 <= 0
        stat[7 * o] = none ? nan : Q;
        stat[7 * o + 1] = none ? nan : Ub;
#pragma unroll
        for (int k = 0; k < 5; k++) stat[7 * o + 2 + k] = none ? nan : r[k];
        info[2 * o] = none ? 2 : 0;
        info[2 * o + 1] = m - ndeg;
    }
}

// order: the sets of this launch (positions in set_ptr), all of T = ceil(m / 16) marker tiles.
template <int T>
static void st_launch(hipStream_t s, long count, const double* Z, long ldz, const double* O16, const double* d64, long n64, int c, double varG,
                      const long* set_ptr, const long* set_idx, const double* omega, const long* order, const long* cov_off, double* stat,
                      int32_t* info, double* score, double* cov) {
    hipLaunchKernelGGL(k_settest_gram<T>, dim3((unsigned)count), dim3(256), 0, s, Z, ldz, O16, d64, n64, c, varG, set_ptr, set_idx, omega, order,
                       cov_off, stat, info, score, cov);
}

// argument errors are decided before the context is touched: without one the text goes where eagle_open_error() finds it
static int settest_fail(eagle_ctx* ctx, const char* what) {
    char msg[160];
    snprintf(msg, sizeof msg, "spectral_settest: %s", what);
    if (ctx) return eagle_fail(ctx, EAGLE_ERR_ARG, msg);
    snprintf(g_open_err, sizeof g_open_err, "%s", msg);
    return EAGLE_ERR_ARG;
}

extern "C" int eagle_spectral_settest(eagle_ctx* ctx, const double* lambda, const double* UtX, const double* Uty, int c, double varE, double varG,
                                      long nsets, const long* set_ptr, const long* set_idx, const double* omega, double* stat_out,
                                      int32_t* info_out, double* score_out, double* cov_out) {
    if (!lambda || !UtX || !Uty || !set_ptr || !set_idx || !omega || !stat_out || !info_out) return settest_fail(ctx, "NULL argument");
    if (c < 1 || c > ST_CMAX) return settest_fail(ctx, "c outside [1, 14]");
    if (nsets < 0) return settest_fail(ctx, "nsets is negative");
    if (!(fabs(varE) < INFINITY) || !(fabs(varG) < INFINITY)) return settest_fail(ctx, "varE or varG is not finite");
    if (set_ptr[0] != 0) return settest_fail(ctx, "set_ptr must start at 0 and not decrease");
    for (long o = 0; o < nsets; o++)
        if (set_ptr[o + 1] < set_ptr[o]) return settest_fail(ctx, "set_ptr must start at 0 and not decrease");
    for (long o = 0; o < nsets; o++) {
        if (set_ptr[o + 1] == set_ptr[o]) return settest_fail(ctx, "an empty set");
        if (set_ptr[o + 1] - set_ptr[o] > SETTEST_MAX_MARKERS) return settest_fail(ctx, "a set above SETTEST_MAX_MARKERS = 64 markers");
    }
    const long nnz = set_ptr[nsets];
    for (long e = 0; e < nnz; e++)
        if (!(omega[e] >= 0.0) || !(omega[e] < INFINITY)) return settest_fail(ctx, "a negative or non-finite weight");
    for (long e = 0; e < nnz; e++)
        if (set_idx[e] < 0) return settest_fail(ctx, "marker index out of range");
    if (!ctx) return settest_fail(ctx, "no context");
    if (!ctx->peers.empty()) return settest_fail(ctx, "a multi-device context is not supported (single device only)");
    if (ctx->spectral_L <= 0 || !ctx->d_Z) return settest_fail(ctx, "eagle_spectral_prepare has not run");
    const long n = ctx->z_n, L = ctx->z_L, np = eagle_pad(n), n64 = (n + 63) / 64 * 64;
    if (n <= c + 1) return settest_fail(ctx, "n <= c + 1: no residual degrees of freedom");
    // the resident Z holds the markers [z_first, z_first + L) (eagle_spectral_prepare on one device: z_first = 0): rows of Z, as the scan counts them
    const long m0 = ctx->z_first;
    std::vector<long> rows(nnz);
    for (long e = 0; e < nnz; e++) {
        if (set_idx[e] < m0 || set_idx[e] >= m0 + L) return settest_fail(ctx, "marker index out of range");
        rows[e] = set_idx[e] - m0;
    }
    std::vector<double> O16((size_t)n64 * ST_P, 0.0), d64(n64, 0.0);
    for (long k = 0; k < n; k++) {
        const double h = varE + varG * lambda[k];
        if (!(h > 0.0) || !(h < INFINITY)) return settest_fail(ctx, "varE + varG * lambda_k must be positive and finite");
        d64[k] = 1.0 / h;
        for (int j = 0; j < c; j++) O16[(size_t)k * ST_P + j] = UtX[(size_t)j * n + k];
        O16[(size_t)k * ST_P + c] = Uty[k];
    }
    for (size_t e = 0; e < O16.size(); e++)
        if (!(fabs(O16[e]) < INFINITY)) return settest_fail(ctx, "a non-finite entry of UtX or Uty");
    if (nsets == 0) return EAGLE_OK;
    // the sets in the order of their tile count T (stable), one launch per T; the packed positions of cov_out
    std::vector<long> order, cov_off(nsets + 1, 0);
    order.reserve(nsets);
    long nT[5] = {0, 0, 0, 0, 0};
    for (int t = 1; t <= 4; t++)
        for (long o = 0; o < nsets; o++)
            if ((set_ptr[o + 1] - set_ptr[o] + 15) / 16 == t) { order.push_back(o); nT[t]++; }
    for (long o = 0; o < nsets; o++) {
        const long m = set_ptr[o + 1] - set_ptr[o];
        cov_off[o + 1] = cov_off[o] + m * m;
    }
    if (nsets > 0x7fffffffL) return settest_fail(ctx, "too many sets");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf dO, dd, dp, di, dw, dord, doff, ds, dn, dsc, dcv;
    HIPCHK(ctx, dO.alloc(sizeof(double) * O16.size()));
    HIPCHK(ctx, dd.alloc(sizeof(double) * n64));
    HIPCHK(ctx, dp.alloc(sizeof(long) * (nsets + 1)));
    HIPCHK(ctx, di.alloc(sizeof(long) * nnz));
    HIPCHK(ctx, dw.alloc(sizeof(double) * nnz));
    HIPCHK(ctx, dord.alloc(sizeof(long) * nsets));
    HIPCHK(ctx, ds.alloc(sizeof(double) * 7 * nsets));
    HIPCHK(ctx, dn.alloc(sizeof(int32_t) * 2 * nsets));
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(dO.p, O16.data(), sizeof(double) * O16.size(), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(dd.p, d64.data(), sizeof(double) * n64, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(dp.p, set_ptr, sizeof(long) * (nsets + 1), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(di.p, rows.data(), sizeof(long) * nnz, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(dw.p, omega, sizeof(double) * nnz, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(dord.p, order.data(), sizeof(long) * nsets, hipMemcpyHostToDevice, s));
    if (score_out) HIPCHK(ctx, dsc.alloc(sizeof(double) * nnz));
    if (cov_out) {
        HIPCHK(ctx, dcv.alloc(sizeof(double) * cov_off[nsets]));
        HIPCHK(ctx, doff.alloc(sizeof(long) * (nsets + 1)));
        HIPCHK(ctx, hipMemcpyAsync(doff.p, cov_off.data(), sizeof(long) * (nsets + 1), hipMemcpyHostToDevice, s));
    }
    long first = 0;
    for (int t = 1; t <= 4; t++) {
        if (!nT[t]) continue;
        const long* ord = dord.as<long>() + first;
        double *sc = score_out ? dsc.as<double>() : nullptr, *cv = cov_out ? dcv.as<double>() : nullptr;
        const long* off = cov_out ? doff.as<long>() : nullptr;
#define ST_GO(TT) st_launch<TT>(s, nT[t], ctx->d_Z, np, dO.as<double>(), dd.as<double>(), n64, c, varG, dp.as<long>(), di.as<long>(), \
                                dw.as<double>(), ord, off, ds.as<double>(), dn.as<int32_t>(), sc, cv)
        switch (t) {
            case 1: ST_GO(1); break;
            case 2: ST_GO(2); break;
            case 3: ST_GO(3); break;
            default: ST_GO(4); break;
        }
#undef ST_GO
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return eagle_fail_hip(ctx, e, "k_settest_gram");
        first += nT[t];
    }
    HIPCHK(ctx, hipMemcpyAsync(stat_out, ds.p, sizeof(double) * 7 * nsets, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(info_out, dn.p, sizeof(int32_t) * 2 * nsets, hipMemcpyDeviceToHost, s));
    if (score_out) HIPCHK(ctx, hipMemcpyAsync(score_out, dsc.p, sizeof(double) * nnz, hipMemcpyDeviceToHost, s));
    if (cov_out) HIPCHK(ctx, hipMemcpyAsync(cov_out, dcv.p, sizeof(double) * cov_off[nsets], hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    for (long o = 0; o < nsets; o++)                                             // G_xx is the same in every set: so is this verdict
        if (info_out[2 * o] == ST_CODE_XX) return settest_fail(ctx, "X^T H^-1 X is not positive definite (collinear fixed effects)");
    return EAGLE_OK;
}
