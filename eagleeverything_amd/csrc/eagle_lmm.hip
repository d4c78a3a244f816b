// eagle_lmm.hip -- the exact per-marker mixed-model test in the eigenbasis of K (include/eagle_hip.h section 1d-i): for every marker i
// of the resident Z = Mt U the fit of  y = X beta + m_i gamma + g + e  with delta = sigma_e^2 / sigma_g^2 RE-ESTIMATED for that
// marker (REML or ML), by safeguarded Newton steps in theta = ln delta from the null fit's theta0.
//
//   k_lmm_exact<REML> ... Z (rows of n_pad fp64, row i = U^T m_i) + the staged image B16 (n64 x 16 fp64, one 128-byte row per
//                         eigen-direction k: U^T X in columns 0..c-1, column c left zero for z, U^T y in column c+1, zeros after) +
//                         lam64 (n64 fp64, +inf from k = n on, so a padded k has w = 0)  ->  stat[5 o ..] = (gamma, se, delta, vg, ll),
//                         info[2 o ..] = (code, iterations) for output position o (marker idx[o], or o without a list).
//
// One wave owns one marker from the first evaluation to the result, four markers per 256-thread workgroup; the waves of a
// workgroup share nothing and meet at no barrier (their iteration counts differ), so a marker's result depends on its row of Z,
// B16, lam64 and theta0 alone: the same bits for all markers, for an index list and in any order.
//
// One evaluation at delta walks the eigen-directions in chunks of 64.
//   Part A, one lane = one k of the chunk: w = 1 / (lam_k + delta) (the one division), w^2, w^3 and z_k from the marker's row go to
//   the wave's LDS; sum w, sum w^2, sum w^3 ride in one register each per lane and are added across the wave at the end.
//   Part B, lane = (j = lane & 15, q = lane >> 4): sixteen steps per chunk, step s taking the directions 4 s + q, with B operand
//   x = B16[k][j] (x = z_k for j = c) and the three A operands w x, w^2 x, w^3 x: three v_mfma_f64_16x16x4_f64 per four k into
//   S_r = B' W^r B, r = 1, 2, 3 (C/D: col = lane & 15, row = (lane >> 4) + 4 reg) -- the matrix pipe does the reduction over k.
// The Cholesky factor of A_1 (in place in S_1's p x p block; S_1's row p keeps b_1 and y_1), the solves for beta and A_1^-1 u, A_1^-1
// (sixteen solves, four at a time in the four 16-lane groups), the traces and the step are the wave's own fp64 work in LDS, every
// verdict formed from values that are the same in all 64 lanes.  The log terms of the likelihood are needed for the reported l only:
// one pass over lam64 after the last evaluation.  No atomics, no inline assembly, no block barrier; lane 0 owns the output words.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"

typedef double lm_f64x4 __attribute__((ext_vector_type(4)));

#define LM_P 16            /* padded column count of B */
#define LM_CHUNK 64        /* eigen-directions per chunk = lanes */

struct LmWave {
    double S1[LM_P * LM_P];    // S_1, then the Cholesky factor of A_1 in the lower triangle of its p x p block
    double S2[LM_P * LM_P], S3[LM_P * LM_P];
    double Inv[LM_P * LM_P];   // A_1^-1, zero outside p x p
    double M[LM_P * LM_P];     // A_1^-1 A_2, zero outside p x p
    double w[LM_CHUNK], w2[LM_CHUNK], w3[LM_CHUNK], z[LM_CHUNK];
    double beta[LM_P];
};

struct LmArgs {
    const double* zrow;        // the marker's row of Z
    const double* B16;
    const double* lam;
    long n, n64;
    int c, p;
};

struct LmEval {
    double g, gp, R, gamma, ipp;
};

// LDS traffic between the lanes of ONE wave: its DS operations complete in order, so only the compiler has to be held.
__device__ __forceinline__ void lm_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Butterfly sums: a + b == b + a bit for bit, so every lane (of the wave / of each 16-lane group) ends with the same word.
__device__ __forceinline__ double lm_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double lm_sum16(double v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One pass over the eigen-directions at delta: S_1..S_3 -> S (LDS), sum w^r -> s1..s3 (the same in every lane).
__device__ __forceinline__ void lm_pass(const LmArgs& a, LmWave& S, int lane, double delta, double& s1, double& s2, double& s3) {
    const int j = lane & 15, q = lane >> 4, c = a.c;
    lm_f64x4 acc1 = {0.0, 0.0, 0.0, 0.0}, acc2 = acc1, acc3 = acc1;
    double t1 = 0.0, t2 = 0.0, t3 = 0.0;
    for (long i0 = 0; i0 < a.n64; i0 += LM_CHUNK) {
        {   // part A: this lane's direction (i < n64: lam64 and B16 are padded to it, the row of Z to n_pad >= n64)
            const long i = i0 + lane;
            const double w = 1.0 / (a.lam[i] + delta), w2 = w * w, w3 = w2 * w;
            S.w[lane] = w;
            S.w2[lane] = w2;
            S.w3[lane] = w3;
            S.z[lane] = a.zrow[i];
            t1 += w;
            t2 += w2;
            t3 += w3;
        }
        lm_sync();
#pragma unroll 4
        for (int s = 0; s < LM_CHUNK / 4; s++) {   // part B: directions 4 s + q, column j
            const int kk = 4 * s + q;
            double xv = a.B16[(i0 + kk) * LM_P + j];
            if (j == c) xv = S.z[kk];
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(S.w[kk] * xv, xv, acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(S.w2[kk] * xv, xv, acc2, 0, 0, 0);
            acc3 = __builtin_amdgcn_mfma_f64_16x16x4f64(S.w3[kk] * xv, xv, acc3, 0, 0, 0);
        }
        lm_sync();
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        S.S1[(q + 4 * r) * LM_P + j] = acc1[r];
        S.S2[(q + 4 * r) * LM_P + j] = acc2[r];
        S.S3[(q + 4 * r) * LM_P + j] = acc3[r];
    }
    lm_sync();
    s1 = lm_wave_sum(t1);
    s2 = lm_wave_sum(t2);
    s3 = lm_wave_sum(t3);
}

// In-place Cholesky of the p x p lower triangle of A; d0 = this lane's original diagonal entry A[j][j], j = lane & 15.  False when a
// pivot is not above LMM_PIVOT_REL of its diagonal entry or not finite (the same verdict in every lane: all read the same words).
__device__ __forceinline__ bool lm_chol(double* A, int p, int lane, double d0) {
    for (int j = 0; j < p; j++) {
        const double d = A[j * LM_P + j], dj = __shfl(d0, j);
        if (!(d > dj * LMM_PIVOT_REL) || !(d < __builtin_inf())) return false;
        const double l = sqrt(d);
        lm_sync();
        if (lane == j) A[j * LM_P + j] = l;
        else if (lane > j && lane < p) A[lane * LM_P + j] = A[lane * LM_P + j] / l;
        lm_sync();
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int e = lane + 64 * t, i = e >> 4, kk = e & 15;
            if (kk > j && i >= kk && i < p) A[i * LM_P + kk] -= A[i * LM_P + j] * A[kk * LM_P + j];
        }
        lm_sync();
    }
    return true;
}

// L L' x = b inside every 16-lane group: lane i = lane & 15 holds b_i and returns x_i (lanes i >= p return what they brought).
__device__ __forceinline__ double lm_solve(const double* Lm, int p, int lane, double b) {
    const int i = lane & 15, base = lane & 48;
    for (int j = 0; j < p; j++) {
        const double y = __shfl(b, base | j) / Lm[j * LM_P + j];
        if (i == j) b = y;
        else if (i > j && i < p) b -= Lm[i * LM_P + j] * y;
    }
    for (int j = p - 1; j >= 0; j--) {
        const double x = __shfl(b, base | j) / Lm[j * LM_P + j];
        if (i == j) b = x;
        else if (i < j) b -= Lm[j * LM_P + i] * x;
    }
    return b;
}

// g(theta) = delta l'(delta) and g'(theta) = delta l' + delta^2 l'' from S_1..S_3 in LDS (section 1d-i).  False: singular (code 2).
template <bool REML>
__device__ __forceinline__ bool lm_algebra(const LmArgs& a, LmWave& S, int lane, double delta, double s1, double s2, LmEval& E) {
    const int j = lane & 15, q = lane >> 4, c = a.c, p = a.p;
    const bool in = j < p;
    const double d0 = S.S1[j * LM_P + j];
    const double y1 = S.S1[p * LM_P + p], y2 = S.S2[p * LM_P + p], y3 = S.S3[p * LM_P + p];
    const double b1 = in ? S.S1[p * LM_P + j] : 0.0, b2 = in ? S.S2[p * LM_P + j] : 0.0, b3 = in ? S.S3[p * LM_P + j] : 0.0;
    lm_sync();
    if (!lm_chol(S.S1, p, lane, d0)) return false;
    double beta = lm_solve(S.S1, p, lane, b1);
    if (!in) beta = 0.0;
    if (lane < LM_P) S.beta[lane] = beta;
    lm_sync();
    E.R = y1 - lm_sum16(b1 * beta);
    if (!(E.R > y1 * LMM_PIVOT_REL) || !(E.R < __builtin_inf())) return false;   // the trait lies in the span of [X z]
    double a2 = 0.0, a3 = 0.0;
#pragma unroll
    for (int t = 0; t < LM_P; t++) {                                            // beta is zero from p on: column p (b_r) meets a zero
        a2 = fma(S.S2[j * LM_P + t], S.beta[t], a2);
        a3 = fma(S.S3[j * LM_P + t], S.beta[t], a3);
    }
    const double Q = y2 + lm_sum16(beta * (a2 - 2.0 * b2));
    const double W3 = y3 + lm_sum16(beta * (a3 - 2.0 * b3));
    const double u = in ? b2 - a2 : 0.0;
    double v = lm_solve(S.S1, p, lane, u);
    if (!in) v = 0.0;
    const double Cq = W3 - lm_sum16(u * v);                                     // y' P^3 y
#pragma unroll 1
    for (int t = 0; t < 4; t++) {                                               // A_1^-1, columns 4 t + q
        const int e = 4 * t + q;
        const double b = lm_solve(S.S1, p, lane, j == e ? 1.0 : 0.0);
        S.Inv[j * LM_P + e] = (in && e < p) ? b : 0.0;
    }
    lm_sync();
    E.gamma = __shfl(beta, c);
    E.ipp = S.Inv[c * LM_P + c];
    double T = s1, T2 = s2, m = (double)a.n;
    if (REML) {
        double t12 = 0.0, t13 = 0.0, tmm = 0.0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int e = lane + 64 * t, i = e >> 4, kk = e & 15;
            double mv = 0.0;
#pragma unroll
            for (int r = 0; r < LM_P; r++) mv = fma(S.Inv[i * LM_P + r], S.S2[r * LM_P + kk], mv);
            S.M[e] = kk < p ? mv : 0.0;                                          // row i >= p of Inv is zero
            t12 = fma(S.Inv[e], S.S2[e], t12);                                   // Inv is zero outside p x p
            t13 = fma(S.Inv[e], S.S3[e], t13);
        }
        lm_sync();
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int e = lane + 64 * t, i = e >> 4, kk = e & 15;
            tmm = fma(S.M[e], S.M[kk * LM_P + i], tmm);
        }
        T = s1 - lm_wave_sum(t12);                                               // tr P
        T2 = s2 - 2.0 * lm_wave_sum(t13) + lm_wave_sum(tmm);                     // tr P^2
        m = (double)(a.n - p);
    }
    const double qr = Q / E.R;
    const double lp = 0.5 * (m * qr - T);
    const double lpp = 0.5 * (m * (qr * qr - 2.0 * Cq / E.R) + T2);
    E.g = delta * lp;
    E.gp = E.g + delta * delta * lpp;
    lm_sync();
    return true;
}

template <bool REML>
__global__ __launch_bounds__(256) void k_lmm_exact(const double* __restrict__ Z, long ldz, const double* __restrict__ B16,
                                                   const double* __restrict__ lam64, long n, long n64, int c, double theta0, double tol,
                                                   int max_iter, const long* __restrict__ idx, long count, double* __restrict__ stat,
                                                   int32_t* __restrict__ info) {
    __shared__ LmWave sh[4];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long o = (long)blockIdx.x * 4 + wv;
    if (o >= count) return;                                                     // the whole wave; no block barrier follows
    LmWave& S = sh[wv];
    const long mk = idx ? idx[o] : o;
    const LmArgs a = {Z + mk * ldz, B16, lam64, n, n64, c, c + 1};
    const double nan = __builtin_nan("");
    double theta = theta0, lo = LMM_THETA_MIN, hi = LMM_THETA_MAX, delta = 0.0;
    bool have_lo = false, have_hi = false;
    int code = 1, it = 0;
    LmEval E;
    for (;;) {
        double s1, s2, s3;
        delta = exp(theta);
        lm_pass(a, S, lane, delta, s1, s2, s3);
        if (!lm_algebra<REML>(a, S, lane, delta, s1, s2, E) || !(fabs(E.g) < __builtin_inf()) || !(fabs(E.gp) < __builtin_inf())) {
            code = 2;
            break;
        }
        if (E.g > 0.0) { lo = theta; have_lo = true; }
        if (E.g < 0.0) { hi = theta; have_hi = true; }
        if (E.g > 0.0 && theta >= LMM_THETA_MAX) { code = 4; break; }
        if (E.g < 0.0 && theta <= LMM_THETA_MIN) { code = 3; break; }
        double t = theta - E.g / E.gp;
        if (!(E.gp < 0.0 && t > lo && t < hi && fabs(t - theta) <= LMM_STEP_MAX)) {
            if ((E.g > 0.0 && have_hi) || (E.g < 0.0 && have_lo)) t = 0.5 * (lo + hi);
            else if (E.g > 0.0) t = fmin(theta + LMM_STEP_MAX, LMM_THETA_MAX);
            else if (E.g < 0.0) t = fmax(theta - LMM_STEP_MAX, LMM_THETA_MIN);
            else t = theta;                                                     // g == 0
        }
        if (fabs(t - theta) <= tol) { code = 0; break; }
        if (it >= max_iter) break;
        theta = t;
        it++;
    }
    double gamma = nan, se = nan, vg = nan, ll = nan, dl = nan;
    if (code != 2) {
        const int p = a.p;
        const double m = REML ? (double)(n - p) : (double)n;
        double ls = 0.0;
        for (long i = lane; i < n; i += LM_CHUNK) ls += log(lam64[i] + delta);
        ls = lm_wave_sum(ls);                                                   // - sum log w
        double ld = lane < p ? log(S.S1[lane * LM_P + lane]) : 0.0;             // log det A_1 = 2 sum log L_jj
        ld = 2.0 * lm_sum16(ld);
        ld = __shfl(ld, 0);
        gamma = E.gamma;
        vg = E.R / m;
        se = sqrt(vg * E.ipp);
        dl = delta;
        ll = 0.5 * (m * (log(m / (2.0 * M_PI)) - 1.0 - log(E.R)) - ls - (REML ? ld : 0.0));
    }
    if (lane == 0) {
        stat[5 * o] = gamma;
        stat[5 * o + 1] = se;
        stat[5 * o + 2] = dl;
        stat[5 * o + 3] = vg;
        stat[5 * o + 4] = ll;
        info[2 * o] = code;
        info[2 * o + 1] = it;
    }
}

// Z: rows of ldz fp64 (ldz >= n64), B16: n64 x 16 fp64, lam64: n64 fp64 with +inf from n on, n64 = n rounded up to 64; idx: count
// device longs (rows of Z) or NULL = rows 0 .. count - 1.  theta0 inside [LMM_THETA_MIN, LMM_THETA_MAX].
extern "C" int eagle_dev_lmm(eagle_ctx* ctx, const double* Z, long ldz, const double* B16, const double* lam64, long n, int c, int reml,
                             double theta0, double tol, int max_iter, const long* idx, long count, double* stat, int32_t* info, void* stream) {
    if (count <= 0) return EAGLE_OK;
    const long n64 = (n + 63) / 64 * 64;
    if (n <= 0 || n64 > ldz || c < 1 || c > LM_P - 2 || n <= c + 2) return eagle_fail(ctx, EAGLE_ERR_ARG, "lmm: bad shape");
    if (!(theta0 >= LMM_THETA_MIN && theta0 <= LMM_THETA_MAX) || !(tol > 0.0 && tol < 1.0) || max_iter < 0 || max_iter > 1000)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "lmm: bad fit parameters");
    const long blocks = (count + 3) / 4;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "lmm: too many markers");
    const dim3 grid((unsigned)blocks), blk(256);
    hipStream_t s = (hipStream_t)stream;
    if (reml) hipLaunchKernelGGL(k_lmm_exact<true>, grid, blk, 0, s, Z, ldz, B16, lam64, n, n64, c, theta0, tol, max_iter, idx, count, stat, info);
    else hipLaunchKernelGGL(k_lmm_exact<false>, grid, blk, 0, s, Z, ldz, B16, lam64, n, n64, c, theta0, tol, max_iter, idx, count, stat, info);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return eagle_fail_hip(ctx, e, __func__);
    return EAGLE_OK;
}

// argument errors are decided before the context is touched: without one the text goes where eagle_open_error() finds it
static int lmm_fail(eagle_ctx* ctx, const char* what) {
    char msg[160];
    snprintf(msg, sizeof msg, "spectral_lmm: %s", what);
    if (ctx) return eagle_fail(ctx, EAGLE_ERR_ARG, msg);
    snprintf(g_open_err, sizeof g_open_err, "%s", msg);
    return EAGLE_ERR_ARG;
}

extern "C" int eagle_spectral_lmm(eagle_ctx* ctx, const double* lambda, const double* UtX, const double* Uty, int c, int reml, double theta0,
                                  double tol, int max_iter, const long* idx, long nidx, double* stat_out, int32_t* info_out) {
    if (!lambda || !UtX || !Uty || !stat_out || !info_out) return lmm_fail(ctx, "NULL argument");
    if (c < 1 || c > LM_P - 2) return lmm_fail(ctx, "c outside [1, 14]");
    if (reml != 0 && reml != 1) return lmm_fail(ctx, "reml outside {0, 1}");
    if (!(theta0 == theta0) || fabs(theta0) == INFINITY) return lmm_fail(ctx, "theta0 is not finite");
    if (!(tol > 0.0 && tol < 1.0)) return lmm_fail(ctx, "tol not in (0, 1)");
    if (max_iter < 0 || max_iter > 1000) return lmm_fail(ctx, "max_iter outside [0, 1000]");
    if (idx && nidx < 0) return lmm_fail(ctx, "nidx is negative");
    if (!ctx) return lmm_fail(ctx, "no context");
    if (!ctx->peers.empty()) return lmm_fail(ctx, "a multi-device context is not supported (single device only)");
    if (ctx->spectral_L <= 0 || !ctx->d_Z) return lmm_fail(ctx, "eagle_spectral_prepare has not run");
    const long n = ctx->z_n, L = ctx->z_L, np = eagle_pad(n), n64 = (n + 63) / 64 * 64;
    if (n <= c + 2) return lmm_fail(ctx, "n <= c + 2: no residual degrees of freedom");
    const long count = idx ? nidx : L;
    for (long o = 0; idx && o < nidx; o++)
        if (idx[o] < 0 || idx[o] >= L) return lmm_fail(ctx, "marker index out of range");
    const double dmin = exp(LMM_THETA_MIN);
    std::vector<double> B16((size_t)n64 * LM_P, 0.0), lam64(n64, INFINITY);
    for (long k = 0; k < n; k++) {
        if (!(lambda[k] + dmin > 0.0) || !(lambda[k] < INFINITY)) return lmm_fail(ctx, "lambda_k + e^-10 must be positive and finite");
        lam64[k] = lambda[k];
        for (int j = 0; j < c; j++) B16[(size_t)k * LM_P + j] = UtX[(size_t)j * n + k];
        B16[(size_t)k * LM_P + c + 1] = Uty[k];
    }
    for (size_t e = 0; e < B16.size(); e++)
        if (!(fabs(B16[e]) < INFINITY)) return lmm_fail(ctx, "a non-finite entry of UtX or Uty");
    if (count == 0) return EAGLE_OK;
    const double th0 = fmin(fmax(theta0, LMM_THETA_MIN), LMM_THETA_MAX);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf dB, dl, di, ds, dn;
    HIPCHK(ctx, dB.alloc(sizeof(double) * B16.size()));
    HIPCHK(ctx, dl.alloc(sizeof(double) * n64));
    HIPCHK(ctx, ds.alloc(sizeof(double) * 5 * count));
    HIPCHK(ctx, dn.alloc(sizeof(int32_t) * 2 * count));
    HIPCHK(ctx, hipMemcpyAsync(dB.p, B16.data(), sizeof(double) * B16.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dl.p, lam64.data(), sizeof(double) * n64, hipMemcpyHostToDevice, ctx->stream));
    if (idx) {
        HIPCHK(ctx, di.alloc(sizeof(long) * count));
        HIPCHK(ctx, hipMemcpyAsync(di.p, idx, sizeof(long) * count, hipMemcpyHostToDevice, ctx->stream));
    }
    int rc = eagle_dev_lmm(ctx, ctx->d_Z, np, dB.as<double>(), dl.as<double>(), n, c, reml, th0, tol, max_iter, idx ? di.as<long>() : nullptr, count,
                           ds.as<double>(), dn.as<int32_t>(), ctx->stream);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(stat_out, ds.p, sizeof(double) * 5 * count, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(info_out, dn.p, sizeof(int32_t) * 2 * count, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}
