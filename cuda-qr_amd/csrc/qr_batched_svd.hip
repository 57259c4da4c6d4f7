// qr_batched_svd.hip -- the kernel of the batched SVD (qr_batched.c, mi355x_qr.h section 8c): the SVD of the n x n triangle (n <= 64) of
// every matrix of a batch factored by qrd_b_geqp3, in one launch and without a host wait.
//
//   bs_jsvd_kernel<false>   n <= 32: one wave per matrix, four matrices per workgroup (as b_wave_kernel, qr_batched.hip), 4 lanes per pair
//   bs_jsvd_kernel<true>    33 <= n <= 64: one workgroup of 256 threads per matrix, 8 lanes per pair
//
// Per matrix, with A P = Q R already in place:
//   rank cut   r = the leading run of |R(i,i)| > sqrt(n) eps |R(0,0)| (dgejsv's threshold for an absolute error bound); rows r.. of R are
//              dropped (their norm is at most n eps |R(0,0)|: the diagonal of a pivoted R bounds every later row)
//   Jacobi     one-sided, on G = (R with rows r.. zeroed)^T, n x n in LDS, columns r.. exact zeros that are never touched.  Round-robin
//              circle ordering over the columns (qr_jsvd_round_pairs with blocks of one column): a round's floor(n/2) pairs are disjoint,
//              one lane group each.  For (p, q): a = g_p.g_p, b = g_q.g_q, c = g_p.g_q; skipped where a or b is 0, where the pair is not
//              live (js_live of qr_svd.hip: a > eps^2 b and b > eps^2 a) or where |c| <= tol sqrt(a) sqrt(b), tol = sqrt(n) eps; else the
//              rotation of the smaller angle, zeta = (b - a) / (2 c), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), applied to G and, when
//              U is wanted, to W (n x n, starts as I).  The first sweep that rotates nothing ends the iteration and is counted.
//   values     sigma = the column norms of G, sorted descending and stably by rank counting; V-hat = the normalised live columns,
//              row jpvt[j] of V = row j of V-hat
//   complete   r < n only: dgeqr2 of the n x r live block in LDS (one wave, a lane per row); the trailing n - r columns of its Q complete V
//   U          W's columns in sorted order into rows 0 .. n-1 of U, zeros below: qrd_b_ormqr 'N' then makes U = Q [W; 0]
//
// LDS.  G and W are column-major at a leading dimension of 4 mod 8 (wave route) or 8 mod 16 (workgroup route): a ds_read_b64 is served
// per 32-lane half, which is 8 groups of 4 lanes or 4 groups of 8, and the circle ordering hands consecutive groups consecutive columns
// (p ascending, q descending), so the groups of a half read 32 distinct 8-byte slots.  One barrier per round: the wave barrier or
// __syncthreads() in the forms of qr_batched.hip.  The sweep loop's exit is uniform (a ballot; a flag in LDS between barriers).
//
// Every sum runs in an order that n alone fixes (a serial sum per lane over rows l, l + L, ..., then a butterfly over the L lanes of the
// group): results are bitwise repeatable, independent of `batch` and of a matrix's index, and sigma does not depend on whether W is
// accumulated.  No atomics, nothing crosses a workgroup, nothing spins.
//
// From qr_batched_dev.h: the wave helpers, the dlarfg scalars (bs_house) and the LDS cap; the opt-in is qr_common.h's.
//
// Out of scope: a single launch fused with the factorisation and with the product by Q; wide matrices; n > 64.
#include <float.h>

#include "qr_batched_dev.h"

static_assert(QRD_B_MAX_N == 64, "a column per lane of one wave: at most 64 columns");

// leading dimension of G and W: >= n, 4 mod 8 for n <= 32 and 8 mod 16 above (see the header of this file)
__host__ __device__ __forceinline__ int bs_ld(int n) { return n <= 32 ? ((n + 3) / 8) * 8 + 4 : ((n + 7) / 16) * 16 + 8; }

// doubles of LDS per matrix: G, W when U is wanted, sigma[n], tau[n], pos[n] (ints, in n doubles), the flag word (in 2 doubles)
__host__ __device__ __forceinline__ size_t bs_doubles(int n, int wantu) { return (size_t) (wantu ? 2 : 1) * n * bs_ld(n) + 3 * (size_t) n + 2; }

// One wave, lane = row.  dgeqr2 of the n x r block Gs (Gs[c * ld + i], r < n <= 64): v below the diagonal, tau to taus.
__device__ __forceinline__ void bs_house(double* Gs, int ld, int n, int r, double* taus, int lane)
{
    const bool in = lane < n;
    for (int j = 0; j < r; ++j) {
        const double x = in && lane > j ? Gs[j * ld + lane] : 0.0;
        const double xnorm = qb_wave_nrm(x, qb_wave_sum(x * x));
        const double alpha = Gs[j * ld + j];
        double tj = 0.0;
        if (xnorm != 0.0) {                   // (wave-uniform)
            double beta, scal;                // (beta is not stored: only the trailing columns of this Q are used)
            tj = qb_larfg_n(alpha, xnorm, beta, scal);
            const double v = lane > j ? x * scal : (lane == j ? 1.0 : 0.0);
            for (int c = j + 1; c < r; ++c) {
                const double y = in && lane >= j ? Gs[c * ld + lane] : 0.0;
                const double w = tj * qb_wave_sum(v * y);
                if (in && lane >= j) Gs[c * ld + lane] = fma(-w, v, y);
            }
            if (in && lane > j) Gs[j * ld + lane] = v;
        }
        if (lane == 0) taus[j] = tj;
        QB_WAVE_SYNC();                       // (the next column's alpha was written by another lane)
    }
}

template <bool WG>
__global__ void __launch_bounds__(256) bs_jsvd_kernel(const double* __restrict__ A, int m, int n, int lda, size_t strideA,
                                                      const int* __restrict__ jpvt, size_t stridej, double* __restrict__ S, size_t strideS,
                                                      double* __restrict__ U, int ldu, size_t strideU, double* __restrict__ V, int ldv,
                                                      size_t strideV, int* __restrict__ rank, int* __restrict__ sweeps,
                                                      int* __restrict__ info, double tol, int max_sweeps, int batch)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int L = WG ? 8 : 4;             // lanes per pair
    constexpr int NT = WG ? 256 : 64;         // threads per matrix
    constexpr int NG = NT / L;                // lane groups per matrix: >= n / 2 on either route
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int t = WG ? (int) threadIdx.x : lane;
    const size_t q = WG ? (size_t) blockIdx.x : (size_t) blockIdx.x * 4 + wv;
    if (!WG && q >= (size_t) batch) return;   // (wave route: no workgroup barrier below, the waves are independent)
#define BS_SYNC() do { if (WG) __syncthreads(); else QB_WAVE_SYNC(); } while (0)
    const bool wantu = U != nullptr;
    const int ld = bs_ld(n);
    double* Gs = sm + (WG ? 0 : (size_t) wv * bs_doubles(n, wantu));
    double* Ws = Gs + (size_t) n * ld;        // (used only when U is wanted)
    double* sig = Gs + (size_t) (wantu ? 2 : 1) * n * ld;
    double* taus = sig + n;
    int* pos = reinterpret_cast<int*>(taus + n);
    int* flag = reinterpret_cast<int*>(taus + 2 * n);
    const double* Aq = A + q * strideA;
    const int* jq = jpvt + q * stridej;

    // the rank cut, the same in every wave
    const double d = lane < n ? Aq[(size_t) lane * lda + lane] : 0.0;
    const double thr = tol * fabs(__shfl(d, 0));
    const unsigned long long small = __ballot(lane < n && !(fabs(d) > thr));
    const int r = small ? __ffsll((long long) small) - 1 : n;

    // G(i, c) = R(c, i) for c < r, i >= c; W = I
    for (int idx = t; idx < n * n; idx += NT) {
        const int i = idx / n, c = idx - i * n;
        Gs[c * ld + i] = c < r && i >= c ? Aq[(size_t) i * lda + c] : 0.0;
        if (wantu) Ws[c * ld + i] = i == c ? 1.0 : 0.0;
    }
    if (WG && t == 0) *flag = 0;
    BS_SYNC();

    const int g = t / L, l = t & (L - 1);
    const int N = (n & 1) ? n : n - 1;        // the columns on the circle; an even count leaves column n - 1 in the middle
    const int nrounds = n < 2 ? 0 : N, npairs = n / 2;
    const double e2 = DBL_EPSILON * DBL_EPSILON;
    int sw = 0;
    bool done = false;
    while (!done && sw < max_sweeps) {        // (uniform: `done` is the same in every thread of the matrix)
        bool rot = false;
        for (int rd = 0; rd < nrounds; ++rd) {
            int p = 0, qq = 0;
            bool act = g < npairs;
            if (act) {
                if (!(n & 1) && g == 0) {
                    p = rd;
                    qq = n - 1;
                } else {
                    const int k = (n & 1) ? g + 1 : g;
                    const int ca = (rd + k) % N, cb = (rd - k + N) % N;
                    p = ca < cb ? ca : cb;
                    qq = ca < cb ? cb : ca;
                }
                act = qq < r;                 // (columns r.. are exact zeros: b == 0)
            }
            double a = 0.0, b = 0.0, c = 0.0;
            if (act)
                for (int i = l; i < n; i += L) {
                    const double x = Gs[p * ld + i], y = Gs[qq * ld + i];
                    a = fma(x, x, a);
                    b = fma(y, y, b);
                    c = fma(x, y, c);
                }
#pragma unroll
            for (int o = 1; o < L; o <<= 1) {
                a += __shfl_xor(a, o);
                b += __shfl_xor(b, o);
                c += __shfl_xor(c, o);
            }
            if (act && a > 0.0 && b > 0.0 && a > e2 * b && b > e2 * a && fabs(c) > tol * sqrt(a) * sqrt(b)) {
                const double zeta = (b - a) / (2.0 * c);
                const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
                for (int i = l; i < n; i += L) {
                    const double x = Gs[p * ld + i], y = Gs[qq * ld + i];
                    Gs[p * ld + i] = fma(cs, x, -(sn * y));
                    Gs[qq * ld + i] = fma(sn, x, cs * y);
                }
                if (wantu)
                    for (int i = l; i < n; i += L) {
                        const double x = Ws[p * ld + i], y = Ws[qq * ld + i];
                        Ws[p * ld + i] = fma(cs, x, -(sn * y));
                        Ws[qq * ld + i] = fma(sn, x, cs * y);
                    }
                rot = true;
            }
            BS_SYNC();
        }
        ++sw;
        if (WG) {
            if (rot) *flag = 1;
            __syncthreads();
            done = *flag == 0;
            __syncthreads();
            if (t == 0) *flag = 0;
            __syncthreads();
        } else {
            done = __ballot(rot) == 0ull;
        }
    }

    // sigma = the column norms, by the lane groups again
    for (int c0 = 0; c0 < n; c0 += NG) {
        const int c = c0 + g;
        double a = 0.0;
        if (c < r)
            for (int i = l; i < n; i += L) {
                const double x = Gs[c * ld + i];
                a = fma(x, x, a);
            }
#pragma unroll
        for (int o = 1; o < L; o <<= 1) a += __shfl_xor(a, o);
        if (c < n && l == 0) sig[c] = c < r ? sqrt(a) : 0.0;
    }
    BS_SYNC();
    // descending, stable, by rank counting: column t goes to place pos[t].  n <= 64: all of it is in wave 0
    if (!WG || wv == 0) {
        double s = 0.0;
        if (lane < n) {
            s = sig[lane];
            int k = 0;
            for (int i = 0; i < n; ++i) {
                const double si = sig[i];
                k += (si > s || (si == s && i < lane)) ? 1 : 0;
            }
            pos[lane] = k;
            S[q * strideS + k] = s;
        }
        const unsigned long long nz = __ballot(lane < n && s > 0.0);
        if (lane == 0) {
            if (rank) rank[q] = __popcll(nz);
            if (sweeps) sweeps[q] = sw;
            info[q] = done ? 0 : 1;
        }
    }
    BS_SYNC();

    if (wantu) {                              // W's columns in sorted order over rows 0 .. n-1, zeros below
        double* Uq = U + q * strideU;
        for (int idx = t; idx < n * m; idx += NT) {
            const int c = idx / m, i = idx - c * m;
            Uq[(size_t) pos[c] * ldu + i] = i < n ? Ws[c * ld + i] : 0.0;
        }
    }
    if (!V) return;                           // (uniform)
    double* Vq = V + q * strideV;
    for (int idx = t; idx < r * n; idx += NT) {
        const int c = idx / n, i = idx - c * n;
        const double s = sig[c];
        if (s > 0.0) Gs[c * ld + i] /= s;
    }
    BS_SYNC();
    for (int idx = t; idx < r * n; idx += NT) {
        const int c = idx / n, j = idx - c * n;
        const int row = min(max(jq[j], 0), n - 1);
        Vq[(size_t) pos[c] * ldv + row] = Gs[c * ld + j];
    }
    if (r == n) return;                       // (uniform)
    BS_SYNC();                                // (the live block is read no more: the reflectors may overwrite it)
    if (!WG || wv == 0) bs_house(Gs, ld, n, r, taus, lane);
    BS_SYNC();
    // column k >= r of V-hat = H_0 .. H_{r-1} e_k, a wave per column with the column in registers (lane = row); sigma_k = 0 sorts it to place k
    const int row = lane < n ? min(max(jq[lane], 0), n - 1) : 0;
    for (int k = r + (WG ? wv : 0); k < n; k += (WG ? 4 : 1)) {
        double y = lane == k ? 1.0 : 0.0;
        for (int j = r - 1; j >= 0; --j) {
            const double v = lane < n && lane > j ? Gs[j * ld + lane] : (lane == j ? 1.0 : 0.0);
            const double w = taus[j] * qb_wave_sum(v * y);
            y = fma(-w, v, y);
        }
        if (lane < n) Vq[(size_t) k * ldv + row] = y;
    }
#undef BS_SYNC
}

// the kernels that may ask for more than 64 KiB of LDS (qr_allow_lds)
static int bs_allow_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(bs_jsvd_kernel<false>), reinterpret_cast<const void*>(bs_jsvd_kernel<true>)};
    return qr_allow_lds(fns, QB_LDS_CAP, done);
}

extern "C" {

// The SVD of the triangle of every matrix factored by qrd_b_geqp3: S (n per matrix, descending), U (may be NULL) <- [W; 0] (m x n,
// for qrd_b_ormqr 'N'), V (may be NULL, n x n), rank and sweeps (may be NULL), info (0, or 1: max_sweeps reached).  -7: shape not taken
int qrd_b_jsvd(void* stream, const double* A, int m, int n, int lda, size_t strideA, const int* jpvt, size_t stridej, double* S,
               size_t strideS, double* U, int ldu, size_t strideU, double* V, int ldv, size_t strideV, int* rank, int* sweeps, int* info,
               int max_sweeps, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || n > QRD_B_MAX_N || m < n || m > QRD_B_MAX_ROWS || lda < m || !A || !jpvt || !S || !info || max_sweeps < 1 ||
        (U && ldu < m) || (V && ldv < n))
        return -7;
    const int rc = bs_allow_lds();
    if (rc) return rc;
    hipStream_t s = (hipStream_t) stream;
    const double tol = sqrt((double) n) * DBL_EPSILON;
    const size_t per = sizeof(double) * bs_doubles(n, U != nullptr);
    if (n <= 32)
        hipLaunchKernelGGL(bs_jsvd_kernel<false>, dim3((unsigned) (((size_t) batch + 3) / 4)), dim3(256), 4 * per, s, A, m, n, lda, strideA, jpvt,
                           stridej, S, strideS, U, ldu, strideU, V, ldv, strideV, rank, sweeps, info, tol, max_sweeps, batch);
    else
        hipLaunchKernelGGL(bs_jsvd_kernel<true>, dim3((unsigned) batch), dim3(256), per, s, A, m, n, lda, strideA, jpvt, stridej, S, strideS, U,
                           ldu, strideU, V, ldv, strideV, rank, sweeps, info, tol, max_sweeps, batch);
    return (int) hipGetLastError();
}

}   // extern "C"
