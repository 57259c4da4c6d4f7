// qr_pivot.hip -- kernels of the column-pivoted factorisation (qr_pivot.c; LAPACK dgeqp3 / dlaqps with every column free) and of
// the rank-deficient solve.  Three launches per column c = k0 + j of a panel that starts at column / row k0:
//
//   pv_col_kernel      (row blocks)       pivot = the best of the candidates the previous launch left; swap columns c and pivot over the
//                                         whole height; A(c:, c) -= V(c:, 0..j) F(pivot, 0..j)^T; partial sums of squares of the tail;
//   pv_gemv_kernel     (columns x rows)   THE HOT ONE: P_s(col) = A(rows of split s, col)^T v for every column from k0 on -- the trailing
//                                         ones give F(:, j), the panel's own give V^T v -- with v = the reflector of column c, formed on the
//                                         fly from the unscaled column (nobody writes A here); one workgroup swaps the small state;
//   pv_finish_kernel   (column blocks)    F(col, j) = tau (sum_s P_s(col) - F(col, 0..j) (V^T v)), the pivot row A(c, col) brought up to date,
//                                         the partial norm of col downdated with LAPACK's safeguard, one pivot candidate per workgroup;
//                      (+ row blocks)     the tail of column c scaled, beta and tau stored.
//
// tau, beta and the scale of v are recomputed by every workgroup from the same partial sums in the same order, so no launch waits for a
// one-workgroup step.  Sums over row blocks / row splits are added in index order, never with atomics: repeated calls are bitwise equal.
// A column whose downdated norm has lost too much accuracy is flagged and ends the panel: the panel-length word `pend` drops to j + 1 and
// every later launch of the panel returns at once; the host reads the word once per panel.
// pv_norms_kernel: exact partial norms (all columns at the start, the flagged ones after a block update) and the first candidates.
#include <float.h>
#include <limits.h>
#include <stdint.h>
#include "qr_common.h"
#include "qr_device.h"

#define PV_CB 256          // columns per workgroup of the column-parallel launches = columns per pivot candidate
#define PV_GC 16           // columns per workgroup of the gemv: four waves, four columns each at a time

__device__ __forceinline__ double pv_wave_sum(double x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// sum over the 256 threads of a workgroup, the same bits in every thread (and in every workgroup that sums the same values)
__device__ __forceinline__ double pv_block_sum(double x, double* red)
{
    x = pv_wave_sum(x);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// LAPACK dlarfg from alpha and sigma = |tail|^2 (the library's convention: a zero tail gives tau = 0); iu scales the tail
__device__ __forceinline__ void pv_reflector(double alpha, double sigma, double& tau, double& beta, double& iu)
{
    if (sigma == 0.0) { tau = 0.0; beta = alpha; iu = 0.0; return; }
    const double nrm = sqrt(alpha * alpha + sigma);
    beta = -copysign(nrm, alpha);
    tau = (beta - alpha) / beta;
    iu = 1.0 / (alpha - beta);
}

// the remaining column of largest partial norm, lowest index on a tie, from the per-workgroup candidates (one thread)
__device__ __forceinline__ int pv_pivot(const double* __restrict__ cval, const int* __restrict__ cidx, int ncb, int c)
{
    double best = -1.0;
    int idx = c;
    for (int g = c / PV_CB; g < ncb; ++g) {
        const double v = cval[g];
        if (v > best) { best = v; idx = cidx[g]; }
    }
    return idx;
}

// candidate of one workgroup from sv / si[0 .. 256) (si ascending; entries out of range hold -1): wave 0
__device__ __forceinline__ void pv_block_argmax(const double* sv, const int* si, double* __restrict__ cval, int* __restrict__ cidx, int g)
{
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    double v = -1.0;
    int i = INT_MAX;
#pragma unroll
    for (int q = 0; q < PV_CB / 64; ++q) {
        const int e = lane + 64 * q;
        if (sv[e] > v) { v = sv[e]; i = si[e]; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    if (lane == 0) { cval[g] = v; cidx[g] = i; }
}

// vn1 = vn2 = |A(r0:m, col)| for every column >= c0 (all) or the flagged ones; candidates; the panel-length word reset.
// 16 waves, a column per wave at a time.
__global__ void __launch_bounds__(1024) pv_norms_kernel(const double* __restrict__ A, int lda, int m, int n, int r0, int c0, int all,
                                                        double* __restrict__ vn1, double* __restrict__ vn2, int* __restrict__ flag,
                                                        int* __restrict__ jpvt, double* __restrict__ cval, int* __restrict__ cidx,
                                                        int* __restrict__ pend)
{
    __shared__ double sv[PV_CB];
    __shared__ int si[PV_CB];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (blockIdx.x == 0 && t == 0) *pend = INT_MAX;
    for (int q = 0; q < PV_CB / 16; ++q) {
        const int lc = wave * (PV_CB / 16) + q, col = blockIdx.x * PV_CB + lc;
        double v = -1.0;
        if (col >= c0 && col < n) {
            if (all || flag[col]) {
                const double* __restrict__ a = A + (size_t) col * lda;
                double ss = 0.0;
#pragma unroll 4
                for (int r = r0 + lane; r < m; r += 64) { const double x = a[r]; ss = fma(x, x, ss); }
                v = sqrt(pv_wave_sum(ss));
                if (lane == 0) {
                    vn1[col] = v; vn2[col] = v; flag[col] = 0;
                    if (all) jpvt[col] = col;
                }
            } else v = vn1[col];
        }
        if (lane == 0) { sv[lc] = v; si[lc] = col; }
    }
    __syncthreads();
    pv_block_argmax(sv, si, cval, cidx, blockIdx.x);
}

// rows [blockIdx.x rb, + rb): swap columns c and pivot, bring column c up to date, |tail|^2 of the block
__global__ void __launch_bounds__(256) pv_col_kernel(double* __restrict__ A, int lda, int m, int k0, int j, int rb, const double* __restrict__ F,
                                                     int ldf, const double* __restrict__ cval, const int* __restrict__ cidx, int ncb,
                                                     const int* __restrict__ pend, double* __restrict__ npart, double* __restrict__ alpha_out)
{
    if (j >= *pend) return;
    __shared__ double Fr[QRD_PIVOT_NBP];
    __shared__ double red[4];
    __shared__ int spv;
    const int t = threadIdx.x, c = k0 + j;
    if (t == 0) spv = pv_pivot(cval, cidx, ncb, c);
    __syncthreads();
    const int pvt = spv;
    if (t < j) Fr[t] = F[(size_t) t * ldf + pvt];          // the row of F that the swap brings to position c
    __syncthreads();
    const int rbeg = blockIdx.x * rb, rend = min(m, rbeg + rb);
    double* Ac = A + (size_t) c * lda;
    double* Ap = A + (size_t) pvt * lda;
    const double* Vk = A + (size_t) k0 * lda;
    double ss = 0.0;
    for (int r = rbeg + t; r < rend; r += 256) {
        double x = Ap[r];
        if (pvt != c) Ap[r] = Ac[r];
        if (r >= c) {
            double s = 0.0;
#pragma unroll 8
            for (int k = 0; k < j; ++k) s = fma(Vk[(size_t) k * lda + r], Fr[k], s);
            x -= s;
            if (r == c) *alpha_out = x;
            else ss = fma(x, x, ss);
        }
        Ac[r] = x;
    }
    ss = pv_block_sum(ss, red);
    if (t == 0) npart[blockIdx.x] = ss;
}

// P[blockIdx.y][col] = sum over the rows of split blockIdx.y of A(r, col) v(r): v(c) = 1, v(r > c) = A(r, c) * iu, zero above.
// Splits start at even rows (c & ~1 plus multiples of 128): with an aligned base and an even lda every lane loads 16 bytes.
__global__ void __launch_bounds__(256) pv_gemv_kernel(const double* __restrict__ A, int lda, int m, int n, int k0, int j, int nblk, int rps,
                                                      int vec, const double* __restrict__ npart, const double* __restrict__ alpha_p,
                                                      double* __restrict__ P, int ldp, double* __restrict__ F, int ldf,
                                                      double* __restrict__ vn1, double* __restrict__ vn2, int* __restrict__ jpvt,
                                                      const double* __restrict__ cval, const int* __restrict__ cidx, int ncb,
                                                      const int* __restrict__ pend)
{
    if (j >= *pend) return;
    __shared__ double red[4];
    __shared__ int spv;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, c = k0 + j;
    double tau, beta, iu;
    pv_reflector(*alpha_p, pv_block_sum(t < nblk ? npart[t] : 0.0, red), tau, beta, iu);
    const int rs = (c & ~1) + blockIdx.y * rps, re = min(m, rs + rps);
    const int col0 = k0 + blockIdx.x * PV_GC + wave * 4;
    const double* __restrict__ u = A + (size_t) c * lda;
    const double* cp[4];
    double acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        cp[q] = A + (size_t) (col0 + q < n ? col0 + q : c) * lda;
        acc[q] = 0.0;
    }
#pragma unroll 2
    for (int r = rs + 2 * lane; r < re; r += 128) {
        double u0, u1, a0[4], a1[4];
        if (vec && r + 1 < re) {
            const v2d uu = *reinterpret_cast<const v2d*>(u + r);
            u0 = uu[0]; u1 = uu[1];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const v2d aa = *reinterpret_cast<const v2d*>(cp[q] + r);
                a0[q] = aa[0]; a1[q] = aa[1];
            }
        } else {
            const bool two = r + 1 < re;
            u0 = u[r]; u1 = two ? u[r + 1] : 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { a0[q] = cp[q][r]; a1[q] = two ? cp[q][r + 1] : 0.0; }
        }
        const double v0 = r < c ? 0.0 : (r == c ? 1.0 : u0 * iu);
        const double v1 = r + 1 < c ? 0.0 : (r + 1 == c ? 1.0 : u1 * iu);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = fma(a1[q], v1, fma(a0[q], v0, acc[q]));
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double s = pv_wave_sum(acc[q]);
        if (lane == 0 && col0 + q < n) P[(size_t) blockIdx.y * ldp + col0 + q] = s;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0) {        // nobody reads F, the norms or jpvt in this launch: the swap's small state
        if (t == 0) spv = pv_pivot(cval, cidx, ncb, c);
        __syncthreads();
        const int pvt = spv;
        if (pvt != c) {
            if (t < j) {
                const double f = F[(size_t) t * ldf + c];
                F[(size_t) t * ldf + c] = F[(size_t) t * ldf + pvt];
                F[(size_t) t * ldf + pvt] = f;
            }
            if (t == 0) {
                vn1[pvt] = vn1[c]; vn2[pvt] = vn2[c];
                const int jp = jpvt[c]; jpvt[c] = jpvt[pvt]; jpvt[pvt] = jp;
            }
        }
    }
}

// workgroups [0, ncb): column blocks (F(:, j), pivot row, downdate, candidates); [ncb, ncb + nblk): row blocks (column c scaled, beta, tau)
__global__ void __launch_bounds__(256) pv_finish_kernel(double* __restrict__ A, int lda, int m, int n, int k0, int j, int nblk, int rb, int ncb,
                                                        int nsplit, const double* __restrict__ npart, const double* __restrict__ alpha_p,
                                                        const double* __restrict__ P, int ldp, double* __restrict__ F, int ldf,
                                                        double* __restrict__ vn1, const double* __restrict__ vn2, int* __restrict__ flag,
                                                        double* __restrict__ cval, int* __restrict__ cidx, int* __restrict__ pend,
                                                        double* __restrict__ tau_out)
{
    if (j >= *pend) return;         // (a workgroup of this launch may lower *pend to j + 1: the test reads the same either way)
    __shared__ double red[4];
    __shared__ double aux[QRD_PIVOT_NBP], Vr[QRD_PIVOT_NBP];
    __shared__ double sv[PV_CB];
    __shared__ int si[PV_CB];
    const int t = threadIdx.x, c = k0 + j;
    double tau, beta, iu;
    pv_reflector(*alpha_p, pv_block_sum(t < nblk ? npart[t] : 0.0, red), tau, beta, iu);
    if ((int) blockIdx.x >= ncb) {
        const int rbeg = (blockIdx.x - ncb) * rb, rend = min(m, rbeg + rb);
        double* Ac = A + (size_t) c * lda;
        for (int r = rbeg + t; r < rend; r += 256) {
            if (r > c) Ac[r] *= iu;
            else if (r == c) { Ac[r] = beta; tau_out[c] = tau; }
        }
        return;
    }
    if (t < j) {
        double s = 0.0;
        for (int sp = 0; sp < nsplit; ++sp) s += P[(size_t) sp * ldp + k0 + t];
        aux[t] = s;                                          // (V^T v)(t)
        Vr[t] = A[(size_t) (k0 + t) * lda + c];              // row c of V (its entry in column j is the unit diagonal)
    }
    __syncthreads();
    const int col = blockIdx.x * PV_CB + t;
    double cand = -1.0;
    if (col > c && col < n) {
        double f = 0.0;
        for (int sp = 0; sp < nsplit; ++sp) f += P[(size_t) sp * ldp + col];
        double a = A[(size_t) col * lda + c];
#pragma unroll 8
        for (int k = 0; k < j; ++k) {
            const double fk = F[(size_t) k * ldf + col];
            f = fma(-fk, aux[k], f);
            a = fma(-Vr[k], fk, a);
        }
        f *= tau;
        a -= f;
        F[(size_t) j * ldf + col] = f;
        A[(size_t) col * lda + c] = a;
        double v1 = vn1[col];
        if (v1 != 0.0) {
            double tmp = fabs(a) / v1;
            tmp = fmax(0.0, (1.0 + tmp) * (1.0 - tmp));
            const double q = v1 / vn2[col];
            if (tmp * q * q <= 1.4901161193847656e-08) {      // sqrt(DBL_EPSILON): the downdate has lost half of the digits
                flag[col] = 1;
                atomicMin(pend, j + 1);
            } else {
                v1 *= sqrt(tmp);
                vn1[col] = v1;
            }
        }
        cand = v1;
    } else if (col >= k0 && col <= c) F[(size_t) j * ldf + col] = 0.0;
    sv[t] = cand; si[t] = col;
    __syncthreads();
    pv_block_argmax(sv, si, cval, cidx, blockIdx.x);
}

// S (n x nrhs, ld n): row jpvt[i] = row i of B for i < r, zero for the others
__global__ void __launch_bounds__(256) pv_scatter_kernel(const double* __restrict__ B, int ldb, int n, int r, const int* __restrict__ jpvt,
                                                         double* __restrict__ S)
{
    const int i = blockIdx.x * 256 + threadIdx.x, jc = blockIdx.y;
    if (i < n) S[(size_t) jc * n + jpvt[i]] = i < r ? B[(size_t) jc * ldb + i] : 0.0;
}

// resid[j] = |B(r0:m, j)|, one workgroup per column
__global__ void __launch_bounds__(256) pv_resid_kernel(const double* __restrict__ B, int ldb, int r0, int m, double* __restrict__ resid)
{
    __shared__ double red[4];
    const double* __restrict__ b = B + (size_t) blockIdx.x * ldb;
    double ss = 0.0;
    for (int r = r0 + threadIdx.x; r < m; r += 256) { const double x = b[r]; ss = fma(x, x, ss); }
    ss = pv_block_sum(ss, red);
    if (threadIdx.x == 0) resid[blockIdx.x] = sqrt(ss);
}

static int pv_rb(int m) { return 256 * ((m + 65535) / 65536); }      // rows per row block: at most 256 blocks

static int qrd_pivot_ld(int n) { return (n + 1) & ~1; }                       // even: the block update reads F with 16-byte loads
static int qrd_pivot_ncb(int n) { return (n + PV_CB - 1) / PV_CB; }

extern "C" {

size_t qrd_pivot_ws_doubles(int n)
{
    const size_t ld = (size_t) qrd_pivot_ld(n);
    return ld * (2 * QRD_PIVOT_NBP + 2 + QRD_PIVOT_MAX_SPLIT) + 256 + (size_t) qrd_pivot_ncb(n) + 2;
}
size_t qrd_pivot_ws_ints(int n) { return (size_t) n + (size_t) qrd_pivot_ncb(n) + 2; }

void qrd_pivot_ws_bind(qrd_pivot_ws* w, int n, double* d, int* i)
{
    const size_t ld = (size_t) qrd_pivot_ld(n);
    w->ldf = (int) ld;
    w->F = d; d += ld * QRD_PIVOT_NBP;
    w->FT = d; d += ld * QRD_PIVOT_NBP;
    w->P = d; d += ld * QRD_PIVOT_MAX_SPLIT;
    w->vn1 = d; d += ld;
    w->vn2 = d; d += ld;
    w->npart = d; d += 256;
    w->alpha = d; d += 2;
    w->cval = d;
    w->flag = i; i += n;
    w->cidx = i; i += qrd_pivot_ncb(n);
    w->pend = i;
}

int qrd_pivot_norms(void* stream, const qrd_pivot_ws* w, const double* A, int lda, int m, int n, int r0, int c0, int all, int* jpvt)
{
    if (m < 1 || n < 1 || r0 < 0 || c0 < 0 || lda < m) return -7;
    hipLaunchKernelGGL(pv_norms_kernel, dim3(qrd_pivot_ncb(n)), dim3(1024), 0, (hipStream_t) stream, A, lda, m, n, r0, c0, all, w->vn1, w->vn2,
                       w->flag, jpvt, w->cval, w->cidx, w->pend);
    return (int) hipGetLastError();
}

int qrd_pivot_column(void* stream, const qrd_pivot_ws* w, double* A, int lda, int m, int n, int k0, int j, int* jpvt, double* tau)
{
    const int c = k0 + j;
    if (m < n || n < 1 || k0 < 0 || j < 0 || j >= QRD_PIVOT_NBP || c >= n || lda < m) return -7;
    hipStream_t s = (hipStream_t) stream;
    const int rb = pv_rb(m), nblk = (m + rb - 1) / rb, ncb = qrd_pivot_ncb(n);
    hipLaunchKernelGGL(pv_col_kernel, dim3(nblk), dim3(256), 0, s, A, lda, m, k0, j, rb, w->F, w->ldf, w->cval, w->cidx, ncb, w->pend, w->npart,
                       w->alpha);
    int rc = (int) hipGetLastError();
    if (rc) return rc;
    // the gemv's grid: 16 columns per workgroup, the rows split so that about a thousand workgroups run, 512 rows a split at the least
    const int gx = (n - k0 + PV_GC - 1) / PV_GC, rows = m - (c & ~1);
    int ns = (1024 + gx - 1) / gx;
    if (ns > (rows + 511) / 512) ns = (rows + 511) / 512;
    if (ns > QRD_PIVOT_MAX_SPLIT) ns = QRD_PIVOT_MAX_SPLIT;
    if (ns < 1) ns = 1;
    const int rps = ((rows + ns - 1) / ns + 127) / 128 * 128;
    ns = (rows + rps - 1) / rps;
    const int vec = (((uintptr_t) A) & 15) == 0 && (lda & 1) == 0;
    hipLaunchKernelGGL(pv_gemv_kernel, dim3(gx, ns), dim3(256), 0, s, A, lda, m, n, k0, j, nblk, rps, vec, w->npart, w->alpha, w->P, w->ldf, w->F,
                       w->ldf, w->vn1, w->vn2, jpvt, w->cval, w->cidx, ncb, w->pend);
    rc = (int) hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(pv_finish_kernel, dim3(ncb + nblk), dim3(256), 0, s, A, lda, m, n, k0, j, nblk, rb, ncb, ns, w->npart, w->alpha, w->P,
                       w->ldf, w->F, w->ldf, w->vn1, w->vn2, w->flag, w->cval, w->cidx, w->pend, tau);
    return (int) hipGetLastError();
}

int qrd_pivot_scatter(void* stream, const double* B, int ldb, int n, int nrhs, int r, const int* jpvt, double* S)
{
    if (n < 1 || nrhs < 1 || r < 0 || r > n || ldb < n) return -7;
    hipLaunchKernelGGL(pv_scatter_kernel, dim3((n + 255) / 256, nrhs), dim3(256), 0, (hipStream_t) stream, B, ldb, n, r, jpvt, S);
    return (int) hipGetLastError();
}

int qrd_pivot_resid(void* stream, const double* B, int ldb, int r0, int m, int nrhs, double* resid)
{
    if (nrhs < 1 || r0 < 0 || r0 > m || ldb < m) return -7;
    hipLaunchKernelGGL(pv_resid_kernel, dim3(nrhs), dim3(256), 0, (hipStream_t) stream, B, ldb, r0, m, resid);
    return (int) hipGetLastError();
}

}   // extern "C"
