// qr_batched.hip -- kernels of the batched interface (qr_batched.c, mi355x_qr.h section 8): many small matrices, one per wave or workgroup.
//
//   b_wave_kernel<W>   m <= 64, at most W <= 32 columns: one wave per matrix, four matrices per workgroup.  Lane i holds row i in W
//                      registers; norms and dot products are wave butterflies; no barrier, no LDS in the factorisation
//   b_wg_kernel        everything else within qr_batched_max_rows: one workgroup per matrix, the matrix resident in LDS at a leading
//                      dimension of 2 mod 32 (the column loop of tp_panel_kernel, qr_update.hip, with no triangle on top); the trailing
//                      update is rank-1, one wave per column
//   b_ormqr_kernel     Q^T C / Q C, V resident in LDS, one wave per column of C with the column in registers
//   b_eye_kernel       the thin identity (qr_orgqr_batched_dev = this + b_ormqr_kernel 'N')
//   b_trsm_kernel      R X = B per matrix, one thread per right-hand side, and the info word (the composed route of gels)
//
// Both factorisation kernels take `nrhs` extra columns from B that are updated but never factored (the fused gels: B <- Q^T B) and
// then run the back substitution in the same launch.  LAPACK dgeqr2 / dlarfg per column: beta = -sign(alpha) hypot(alpha,
// |x|), tau = (beta - alpha) / beta, v = x / (alpha - beta); x == 0 exactly: tau = 0, the column unchanged.
//
// Every sum runs in a fixed order that depends on (m, n, nrhs) alone (wave butterflies, waves added in wave order, serial loops):
// repeated launches are bitwise equal and a matrix's result does not depend on the batch count or its index.  No atomics.
#include <atomic>

#include "qr_common.h"
#include "qr_device.h"

#define B_MAXN QRD_B_MAX_N

static_assert(QRD_B_MAX_N == 64, "the routes below assume at most 64 columns in LDS");

// the same sum in every lane; the order of the additions does not depend on the data
__device__ __forceinline__ double b_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the smallest leading dimension >= m that is 2 mod 32 (conflict-free column-major LDS image, see qr_update.hip)
__host__ __device__ __forceinline__ int b_ld(int m) { return ((m + 29) / 32) * 32 + 2; }

// ---------------------------------------------------------------------------------------------------------------------------------
// wave route.  Dynamic LDS is used by the fused solve only: per wave R (W x (W + 1)) and the right-hand sides (W x (W + 1)).
// ---------------------------------------------------------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(256) b_wave_kernel(double* __restrict__ A, int m, int n, int lda, size_t strideA, double* __restrict__ tau,
                                                     size_t stridetau, double* __restrict__ B, int nrhs, int ldb, size_t strideB,
                                                     int* __restrict__ info, int batch)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) batch) return;          // (no barrier below: the waves of a workgroup are independent)
    double* Aq = A + q * strideA;
    double* Bq = nrhs ? B + q * strideB : nullptr;
    const int ntot = n + nrhs;
    const bool row = lane < m;
    double a[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
        double v = 0.0;
        if (row && c < n) v = Aq[(size_t) c * lda + lane];
        else if (row && c < ntot) v = Bq[(size_t) (c - n) * ldb + lane];
        a[c] = v;
    }
    double tauv = 0.0, diag = 1.0;            // lane j: tau[j] and R(j, j)
#pragma unroll
    for (int j = 0; j < W; ++j) {
        if (j < n) {                          // (wave-uniform)
            const double x = lane > j ? a[j] : 0.0;          // (rows >= m hold zeros)
            const double ssq = b_wave_sum(x * x);
            const double alpha = __shfl(a[j], j);
            double tj = 0.0;
            if (ssq != 0.0) {
                const double beta = -copysign(hypot(alpha, sqrt(ssq)), alpha);
                const double scal = 1.0 / (alpha - beta);
                tj = (beta - alpha) / beta;
                const double v = lane > j ? a[j] * scal : (lane == j ? 1.0 : 0.0);
#pragma unroll
                for (int c = j + 1; c < W; ++c) {
                    if (c < ntot) {
                        const double tw = tj * b_wave_sum(v * a[c]);
                        a[c] = fma(-tw, v, a[c]);
                    }
                }
                a[j] = lane > j ? v : (lane == j ? beta : a[j]);
            }
            if (lane == j) { tauv = tj; diag = a[j]; }
        }
    }
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (row && c < n) Aq[(size_t) c * lda + lane] = a[c];
    if (lane < n) tau[q * stridetau + lane] = tauv;
    if (!nrhs) return;
    const unsigned long long z = __ballot(lane < n && diag == 0.0);
    const int inf = z ? __ffsll((long long) z) : 0;
    if (lane == 0) info[q] = inf;
    if (inf) {                                // B <- Q^T B, no solve
#pragma unroll
        for (int c = 0; c < W; ++c)
            if (row && c >= n && c < ntot) Bq[(size_t) (c - n) * ldb + lane] = a[c];
        return;
    }
    // staging: rows 0 .. n-1 of R and of Q^T B into this wave's LDS, the rest of Q^T B straight back
    constexpr int LW = W + 1;
    double* Rs = sm + (size_t) wv * 2 * W * LW;       // Rs[c * LW + r] = R[r, c]
    double* Xs = Rs + W * LW;                          // Xs[r * LW + k] = (Q^T B)[k, r], then X
#pragma unroll
    for (int c = 0; c < W; ++c) {
        if (c < n) {
            if (lane < n) Rs[c * LW + lane] = a[c];
        } else if (c < ntot) {
            if (lane < n) Xs[(c - n) * LW + lane] = a[c];
            else if (row) Bq[(size_t) (c - n) * ldb + lane] = a[c];
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < nrhs) {                        // (nrhs < W <= 32: one lane per right-hand side)
        double* xr = Xs + lane * LW;
        for (int k = n - 1; k >= 0; --k) {
            double s = xr[k];
            for (int l = k + 1; l < n; ++l) s = fma(-Rs[l * LW + k], xr[l], s);
            xr[k] = s / Rs[k * LW + k];
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int r = 0; r < nrhs; ++r)
        if (lane < n) Bq[(size_t) r * ldb + lane] = Xs[r * LW + lane];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// workgroup route.  LDS: As[c * ld + i] = column c of [A | B], ld = b_ld(m); then red[4], a word for info, 3 spare.
// ---------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ size_t b_wg_lds(int m, int ntot) { return sizeof(double) * ((size_t) ntot * b_ld(m) + 8); }

__global__ void __launch_bounds__(256) b_wg_kernel(double* __restrict__ A, int m, int n, int lda, size_t strideA, double* __restrict__ tau,
                                                   size_t stridetau, double* __restrict__ B, int nrhs, int ldb, size_t strideB,
                                                   int* __restrict__ info)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const int ld = b_ld(m), ntot = n + nrhs;
    double* As = sm;
    double* red = As + (size_t) ntot * ld;
    int* sinfo = (int*) (red + 4);
    double* Aq = A + q * strideA;
    double* Bq = nrhs ? B + q * strideB : nullptr;
    double* tq = tau + q * stridetau;
    for (int c = wv; c < ntot; c += 4) {
        const double* src = c < n ? Aq + (size_t) c * lda : Bq + (size_t) (c - n) * ldb;
        for (int i = lane; i < m; i += 64) As[c * ld + i] = src[i];
    }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        double* vj = As + j * ld;
        double s = 0.0;
        for (int i = j + 1 + t; i < m; i += 256) s = fma(vj[i], vj[i], s);
        s = b_wave_sum(s);
        if (lane == 0) red[wv] = s;
        __syncthreads();
        const double ssq = ((red[0] + red[1]) + red[2]) + red[3];
        double tj = 0.0;
        if (ssq != 0.0) {                     // (the same value in every thread)
            const double alpha = vj[j];
            const double beta = -copysign(hypot(alpha, sqrt(ssq)), alpha);
            const double scal = 1.0 / (alpha - beta);
            tj = (beta - alpha) / beta;
            __syncthreads();                  // (every thread has read alpha and the column)
            for (int i = j + 1 + t; i < m; i += 256) vj[i] *= scal;
            if (t == 0) vj[j] = beta;
            __syncthreads();
            // wave wv: columns j + 1 + wv, + 4, ..: w = v^T c with the unit entry at row j, c -= tau w v
            for (int c = j + 1 + wv; c < ntot; c += 4) {
                double* bc = As + c * ld;
                double d = 0.0;
                for (int i = j + 1 + lane; i < m; i += 64) d = fma(vj[i], bc[i], d);
                d = b_wave_sum(d);
                const double tw = tj * (bc[j] + d);
                for (int i = j + 1 + lane; i < m; i += 64) bc[i] = fma(-tw, vj[i], bc[i]);
                if (lane == 0) bc[j] -= tw;   // (read by every lane above: the wave runs in lock step up to the butterfly; ordered below)
            }
        }
        if (t == 0) tq[j] = tj;
        __syncthreads();                      // (red and column j are read no more)
    }
    for (int c = wv; c < n; c += 4)
        for (int i = lane; i < m; i += 64) Aq[(size_t) c * lda + i] = As[c * ld + i];
    if (!nrhs) return;
    if (t == 0) {
        int inf = 0;
        for (int i = n - 1; i >= 0; --i)
            if (As[i * ld + i] == 0.0) inf = i + 1;
        *sinfo = inf;
        info[q] = inf;
    }
    __syncthreads();
    if (*sinfo == 0) {
        if (t < nrhs) {                       // (nrhs < 64: one thread per right-hand side)
            double* xr = As + (size_t) (n + t) * ld;
            for (int k = n - 1; k >= 0; --k) {
                double s = xr[k];
                for (int l = k + 1; l < n; ++l) s = fma(-As[l * ld + k], xr[l], s);
                xr[k] = s / As[k * ld + k];
            }
        }
        __syncthreads();
    }
    for (int c = n + wv; c < ntot; c += 4)
        for (int i = lane; i < m; i += 64) Bq[(size_t) (c - n) * ldb + i] = As[c * ld + i];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// C <- Q^T C (tr != 0) or Q C.  LDS: Vs[c * ld + i] = V[i, c] below the diagonal, then tau[n].  A wave takes a column of C with row
// lane + 64 k in register k -- RR = 1, 2, 4 or 8 registers, the smallest that holds m rows --, reflectors in order 0 .. n-1 (Q^T) or
// n-1 .. 0 (Q).  (A row register beyond m would only add exact zeros: the result does not depend on RR.)
// ---------------------------------------------------------------------------------------------------------------------------------
#define B_ROWREGS 8
static_assert(QRD_B_MAX_ROWS <= 64 * B_ROWREGS, "a column of C is held in B_ROWREGS registers per lane");

__host__ __device__ __forceinline__ size_t b_ormqr_lds(int m, int n) { return sizeof(double) * ((size_t) n * b_ld(m) + B_MAXN); }

template <int RR>
__global__ void __launch_bounds__(256) b_ormqr_kernel(int tr, const double* __restrict__ A, int m, int n, int lda, size_t strideA,
                                                      const double* __restrict__ tau, size_t stridetau, double* __restrict__ Cm, int nrhs,
                                                      int ldc, size_t strideC)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const int ld = b_ld(m);
    double* Vs = sm;
    double* ts = Vs + (size_t) n * ld;
    const double* Aq = A + q * strideA;
    double* Cq = Cm + q * strideC;
    for (int c = wv; c < n; c += 4)
        for (int i = lane; i < m; i += 64) Vs[c * ld + i] = Aq[(size_t) c * lda + i];
    if (t < n) ts[t] = tau[q * stridetau + t];
    __syncthreads();
    for (int col = (int) blockIdx.y * 4 + wv; col < nrhs; col += (int) gridDim.y * 4) {       // (wave-uniform)
        double* cp = Cq + (size_t) col * ldc;
        double c[RR];
#pragma unroll
        for (int k = 0; k < RR; ++k) {
            const int i = lane + 64 * k;
            c[k] = i < m ? cp[i] : 0.0;
        }
        for (int jj = 0; jj < n; ++jj) {
            const int j = tr ? jj : n - 1 - jj;
            const double tj = ts[j];
            if (tj == 0.0) continue;          // (H = I; wave-uniform)
            const double* vj = Vs + j * ld;
            double v[RR];
            double d = 0.0;
#pragma unroll
            for (int k = 0; k < RR; ++k) {
                const int i = lane + 64 * k;
                v[k] = (i > j && i < m) ? vj[i] : (i == j ? 1.0 : 0.0);
                d = fma(v[k], c[k], d);
            }
            const double tw = tj * b_wave_sum(d);
#pragma unroll
            for (int k = 0; k < RR; ++k) c[k] = fma(-tw, v[k], c[k]);
        }
#pragma unroll
        for (int k = 0; k < RR; ++k) {
            const int i = lane + 64 * k;
            if (i < m) cp[i] = c[k];
        }
    }
}

// Q(i, c) = (i == c), m x n per matrix
__global__ void __launch_bounds__(256) b_eye_kernel(double* __restrict__ Q, int m, int n, int ldq, size_t strideQ)
{
    double* Qq = Q + (size_t) blockIdx.x * strideQ;
    for (int idx = threadIdx.x; idx < m * n; idx += 256) {
        const int c = idx / m, i = idx - c * m;
        Qq[(size_t) c * ldq + i] = i == c ? 1.0 : 0.0;
    }
}

// info[q] = 0 or the smallest i + 1 with R(i, i) == 0; info == 0: rows 0 .. n-1 of B <- R^-1 of them.  LDS: Rs[c * (n + 1) + r], a word.
__host__ __device__ __forceinline__ size_t b_trsm_lds(int n) { return sizeof(double) * ((size_t) n * (n + 1) + 2); }

__global__ void __launch_bounds__(256) b_trsm_kernel(const double* __restrict__ A, int n, int lda, size_t strideA, double* __restrict__ B,
                                                     int nrhs, int ldb, size_t strideB, int* __restrict__ info)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lr = n + 1;
    const size_t q = blockIdx.x;
    double* Rs = sm;
    int* sinfo = (int*) (Rs + (size_t) n * lr);
    const double* Aq = A + q * strideA;
    double* Bq = B + q * strideB;
    for (int idx = t; idx < n * n; idx += 256) {
        const int c = idx / n, r = idx - c * n;
        Rs[c * lr + r] = r <= c ? Aq[(size_t) c * lda + r] : 0.0;
    }
    __syncthreads();
    if (t == 0) {
        int inf = 0;
        for (int i = n - 1; i >= 0; --i)
            if (Rs[i * lr + i] == 0.0) inf = i + 1;
        *sinfo = inf;
        info[q] = inf;
    }
    __syncthreads();
    if (*sinfo) return;
    for (int r = t; r < nrhs; r += 256) {     // (a thread owns its column of B: no other thread reads or writes it)
        double* xr = Bq + (size_t) r * ldb;
        for (int k = n - 1; k >= 0; --k) {
            double s = xr[k];
            for (int l = k + 1; l < n; ++l) s = fma(-Rs[l * lr + k], xr[l], s);
            xr[k] = s / Rs[k * lr + k];
        }
    }
}

// more than 64 KiB of LDS per workgroup has to be allowed per kernel and device, once
static int b_allow_lds(void)
{
    static std::atomic<int> done[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int) e;
    if (dev >= 0 && dev < 64 && done[dev].load(std::memory_order_acquire)) return 0;
    const int cap = 160 * 1024;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(b_wg_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, cap);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(b_ormqr_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, cap);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(b_ormqr_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, cap);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(b_ormqr_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, cap);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(b_ormqr_kernel<8>), hipFuncAttributeMaxDynamicSharedMemorySize, cap);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(b_wave_kernel<32>), hipFuncAttributeMaxDynamicSharedMemorySize, cap);
    if (e == hipSuccess && dev >= 0 && dev < 64) done[dev].store(1, std::memory_order_release);
    return (int) e;
}

template <int W>
static void b_launch_wave(hipStream_t s, double* A, int m, int n, int lda, size_t sa, double* tau, size_t st, double* B, int nrhs, int ldb,
                          size_t sb, int* info, int batch)
{
    const size_t lds = nrhs ? sizeof(double) * 4 * 2 * W * (W + 1) : 0;
    hipLaunchKernelGGL(b_wave_kernel<W>, dim3((unsigned) (((size_t) batch + 3) / 4)), dim3(256), lds, s, A, m, n, lda, sa, tau, st, B, nrhs, ldb,
                       sb, info, batch);
}

extern "C" {

int qrd_b_max_rows(int ncols)
{
    if (ncols < 1 || ncols > QRD_B_MAX_N) return 0;
    // rows that fit for EVERY column count of the class: 32 * 514 and 64 * 258 doubles, plus the small arrays, within 160 KiB
    return ncols <= 32 ? QRD_B_MAX_ROWS : QRD_B_MAX_ROWS / 2;
}

// what the kernels hold: at most QRD_B_MAX_ROWS rows (b_ormqr_kernel's registers) and ncols columns at b_ld(m) plus the small arrays
// (72 doubles cover both b_wg_kernel and b_ormqr_kernel) within 160 KiB of LDS.  Every shape within qrd_b_max_rows fits.
int qrd_b_fits(int m, int ncols)
{
    return ncols >= 1 && ncols <= QRD_B_MAX_N && m >= 1 && m <= QRD_B_MAX_ROWS && sizeof(double) * ((size_t) ncols * b_ld(m) + 72) <= 160 * 1024;
}

int qrd_b_wave_route(int m, int ncols) { return m <= 64 && ncols <= 32; }

// [A | B] factored over the first n columns; nrhs > 0: B's columns ride along (B <- Q^T B), then info and, where it is 0, R X = B in the
// same launch.  -7: shape not taken
int qrd_b_geqrf(void* stream, double* A, int m, int n, int lda, size_t strideA, double* tau, size_t stridetau, double* B, int nrhs, int ldb,
                size_t strideB, int* info, int batch)
{
    const int ntot = n + nrhs;
    if (batch <= 0) return 0;
    if (n < 1 || m < n || nrhs < 0 || !qrd_b_fits(m, ntot) || lda < m || (nrhs && (!B || ldb < m || !info)))
        return -7;
    const int rc = b_allow_lds();
    if (rc) return rc;
    hipStream_t s = (hipStream_t) stream;
    if (qrd_b_wave_route(m, ntot)) {
        if (ntot <= 8) b_launch_wave<8>(s, A, m, n, lda, strideA, tau, stridetau, B, nrhs, ldb, strideB, info, batch);
        else if (ntot <= 16) b_launch_wave<16>(s, A, m, n, lda, strideA, tau, stridetau, B, nrhs, ldb, strideB, info, batch);
        else b_launch_wave<32>(s, A, m, n, lda, strideA, tau, stridetau, B, nrhs, ldb, strideB, info, batch);
    } else {
        hipLaunchKernelGGL(b_wg_kernel, dim3((unsigned) batch), dim3(256), b_wg_lds(m, ntot), s, A, m, n, lda, strideA, tau, stridetau, B, nrhs,
                           ldb, strideB, info);
    }
    return (int) hipGetLastError();
}

int qrd_b_ormqr(void* stream, int trans_t, const double* A, int m, int n, int lda, size_t strideA, const double* tau, size_t stridetau,
                double* Cm, int nrhs, int ldc, size_t strideC, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || m < n || !qrd_b_fits(m, n) || lda < m || ldc < m || nrhs < 1) return -7;
    const int rc = b_allow_lds();
    if (rc) return rc;
    int gy = (nrhs + 15) / 16;                // four columns per wave; beyond 1024 workgroups per matrix the waves loop
    if (gy > 1024) gy = 1024;
    const dim3 grid((unsigned) batch, (unsigned) gy);
    const size_t lds = b_ormqr_lds(m, n);
    hipStream_t s = (hipStream_t) stream;
#define B_ORMQR(RR) hipLaunchKernelGGL(b_ormqr_kernel<RR>, grid, dim3(256), lds, s, trans_t, A, m, n, lda, strideA, tau, stridetau, Cm, nrhs, ldc, strideC)
    if (m <= 64) B_ORMQR(1);
    else if (m <= 128) B_ORMQR(2);
    else if (m <= 256) B_ORMQR(4);
    else B_ORMQR(8);
#undef B_ORMQR
    return (int) hipGetLastError();
}

int qrd_b_eye(void* stream, double* Q, int m, int n, int ldq, size_t strideQ, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || m < n || ldq < m) return -7;
    hipLaunchKernelGGL(b_eye_kernel, dim3((unsigned) batch), dim3(256), 0, (hipStream_t) stream, Q, m, n, ldq, strideQ);
    return (int) hipGetLastError();
}

int qrd_b_trsm(void* stream, const double* A, int n, int lda, size_t strideA, double* B, int nrhs, int ldb, size_t strideB, int* info, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || n > QRD_B_MAX_N || lda < n || ldb < n || nrhs < 1 || !info) return -7;
    hipLaunchKernelGGL(b_trsm_kernel, dim3((unsigned) batch), dim3(256), b_trsm_lds(n), (hipStream_t) stream, A, n, lda, strideA, B, nrhs, ldb,
                       strideB, info);
    return (int) hipGetLastError();
}

}   // extern "C"
