// qr_batched_dev.h -- the device code that the batched kernel files (qr_batched.hip, qr_batched_update.hip, qr_batched_minnorm.hip,
// qr_batched_svd.hip, qr_batched_damped.hip) share: the wave helpers, the dlarfg scalars, the Householder column step of the wave route and of the workgroup
// route, one reflector on a column in registers, the triangular solves over an LDS image, the info word, and the LDS opt-in.  No
// kernels, no entry points.  Two kernels that call the same step here run the same operations in the same order: that is what makes
// the factors and tau of qrd_b_geqrf, qrd_b_geqp3 (on the permuted columns) and qrd_bm_fused equal bit for bit on the same route.
//
// Every sum runs in a fixed order (wave butterflies, waves added in wave order, serial loops).  No atomics.
#ifndef QR_BATCHED_DEV_H
#define QR_BATCHED_DEV_H

#include <atomic>

#include "qr_common.h"
#include "qr_device.h"

#define QB_LDS_CAP (160 * 1024)           // what one workgroup may hold, once allowed (qb_allow_lds)
#define QB_WG_SMALL 72                    // doubles beside the image of a workgroup route: red[4], words, 64 per-column values; qrd_b_fits budgets them

#define QB_WAVE_SYNC()                                           \
    do {                                                         \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   \
        __builtin_amdgcn_wave_barrier();                         \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   \
    } while (0)

// the same sum in every lane; the order of the additions does not depend on the data
__device__ __forceinline__ double qb_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// v of lane l, l wave-uniform: two readlanes (what __shfl spends a bpermute pair on)
__device__ __forceinline__ double qb_bcast(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// the smallest leading dimension >= m that is 2 mod 32 (conflict-free column-major LDS image, see qr_update.hip)
__host__ __device__ constexpr int qb_ld(int m) { return ((m + 29) / 32) * 32 + 2; }

// LAPACK dlarfg's scalars from alpha and ssq = |x|^2 != 0: returns tau; v = x * scal
__device__ __forceinline__ double qb_larfg(double alpha, double ssq, double& beta, double& scal)
{
    beta = -copysign(hypot(alpha, sqrt(ssq)), alpha);
    scal = 1.0 / (alpha - beta);
    return (beta - alpha) / beta;
}

// Wave route, step j (wave-uniform, j < the columns factored): lane i holds row i of the member in a[], rows past the last hold zeros.
// Column j becomes beta on and v below the diagonal, columns j+1 .. cend-1 (cend wave-uniform) take the reflector; lane j keeps tau_j
// in tauv and R(j, j) in diag.  x == 0 exactly: tau = 0, nothing changes.  Once the caller's loop over j is unrolled (or j is a template
// constant there) every index into a[] is a constant.
template <int W>
__device__ __forceinline__ void qb_wave_col(double (&a)[W], int j, int cend, int lane, double& tauv, double& diag)
{
    const double x = lane > j ? a[j] : 0.0;
    const double ssq = qb_wave_sum(x * x);
    const double alpha = __shfl(a[j], j);
    double tj = 0.0;
    if (ssq != 0.0) {
        double beta, scal;
        tj = qb_larfg(alpha, ssq, beta, scal);
        const double v = lane > j ? a[j] * scal : (lane == j ? 1.0 : 0.0);
#pragma unroll
        for (int c = j + 1; c < W; ++c) {
            if (c < cend) {
                const double tw = tj * qb_wave_sum(v * a[c]);
                a[c] = fma(-tw, v, a[c]);
            }
        }
        a[j] = lane > j ? v : (lane == j ? beta : a[j]);
    }
    if (lane == j) { tauv = tj; diag = a[j]; }
}

// One wave, column bc of an LDS image <- (I - tj v v^T) bc with v = [1 ; vj(j+1 .. m-1)] at row j: a wave-strided dot product, a
// butterfly, the update.  (bc[j] is read by every lane before lane 0 writes it: the wave runs in lock step up to the butterfly.)
__device__ __forceinline__ void qb_col_reflect(const double* vj, double* bc, int j, int m, double tj, int lane)
{
    double d = 0.0;
    for (int i = j + 1 + lane; i < m; i += 64) d = fma(vj[i], bc[i], d);
    d = qb_wave_sum(d);
    const double tw = tj * (bc[j] + d);
    for (int i = j + 1 + lane; i < m; i += 64) bc[i] = fma(-tw, vj[i], bc[i]);
    if (lane == 0) bc[j] -= tw;
}

// Workgroup route, step j, called by all 256 threads: As[c * ld + i] is the member's image, red four doubles of LDS.  The norm is a
// 256-thread strided sum, the four wave partials added in wave order; wave w then takes columns j + 1 + w, + 4, .. below cend.  Returns
// tau_j to every thread.  The caller closes the step with a barrier of its own (red and column j are then read no more).
__device__ __forceinline__ double qb_wg_col(double* As, int ld, int m, int j, int cend, double* red, int t)
{
    const int lane = t & 63, wv = t >> 6;
    double* vj = As + j * ld;
    double s = 0.0;
    for (int i = j + 1 + t; i < m; i += 256) s = fma(vj[i], vj[i], s);
    s = qb_wave_sum(s);
    if (lane == 0) red[wv] = s;
    __syncthreads();
    const double ssq = ((red[0] + red[1]) + red[2]) + red[3];
    double tj = 0.0;
    if (ssq != 0.0) {                         // (the same value in every thread)
        const double alpha = vj[j];
        double beta, scal;
        tj = qb_larfg(alpha, ssq, beta, scal);
        __syncthreads();                      // (every thread has read alpha and the column)
        for (int i = j + 1 + t; i < m; i += 256) vj[i] *= scal;
        if (t == 0) vj[j] = beta;
        __syncthreads();
        for (int c = j + 1 + wv; c < cend; c += 4) qb_col_reflect(vj, As + c * ld, j, m, tj, lane);
    }
    return tj;
}

// One wave, a column of m rows with row lane + 64 k in c[k] <- (I - tj v v^T) of it, v = [1 ; vj(j+1 .. m-1)] at row j
template <int RR>
__device__ __forceinline__ void qb_regs_reflect(const double* vj, int j, int m, double tj, double (&c)[RR], int lane)
{
    double v[RR];
    double d = 0.0;
#pragma unroll
    for (int k = 0; k < RR; ++k) {
        const int i = lane + 64 * k;
        v[k] = (i > j && i < m) ? vj[i] : (i == j ? 1.0 : 0.0);
        d = fma(v[k], c[k], d);
    }
    const double tw = tj * qb_wave_sum(d);
#pragma unroll
    for (int k = 0; k < RR; ++k) c[k] = fma(-tw, v[k], c[k]);
}

// One thread: x(0 .. r-1) <- R^-1 x over the leading r x r block of R(i, c) = R[c * ldr + i], rows r-1 .. 0
__device__ __forceinline__ void qb_trsv(const double* R, int ldr, int r, double* x)
{
    for (int k = r - 1; k >= 0; --k) {
        double s = x[k];
        for (int l = k + 1; l < r; ++l) s = fma(-R[l * ldr + k], x[l], s);
        x[k] = s / R[k * ldr + k];
    }
}

// One thread: x(0 .. r-1) <- R^-T x, rows 0 .. r-1, each row's sum over l ascending
__device__ __forceinline__ void qb_trsv_t(const double* R, int ldr, int r, double* x)
{
    for (int k = 0; k < r; ++k) {
        double s = x[k];
        for (int l = 0; l < k; ++l) s = fma(-R[k * ldr + l], x[l], s);
        x[k] = s / R[k * ldr + k];
    }
}

// info: 0, or i + 1 for the smallest i with R(i, i) == 0 exactly.  One wave, d = R(lane, lane) in lanes < n <= 64 ..
__device__ __forceinline__ int qb_info_wave(double d, int n, int lane)
{
    const unsigned long long z = __ballot(lane < n && d == 0.0);
    return z ? __ffsll((long long) z) : 0;
}

// .. or one thread over the image
__device__ __forceinline__ int qb_info_serial(const double* R, int ldr, int n)
{
    int inf = 0;
    for (int i = n - 1; i >= 0; --i)
        if (R[i * ldr + i] == 0.0) inf = i + 1;
    return inf;
}

// More than 64 KiB of LDS per workgroup has to be allowed per kernel and device, once: `done` is the calling file's own record of the
// devices on which every kernel of its table `fns` has been allowed.  Returns 0 or the HIP error.
template <size_t N>
static inline int qb_allow_lds(const void* const (&fns)[N], std::atomic<int> (&done)[64])
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int) e;
    if (dev >= 0 && dev < 64 && done[dev].load(std::memory_order_acquire)) return 0;
    for (const void* f : fns) {
        e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, QB_LDS_CAP);
        if (e != hipSuccess) return (int) e;
    }
    if (dev >= 0 && dev < 64) done[dev].store(1, std::memory_order_release);
    return 0;
}

#endif
