// qr_batched_dev.h -- the device code that the batched kernel files (qr_batched.hip, qr_batched_update.hip, qr_batched_minnorm.hip,
// qr_batched_svd.hip, qr_batched_damped.hip, qr_batched_trust.hip, qr_batched_lse.hip, qr_batched_bvls.hip, qr_batched_irls.hip, qr_batched_stats.hip, qr_batched_lsei.hip) share: the wave helpers, the dlarfg scalars, the Householder column step of the wave route and of the workgroup
// route, one reflector on a column in registers, the triangular solves over an LDS image, the info word, the elimination of a damping block (shared by the damped and the
// trust-region kernels; the search itself, which qr_batched_lm.hip runs as well, is qr_batched_trust_dev.h), and the LDS cap.  No
// kernels, no entry points.  Two kernels that call the same step here run the same operations in the same order: that is what makes
// the factors and tau of qrd_b_geqrf, qrd_b_geqp3 (on the permuted columns) and qrd_bm_fused equal bit for bit on the same route.
//
// Every sum runs in a fixed order (wave butterflies, waves added in wave order, serial loops).  No atomics.
#ifndef QR_BATCHED_DEV_H
#define QR_BATCHED_DEV_H

#include <float.h>

#include "qr_common.h"
#include "qr_device.h"

#define QB_LDS_CAP (160 * 1024)           // what one workgroup may hold, once allowed (qr_allow_lds, qr_common.h)
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

// LAPACK dlarfg's scalars from alpha and xnorm = |x| != 0: returns tau; v = x * scal
__device__ __forceinline__ double qb_larfg_n(double alpha, double xnorm, double& beta, double& scal)
{
    beta = -copysign(hypot(alpha, xnorm), alpha);
    scal = 1.0 / (alpha - beta);
    return (beta - alpha) / beta;
}

// .. from alpha and ssq = |x|^2 != 0
__device__ __forceinline__ double qb_larfg(double alpha, double ssq, double& beta, double& scal)
{
    return qb_larfg_n(alpha, sqrt(ssq), beta, scal);
}

// The norm of a column from the plain sum of its squares.  A column of the data's own size squares into the double range wherever the
// data is inside 1e+-150, but a column that cancellation has left at rounding size (a dependent column behind the pivots) lies sixteen
// digits below the data, and from data of about 1e-145 its squares are subnormal: the sum keeps a few bits, and beta and tau belong to no
// reflector.  While the plain sum lies inside QB_SSQ_LO .. QB_SSQ_HI its square root is the norm, bit for bit what the step always formed
// (a term that went subnormal is then below 2^-100 of the sum).  Outside it the column is scaled by the power of two that brings its
// largest entry into [1, 2) and summed again in the same order -- exact, so wherever no term of the plain sum overflows or goes subnormal
// the result keeps the plain sum's bits as well.  A largest entry that is 0 or no finite number takes the plain sum.
#define QB_SSQ_LO 0x1p-900
#define QB_SSQ_HI 0x1p+900
__device__ __forceinline__ bool qb_ssq_plain(double ssq) { return ssq >= QB_SSQ_LO && ssq <= QB_SSQ_HI; }

__device__ __forceinline__ double qb_wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// one wave, lane i holding x_i (0 in the lanes that hold none) and every lane ssq = qb_wave_sum(x * x): |x|, the same word in every lane
__device__ __forceinline__ double qb_wave_nrm(double x, double ssq)
{
    if (qb_ssq_plain(ssq)) return sqrt(ssq);
    const double xmax = qb_wave_max(fabs(x));
    if (xmax == 0.0 || !(xmax <= DBL_MAX)) return sqrt(ssq);
    const int e = ilogb(xmax);
    const double xs = ldexp(x, -e);
    return ldexp(sqrt(qb_wave_sum(xs * xs)), e);
}

// Wave route, step j (wave-uniform, j < the columns factored): lane i holds row i of the member in a[], rows past the last hold zeros.
// Column j becomes beta on and v below the diagonal, columns j+1 .. cend-1 (cend wave-uniform) take the reflector; lane j keeps tau_j
// in tauv and R(j, j) in diag.  x == 0 exactly: tau = 0, nothing changes.  Once the caller's loop over j is unrolled (or j is a template
// constant there) every index into a[] is a constant.
template <int W>
__device__ __forceinline__ void qb_wave_col(double (&a)[W], int j, int cend, int lane, double& tauv, double& diag)
{
    const double x = lane > j ? a[j] : 0.0;
    const double xnorm = qb_wave_nrm(x, qb_wave_sum(x * x));
    const double alpha = __shfl(a[j], j);
    double tj = 0.0;
    if (xnorm != 0.0) {
        double beta, scal;
        tj = qb_larfg_n(alpha, xnorm, beta, scal);
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
    double xnorm = sqrt(ssq);
    if (!qb_ssq_plain(ssq)) {                 // (the same value in every thread: the barriers below are met by all or by none)
        double xmax = 0.0;
        for (int i = j + 1 + t; i < m; i += 256) xmax = fmax(xmax, fabs(vj[i]));
        xmax = qb_wave_max(xmax);
        __syncthreads();                      // (every thread has read the four partial sums)
        if (lane == 0) red[wv] = xmax;
        __syncthreads();
        xmax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        if (xmax != 0.0 && xmax <= DBL_MAX) {
            const int e = ilogb(xmax);
            s = 0.0;
            for (int i = j + 1 + t; i < m; i += 256) {
                const double xs = ldexp(vj[i], -e);
                s = fma(xs, xs, s);
            }
            s = qb_wave_sum(s);
            __syncthreads();                  // (every thread has read the four maxima)
            if (lane == 0) red[wv] = s;
            __syncthreads();
            xnorm = ldexp(sqrt(((red[0] + red[1]) + red[2]) + red[3]), e);
        }
    }
    double tj = 0.0;
    if (xnorm != 0.0) {                       // (the same value in every thread)
        const double alpha = vj[j];
        double beta, scal;
        tj = qb_larfg_n(alpha, xnorm, beta, scal);
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

// ---------------------------------------------------------------------------------------------------------------------------------
// What the damped kernels (qr_batched_damped.hip) and the trust-region search (qr_batched_trust.hip) share: the per-lane operands, the
// loads of the master [R | Z], the factorisation in front of a fused launch, and the elimination of one lambda D against the triangle.
// Both files run the elimination below, so a trust-region result is bitwise the damped solve of the lambda it returns.
// ---------------------------------------------------------------------------------------------------------------------------------

// what a lane needs beside its rows: d of its column (through jpvt), the row of X its x goes to, and rss of right-hand side `lane`
struct bd_lane {
    double dsc, rss;
    int perm;
};

// lane < n: jp = jpvt[lane] (clamped into the block: a jpvt that is none of geqp3's must not carry a store out of it)
__device__ __forceinline__ void bd_lane_setup(const qrd_bd_args& a, size_t q, int lane, bd_lane& L)
{
    const int n = a.n;
    int jp = lane < n ? lane : 0;
    if (a.jpvt && lane < n) {
        const int v = a.jpvt[q * a.sj + lane];
        if (v >= 0 && v < n) jp = v;
    }
    L.dsc = (a.D && lane < n) ? a.D[q * a.sD + jp] : 1.0;
    L.perm = a.flip ? n - 1 - lane : jp;
    L.rss = (a.rss && lane < a.nrhs) ? a.rss[q * (size_t) a.nrhs + lane] : 0.0;
}

// The sum over the wave of a * b, every rounding written out: the products rounded, the first butterfly step one fma on the lane's own
// exact product, then additions.  With contraction left to the compiler the same source line is fused in one kernel and not in another;
// the damped kernels and the search must round alike, so the steps below and the norms of their outputs leave it nothing to decide.
__device__ __forceinline__ double bd_wave_dot(double a, double b)
{
#pragma clang fp contract(off)
    const double p = a * b;
    double v = fma(a, b, __shfl_xor(p, 32));
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}

// Wave route, one lambda: w <- the master r (lane i: row i of [R | Z], zeros below the diagonal and in lanes >= n) with the block
// [S | 0], S(lane, lane) = sd, eliminated against it.  Every index into the arrays is a constant once the loops are unrolled.
template <int W>
__device__ __forceinline__ void bd_wave_elim(const double (&r)[W], double sd, int n, int ntot, int lane, double (&w)[W])
{
#pragma clang fp contract(off)
    double s[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
        w[c] = r[c];
        s[c] = (c < n && lane == c) ? sd : 0.0;
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
        if (j < n) {                      // (wave-uniform)
            const double x = s[j];        // (rows > j of the block's column j are exact zeros)
            const double ssq = bd_wave_dot(x, x);
            if (ssq != 0.0) {             // (the same value in every lane)
                const double alpha = qb_bcast(w[j], j);
                double beta, scal;
                const double tj = qb_larfg(alpha, ssq, beta, scal);
                const double v = x * scal;
#pragma unroll
                for (int c = j + 1; c < W; ++c) {
                    if (c < ntot) {
                        const double t = qb_bcast(w[c], j) + bd_wave_dot(v, s[c]);
                        const double tw = tj * t;
                        if (lane == j) w[c] = fma(-tj, t, w[c]);
                        s[c] = fma(-tw, v, s[c]);
                    }
                }
                if (lane == j) w[j] = beta;
            }
        }
    }
}

// Wave route: the master of member q from R, Z (flip: U(i, c) = R(n-1-c, n-1-i), z reversed) and the tail of Q^T b into L.rss
template <int W>
__device__ __forceinline__ void bd_wave_load(const qrd_bd_args& a, size_t q, int lane, double (&r)[W], bd_lane& L)
{
    const int n = a.n, nrhs = a.nrhs, ntot = n + nrhs;
    const double* Rq = a.R + q * a.sR;
    const double* Zq = a.Z + q * a.sZ;
    const int src = a.flip ? n - 1 - lane : lane;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        double v = 0.0;
        if (lane < n && c < n) {
            if (lane <= c) v = a.flip ? Rq[(size_t) src * a.ldr + (n - 1 - c)] : Rq[(size_t) c * a.ldr + lane];      // (the strict lower triangle is not read)
        } else if (lane < n && c < ntot) {
            v = Zq[(size_t) (c - n) * a.ldz + src];
        }
        r[c] = v;
    }
    if (a.zrows > n) {                        // the tail of Q^T b: rows n .. zrows-1 of every right-hand side
        for (int kk = 0; kk < nrhs; ++kk) {
            const double* zc = Zq + (size_t) kk * a.ldz;
            double t = 0.0;
            for (int i = n + lane; i < a.zrows; i += 64) t = fma(zc[i], zc[i], t);
            t = qb_wave_sum(t);
            if (lane == kk) L.rss += t;
        }
    }
}

// Wave route, fused launch: b_wave_kernel's factorisation of [A | B] (m <= 64 rows), A, tau and Q^T B stored, the master left in r and
// the tail sums in L.rss.  Bq: the member's B (ldz >= m)
template <int W>
__device__ __forceinline__ void bd_wave_factor(double* Aq, int m, int lda, double* tauq, double* Bq, const qrd_bd_args& a, size_t q, int lane,
                                               double (&r)[W], bd_lane& L)
{
    const int n = a.n, nrhs = a.nrhs, ntot = n + nrhs;
    const bool row = lane < m;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        double v = 0.0;
        if (row && c < n) v = Aq[(size_t) c * lda + lane];
        else if (row && c < ntot) v = Bq[(size_t) (c - n) * a.ldz + lane];
        r[c] = v;
    }
    double tauv = 0.0, diag = 1.0;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        if (j < n) qb_wave_col<W>(r, j, ntot, lane, tauv, diag);      // (wave-uniform; B's columns ride along)
    }
    bd_lane_setup(a, q, lane, L);
    L.rss = 0.0;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        if (c < n) {
            if (row) Aq[(size_t) c * lda + lane] = r[c];
            r[c] = (lane < n && lane <= c) ? r[c] : 0.0;         // the master: R alone, V and the rows below it gone
        } else if (c < ntot) {
            if (row) Bq[(size_t) (c - n) * a.ldz + lane] = r[c];
            const double y = lane >= n ? r[c] : 0.0;             // (rows >= m hold zeros)
            const double t = qb_wave_sum(y * y);
            if (lane == c - n) L.rss = t;
            r[c] = lane < n ? r[c] : 0.0;
        }
    }
    if (lane < n) tauq[lane] = tauv;
}

// Workgroup route.  LDS: Ms, Ws, Ss (n x (n + nrhs) each at ld = bd_ld(n): the master [R | Z], the working copy, the block), then
// dsc[64], rss[64], perm[64] (ints), two words.
__host__ __device__ constexpr int bd_ld(int n) { return n | 1; }
__host__ __device__ constexpr size_t bd_wg_lds(int n, int ntot) { return sizeof(double) * (3 * (size_t) ntot * bd_ld(n) + 2 * 64 + 32 + 2); }
static_assert(bd_wg_lds(63, 64) <= QB_LDS_CAP && bd_wg_lds(32, 64) <= QB_LDS_CAP, "the three images fit");

// all 256 threads: the master, dsc, perm and rss (the tail of Q^T b added) of member q.  Ends without a barrier after the tail sums.
__device__ __forceinline__ void bd_wg_load(const qrd_bd_args& a, size_t q, int t, double* Ms, int ld, double* dsc, double* rssv, int* perm)
{
    const int lane = t & 63, wv = t >> 6;
    const int n = a.n, nrhs = a.nrhs, ntot = n + nrhs;
    const double* Rq = a.R + q * a.sR;
    const double* Zq = a.Z + q * a.sZ;
    for (int idx = t; idx < ntot * n; idx += 256) {
        const int c = idx / n, i = idx - c * n;
        const int src = a.flip ? n - 1 - i : i;
        double v = 0.0;
        if (c >= n) v = Zq[(size_t) (c - n) * a.ldz + src];
        else if (i <= c) v = a.flip ? Rq[(size_t) src * a.ldr + (n - 1 - c)] : Rq[(size_t) c * a.ldr + i];
        Ms[c * ld + i] = v;
    }
    if (wv == 0) {                            // (n, nrhs < 64: one lane each)
        bd_lane L;
        bd_lane_setup(a, q, lane, L);
        dsc[lane] = L.dsc;
        perm[lane] = L.perm;
        rssv[lane] = L.rss;
    }
    __syncthreads();
    if (a.zrows > n) {
        for (int kk = wv; kk < nrhs; kk += 4) {
            const double* zc = Zq + (size_t) kk * a.ldz;
            double s = 0.0;
            for (int i = n + lane; i < a.zrows; i += 64) s = fma(zc[i], zc[i], s);
            s = qb_wave_sum(s);
            if (lane == 0) rssv[kk] += s;
        }
    }
}

// Workgroup route, one lambda, all 256 threads: Ws <- Ms, Ss <- [lam diag(dsc) | 0], the block eliminated against Ws.  Opens with a
// barrier (the images of the previous lambda are read no more; dsc is written); R~(n-1, n-1) is written by thread 0 after the last one.
__device__ __forceinline__ void bd_wg_elim(const double* Ms, double* Ws, double* Ss, const double* dsc, double lam, int n, int ntot, int ld, int t)
{
#pragma clang fp contract(off)                // (every rounding written out, as in bd_wave_elim)
    const int lane = t & 63, wv = t >> 6;
    __syncthreads();
    for (int idx = t; idx < ntot * n; idx += 256) {
        const int c = idx / n, i = idx - c * n;
        Ws[c * ld + i] = Ms[c * ld + i];
        Ss[c * ld + i] = (c == i) ? lam * dsc[i] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        // every wave forms the norm and the scalars from the same LDS words: the same values in all 256 threads
        const double x = lane <= j ? Ss[j * ld + lane] : 0.0;
        const double ssq = bd_wave_dot(x, x);
        double beta = 0.0;
        if (ssq != 0.0) {
            const double alpha = Ws[j * ld + j];
            double scal;
            const double tj = qb_larfg(alpha, ssq, beta, scal);
            const double v = x * scal;
            for (int c = j + 1 + wv; c < ntot; c += 4) {     // wave wv: columns j + 1 + wv, + 4, ..
                double* sc = Ss + c * ld;
                const double sv = lane <= j ? sc[lane] : 0.0;
                const double tw = tj * (Ws[c * ld + j] + bd_wave_dot(v, sv));
                if (lane <= j) sc[lane] = fma(-tw, v, sv);
                if (lane == 0) Ws[c * ld + j] = Ws[c * ld + j] - tw;        // (read by every lane above: the wave runs in lock step up to the butterfly)
            }
        }
        __syncthreads();                  // (alpha and column j of the block are read no more)
        if (t == 0 && ssq != 0.0) Ws[j * ld + j] = beta;    // (read next by thread 0 below, by the others after a barrier)
    }
}

#endif
