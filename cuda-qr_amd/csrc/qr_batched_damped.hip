// qr_batched_damped.hip -- kernels of the batched damped least squares (qr_batched_damped.c, mi355x_qr.h section 8f): per member and per
// lambda_k of a list, min |A x - b|^2 + lambda_k^2 |D x|^2 from the factors A = Q R, Z = the top of Q^T b.  MINPACK qrsolv with
// Householder reflectors: the n rows of S = lambda D are eliminated against the n x n triangle R with Z riding along, the L = n case of
// dtpqrt (a triangle stacked on a triangle), then R~ x = z~.  O(n^3) per lambda, the factors untouched.
//
//   bd_wave_kernel<W>        n + nrhs <= W <= 32: one wave per member, four members per workgroup.  Lane i holds row i of the master
//                            [R | Z], of the working copy and of the block [S | 0] in 3 W registers; sums are wave butterflies; no
//                            barrier; the back substitution runs through per-wave LDS as in b_wave_kernel (qr_batched.hip)
//   bd_fused_wave_kernel<W>  m <= 64, n + nrhs <= W: b_wave_kernel's factorisation of [A | B] (qb_wave_col, B riding along), A, tau and
//                            Q^T B stored, then the same lambda loop (bd_wave_lams) on the registers the factors are already in
//   bd_wg_kernel             n + nrhs <= 64 otherwise: one workgroup per member, the three images in LDS at an odd leading dimension
//                            (about 97 KiB at 64 columns); one wave per column per step
//
// The step.  Row i of the block has its non-zeros in columns >= i, so column j of the block lives in rows 0 .. j.  For j = 0 .. n-1,
// x = S(0..j, j), ssq = |x|^2: ssq == 0 exactly gives tau = 0 and touches nothing; otherwise qb_larfg(R(j,j), ssq), and columns
// j+1 .. n+nrhs-1 take the reflector [e_j ; v], the pivot entry in the working copy, the rest in the block (as bu_wave_kernel,
// qr_batched_update.hip, does it).  Every lambda starts from the master again: a result does not depend on nlam or on the position of
// its lambda in the list.  Every sum runs in an order that (n, nrhs) fix; no atomics.
//
// Per (member, lambda): info = 0, or i + 1 for the smallest i with R~(i,i) == 0 exactly, and then nothing else is written for the
// pair; else X (scattered through jpvt, or reversed for flip), xnorm = |D x| and resid = sqrt(|R x - z|^2 + rss) with R x - z formed
// from the master.
#include "qr_batched_dev.h"

static_assert(QRD_B_MAX_N == 64, "one lane per row of the triangle");

// ---------------------------------------------------------------------------------------------------------------------------------
// wave route: the lambda loop.  r[]: lane i < n holds row i of the master [R | Z], zeros below the diagonal and in lanes >= n.  Rs, Xs:
// this wave's LDS, W x (W + 1) doubles each.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int W>
__device__ __forceinline__ void bd_wave_lams(const double (&r)[W], const qrd_bd_args& a, size_t q, int lane, const bd_lane& L, double* Rs,
                                             double* Xs)
{
    constexpr int LW = W + 1;
    const int n = a.n, nrhs = a.nrhs, ntot = n + nrhs, nlam = a.nlam;
    const double* lamq = a.lam + q * a.slam;
    double* Xq = a.X + q * a.sX;
    for (int k = 0; k < nlam; ++k) {
        const double sd = lamq[k] * L.dsc;    // lane j: S(j, j)
        double w[W];
        bd_wave_elim<W>(r, sd, n, ntot, lane, w);
        double diag = 1.0;
#pragma unroll
        for (int c = 0; c < W; ++c)
            if (c < n && lane == c) diag = w[c];
        const int inf = qb_info_wave(diag, n, lane);
        if (lane == 0) a.info[q * (size_t) nlam + k] = inf;
        if (inf) continue;                    // (wave-uniform: nothing else is written for this pair)
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (c < n) {
                if (lane < n) Rs[c * LW + lane] = w[c];
            } else if (c < ntot) {
                if (lane < n) Xs[(c - n) * LW + lane] = w[c];
            }
        }
        QB_WAVE_SYNC();
        if (lane < nrhs) qb_trsv(Rs, LW, n, Xs + lane * LW);      // (nrhs < W <= 32: one lane per right-hand side)
        QB_WAVE_SYNC();
        for (int kk = 0; kk < nrhs; ++kk) {   // (not unrolled: z is picked out of the register file by a select)
            {
                const size_t col = (size_t) k * nrhs + kk;
                double* xc = Xq + col * a.ldx;
                const double xi = lane < n ? Xs[kk * LW + lane] : 0.0;
                if (lane < n) xc[L.perm] = xi;
                for (int i = n + lane; i < a.xrows; i += 64) xc[i] = 0.0;
                if (a.xnorm) {
                    const double dx = L.dsc * xi;
                    const double s2 = bd_wave_dot(dx, dx);
                    if (lane == 0) a.xnorm[q * (size_t) nlam * nrhs + col] = sqrt(s2);
                }
                if (a.resid) {
                    double z = 0.0;
#pragma unroll
                    for (int c = 1; c < W; ++c) z = c == n + kk ? r[c] : z;
                    double t = -z;            // row lane of R x - z, the sum over the columns ascending (zeros below the diagonal)
#pragma unroll
                    for (int cc = 0; cc < W; ++cc)
                        if (cc < n) t = fma(r[cc], Xs[kk * LW + cc], t);
                    t = lane < n ? t : 0.0;
                    const double s2 = bd_wave_dot(t, t);
                    const double rs = qb_bcast(L.rss, kk);
                    if (lane == 0) a.resid[q * (size_t) nlam * nrhs + col] = sqrt(s2 + rs);
                }
            }
        }
        QB_WAVE_SYNC();                       // (Rs and Xs are read no more)
    }
}

template <int W>
__global__ void __launch_bounds__(256) bd_wave_kernel(const qrd_bd_args a)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) a.batch) return;        // (no workgroup barrier below: the waves of a workgroup are independent)
    bd_lane L;
    bd_lane_setup(a, q, lane, L);
    double r[W];
    bd_wave_load<W>(a, q, lane, r, L);
    constexpr int LW = W + 1;
    double* Rs = sm + (size_t) wv * 2 * W * LW;
    bd_wave_lams<W>(r, a, q, lane, L, Rs, Rs + W * LW);
}

// the factorisation of b_wave_kernel, then the lambda loop.  a.Z is B (m x nrhs, ldz >= m), written back as Q^T B in all rows.
template <int W>
__global__ void __launch_bounds__(256) bd_fused_wave_kernel(double* __restrict__ A, int m, int lda, size_t strideA, double* __restrict__ tau,
                                                            size_t stridetau, double* __restrict__ B, const qrd_bd_args a)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) a.batch) return;        // (no workgroup barrier below)
    bd_lane L;
    double r[W];
    bd_wave_factor<W>(A + q * strideA, m, lda, tau + q * stridetau, B + q * a.sZ, a, q, lane, r, L);
    constexpr int LW = W + 1;
    double* Rs = sm + (size_t) wv * 2 * W * LW;
    bd_wave_lams<W>(r, a, q, lane, L, Rs, Rs + W * LW);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// workgroup route: the images and words of bd_wg_lds (qr_batched_dev.h)
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bd_wg_kernel(const qrd_bd_args a)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const int n = a.n, nrhs = a.nrhs, ntot = n + nrhs, nlam = a.nlam, ld = bd_ld(n);
    double* Ms = sm;
    double* Ws = Ms + (size_t) ntot * ld;
    double* Ss = Ws + (size_t) ntot * ld;
    double* dsc = Ss + (size_t) ntot * ld;
    double* rssv = dsc + 64;
    int* perm = (int*) (rssv + 64);
    int* sinfo = perm + 64;
    const double* lamq = a.lam + q * a.slam;
    double* Xq = a.X + q * a.sX;
    bd_wg_load(a, q, t, Ms, ld, dsc, rssv, perm);
    for (int k = 0; k < nlam; ++k) {
        const double lam = lamq[k];
        bd_wg_elim(Ms, Ws, Ss, dsc, lam, n, ntot, ld, t);
        if (t == 0) a.info[q * (size_t) nlam + k] = *sinfo = qb_info_serial(Ws, ld, n);
        __syncthreads();
        if (*sinfo) continue;                 // (the same word in every thread: nothing else is written for this pair)
        if (t < nrhs) qb_trsv(Ws, ld, n, Ws + (size_t) (n + t) * ld);         // (nrhs < 64: one thread per right-hand side)
        __syncthreads();
        for (int kk = wv; kk < nrhs; kk += 4) {
            const double* xs = Ws + (size_t) (n + kk) * ld;
            const size_t col = (size_t) k * nrhs + kk;
            double* xc = Xq + col * a.ldx;
            const double xi = lane < n ? xs[lane] : 0.0;
            if (lane < n) xc[perm[lane]] = xi;
            for (int i = n + lane; i < a.xrows; i += 64) xc[i] = 0.0;
            if (a.xnorm) {
                const double dx = lane < n ? dsc[lane] * xi : 0.0;
                const double s2 = bd_wave_dot(dx, dx);
                if (lane == 0) a.xnorm[q * (size_t) nlam * nrhs + col] = sqrt(s2);
            }
            if (a.resid) {
                double e = 0.0;
                if (lane < n) {
                    e = -Ms[(n + kk) * ld + lane];
                    for (int cc = lane; cc < n; ++cc) e = fma(Ms[cc * ld + lane], xs[cc], e);
                }
                const double s2 = bd_wave_dot(e, e);
                if (lane == 0) a.resid[q * (size_t) nlam * nrhs + col] = sqrt(s2 + rssv[kk]);
            }
        }
    }
}

// the kernels that may ask for more than 64 KiB of LDS (qr_allow_lds)
static int bd_allow_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(bd_wg_kernel), reinterpret_cast<const void*>(bd_wave_kernel<32>),
                               reinterpret_cast<const void*>(bd_fused_wave_kernel<32>)};
    return qr_allow_lds(fns, QB_LDS_CAP, done);
}

static int bd_bad_args(const qrd_bd_args* a)
{
    return a->n < 1 || a->nrhs < 1 || a->n + a->nrhs > QRD_B_MAX_N || a->nlam < 1 || !a->Z || !a->lam || !a->X || !a->info || a->zrows < a->n ||
           a->xrows < a->n || a->ldz < a->zrows || a->ldx < a->xrows || (a->flip && (a->D || a->jpvt));
}

template <int W>
static constexpr size_t bd_wave_lds() { return sizeof(double) * 4 * 2 * W * (W + 1); }

extern "C" {

int qrd_bd_wave_route(int ncols) { return ncols >= 1 && ncols <= 32; }

// the damped solves of every member from factors that exist: one launch.  -7: shape not taken
int qrd_bd_solve(void* stream, const qrd_bd_args* a)
{
    if (!a || a->batch <= 0) return 0;
    if (bd_bad_args(a) || !a->R || a->ldr < a->n) return -7;
    const int rc = bd_allow_lds();
    if (rc) return rc;
    hipStream_t s = (hipStream_t) stream;
    const int ntot = a->n + a->nrhs;
    if (qrd_bd_wave_route(ntot)) {
        const dim3 grid((unsigned) (((size_t) a->batch + 3) / 4));
        if (ntot <= 4) hipLaunchKernelGGL(bd_wave_kernel<4>, grid, dim3(256), bd_wave_lds<4>(), s, *a);
        else if (ntot <= 8) hipLaunchKernelGGL(bd_wave_kernel<8>, grid, dim3(256), bd_wave_lds<8>(), s, *a);
        else if (ntot <= 16) hipLaunchKernelGGL(bd_wave_kernel<16>, grid, dim3(256), bd_wave_lds<16>(), s, *a);
        else hipLaunchKernelGGL(bd_wave_kernel<32>, grid, dim3(256), bd_wave_lds<32>(), s, *a);
    } else {
        hipLaunchKernelGGL(bd_wg_kernel, dim3((unsigned) a->batch), dim3(256), bd_wg_lds(a->n, ntot), s, *a);
    }
    return (int) hipGetLastError();
}

// factor [A | B] (m <= 64 rows, n + nrhs <= 32 columns) and solve for every lambda in one launch: A, tau as qrd_b_geqrf leaves them,
// B <- Q^T B in all rows.  a->Z is not referenced (B, a->ldz >= m and a->sZ describe the right-hand sides); a->R, a->rss, a->jpvt and
// a->flip must be unset.  -7: shape not taken
int qrd_bd_fused(void* stream, double* A, int m, int lda, size_t strideA, double* tau, size_t stridetau, double* B, const qrd_bd_args* a)
{
    if (!a || a->batch <= 0) return 0;
    qrd_bd_args b = *a;
    b.Z = B;
    b.zrows = b.n;
    if (bd_bad_args(&b) || !A || !tau || !B || m < a->n || m > 64 || !qrd_bd_wave_route(a->n + a->nrhs) || lda < m || a->ldz < m || a->R || a->rss ||
        a->jpvt || a->flip)
        return -7;
    const int rc = bd_allow_lds();
    if (rc) return rc;
    hipStream_t s = (hipStream_t) stream;
    const int ntot = a->n + a->nrhs;
    const dim3 grid((unsigned) (((size_t) a->batch + 3) / 4));
#define BD_FUSED(W) hipLaunchKernelGGL(bd_fused_wave_kernel<W>, grid, dim3(256), bd_wave_lds<W>(), s, A, m, lda, strideA, tau, stridetau, B, b)
    if (ntot <= 4) BD_FUSED(4);
    else if (ntot <= 8) BD_FUSED(8);
    else if (ntot <= 16) BD_FUSED(16);
    else BD_FUSED(32);
#undef BD_FUSED
    return (int) hipGetLastError();
}

}   // extern "C"
