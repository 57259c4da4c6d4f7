// qr_batched_trust.hip -- kernels of the batched trust-region step (qr_batched_trust.c, mi355x_qr.h section 8g): per member, given the
// factors A = Q R, z = the top of Q^T b, D = diag(d) and a radius Delta > 0, the lambda >= 0 and x = argmin |A x - b|^2 + lambda^2 |D x|^2
// with either lambda = 0 and |D x| <= (1 + rtol) Delta, or | |D x| - Delta | <= rtol Delta.  MINPACK lmpar (More 1978) with par = lambda^2,
// written from its description: the Gauss-Newton step, the bounds parl and paru, then Newton steps on par, each one elimination of
// sqrt(par) D against the untouched master (bd_wave_elim / bd_wg_elim of qr_batched_dev.h: the code qr_batched_damped.hip runs, so X,
// xnorm and resid are bitwise the damped solve of the lambda returned), a back substitution, and a forward substitution with R~^T for
// the correction.  The whole search of a member runs inside one launch; members leave their loops independently.
//
//   bt_wave_kernel<W>        n + 1 <= W <= 32: one wave per member, four per workgroup, no barrier.  bd_wave_kernel's layout: lane i holds
//                            row i of the master [R | z], of the working copy and of the block; R~ and z~ go through the wave's LDS for
//                            qb_trsv, and qb_trsv_t reads the same image.  Every loop decision is taken on butterfly results: the same
//                            value in all lanes of the wave
//   bt_fused_wave_kernel<W>  m <= 64, n + 1 <= W: bd_wave_factor (b_wave_kernel's factorisation of [A | b]), then the same search
//   bt_wg_kernel             n <= 63 otherwise: one workgroup per member, bd_wg_kernel's three LDS images; thread 0 publishes every decision
//                            (accept, lambda, status) in an LDS word that all threads read after a barrier
//
// Per member: info = -1 for a Delta that is not a finite positive number, i + 1 for the smallest i with R~(i,i) == 0 exactly in an
// elimination, and then nothing else is written; else info = 0, lambda, X, |D x|, resid, the number of eliminations and status
// (0 converged, 1 Gauss-Newton step accepted, 2 left by the lower-bound clause, 3 maxit reached).
//
// A column with d == 0 contributes nothing to the gradient bound g (its quotient is not formed); what the elimination then finds on
// the diagonal decides its info word as in section 8f.
#include "qr_batched_trust_dev.h"

static_assert(QRD_B_MAX_N == 64, "one lane per row of the triangle");

// The state, the search bodies (bt_wave_core, bt_wg_core) and their helpers live in qr_batched_trust_dev.h, which qr_batched_lm.hip
// includes as well; the kernels below read the radius and the starting guess and write the outputs.

template <int W>
__device__ __forceinline__ void bt_wave_search(const double (&r)[W], const qrd_bt_args& a, size_t q, int lane, const bd_lane& L, double* Rs,
                                               double* Xs)
{
    const qrd_bd_args& d = a.d;
    const int n = d.n;
    const double delta = a.delta[q * a.sdelta], rtol = a.rtol;
    if (!bt_delta_ok(delta)) {                // (wave-uniform)
        if (lane == 0) d.info[q] = -1;
        return;
    }
    const double lam0 = a.lam0 ? a.lam0[q * a.slam0] : 0.0;
    double zl;
    bt_found F;
    const double xi = bt_wave_core<W>(r, n, lane, L.dsc, delta, lam0 * lam0, rtol, a.maxit, Rs, Xs, zl, F);
    if (F.info) {                             // (wave-uniform: nothing else is written for this member)
        if (lane == 0) d.info[q] = F.info;
        return;
    }
    // the outputs, as bd_wave_lams writes them for one lambda and one right-hand side
    double* xc = d.X + q * d.sX;
    if (lane < n) xc[L.perm] = xi;
    for (int i = n + lane; i < d.xrows; i += 64) xc[i] = 0.0;
    if (d.resid) {
        double t = -zl;                       // row lane of R x - z, the sum over the columns ascending (zeros below the diagonal)
#pragma unroll
        for (int cc = 0; cc < W; ++cc)
            if (cc < n) t = fma(r[cc], Xs[cc], t);
        t = lane < n ? t : 0.0;
        const double s2 = bd_wave_dot(t, t);
        const double rs = qb_bcast(L.rss, 0);
        if (lane == 0) d.resid[q] = sqrt(s2 + rs);
    }
    if (lane == 0) {
        d.info[q] = 0;
        a.lam[q] = F.lam;
        if (d.xnorm) d.xnorm[q] = F.dxnorm;
        if (a.iter) a.iter[q] = F.it;
        if (a.status) a.status[q] = F.status;
    }
}

template <int W>
__global__ void __launch_bounds__(256) bt_wave_kernel(const qrd_bt_args a)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) a.d.batch) return;      // (no workgroup barrier below: the waves of a workgroup are independent)
    bd_lane L;
    bd_lane_setup(a.d, q, lane, L);
    double r[W];
    bd_wave_load<W>(a.d, q, lane, r, L);
    constexpr int LW = W + 1;
    double* Rs = sm + (size_t) wv * 2 * W * LW;
    bt_wave_search<W>(r, a, q, lane, L, Rs, Rs + W * LW);
}

// the factorisation of b_wave_kernel, then the search.  a.d.Z is b (m rows, ldz >= m), written back as Q^T b in all rows.
template <int W>
__global__ void __launch_bounds__(256) bt_fused_wave_kernel(double* __restrict__ A, int m, int lda, size_t strideA, double* __restrict__ tau,
                                                            size_t stridetau, double* __restrict__ B, const qrd_bt_args a)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) a.d.batch) return;      // (no workgroup barrier below)
    bd_lane L;
    double r[W];
    bd_wave_factor<W>(A + q * strideA, m, lda, tau + q * stridetau, B + q * a.d.sZ, a.d, q, lane, r, L);
    constexpr int LW = W + 1;
    double* Rs = sm + (size_t) wv * 2 * W * LW;
    bt_wave_search<W>(r, a, q, lane, L, Rs, Rs + W * LW);
}

__global__ void __launch_bounds__(256) bt_wg_kernel(const qrd_bt_args a)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const qrd_bd_args& d = a.d;
    const int n = d.n, ntot = n + 1, ld = bd_ld(n);
    double* Ms = sm;
    double* Ws = Ms + (size_t) ntot * ld;
    double* Ss = Ws + (size_t) ntot * ld;
    double* dsc = Ss + (size_t) ntot * ld;
    double* rssv = dsc + 64;
    int* perm = (int*) (rssv + 64);
    int* sinfo = perm + 64;                   // sinfo[0]: info of an elimination, sinfo[1]: nsing
    double* sdec = rssv + 1;                  // the decisions, published by thread 0 (one right-hand side: only rssv[0] is taken)
    const double* xs = Ws + (size_t) n * ld;
    const double delta = a.delta[q * a.sdelta], rtol = a.rtol;
    if (!bt_delta_ok(delta)) {                // (the same word in every thread)
        if (t == 0) d.info[q] = -1;
        return;
    }
    const double lam0 = a.lam0 ? a.lam0[q * a.slam0] : 0.0;
    bd_wg_load(d, q, t, Ms, ld, dsc, rssv, perm);
    bt_found F;
    bt_wg_core(Ms, Ws, Ss, dsc, sdec, sinfo, n, ld, delta, lam0 * lam0, rtol, a.maxit, t, F);
    if (F.info) {                             // (the same word in every thread: nothing else is written for this member)
        if (t == 0) d.info[q] = F.info;
        return;
    }
    if (wv == 0) {                            // the outputs, as bd_wg_kernel writes them for one lambda and one right-hand side
        double* xc = d.X + q * d.sX;
        const double xi = lane < n ? xs[lane] : 0.0;
        if (lane < n) xc[perm[lane]] = xi;
        for (int i = n + lane; i < d.xrows; i += 64) xc[i] = 0.0;
        if (d.resid) {
            double e = 0.0;
            if (lane < n) {
                e = -Ms[n * ld + lane];
                for (int cc = lane; cc < n; ++cc) e = fma(Ms[cc * ld + lane], xs[cc], e);
            }
            const double s2 = bd_wave_dot(e, e);
            if (lane == 0) d.resid[q] = sqrt(s2 + rssv[0]);
        }
        if (lane == 0) {
            d.info[q] = 0;
            a.lam[q] = F.lam;
            if (d.xnorm) d.xnorm[q] = F.dxnorm;
            if (a.iter) a.iter[q] = F.it;
            if (a.status) a.status[q] = F.status;
        }
    }
}

// the kernels that may ask for more than 64 KiB of LDS (qr_allow_lds)
static int bt_allow_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(bt_wg_kernel), reinterpret_cast<const void*>(bt_wave_kernel<32>),
                               reinterpret_cast<const void*>(bt_fused_wave_kernel<32>)};
    return qr_allow_lds(fns, QB_LDS_CAP, done);
}

static int bt_bad_args(const qrd_bt_args* a)
{
    const qrd_bd_args* d = &a->d;
    return d->n < 1 || d->n + 1 > QRD_B_MAX_N || d->nrhs != 1 || d->nlam != 1 || !d->Z || !d->X || !d->info || d->zrows < d->n || d->xrows < d->n ||
           d->ldz < d->zrows || d->ldx < d->xrows || (d->flip && (d->D || d->jpvt)) || !a->delta || !a->lam || !(a->rtol > 0.0 && a->rtol < 1.0) ||
           a->maxit < 1;
}

extern "C" {

// the trust-region step of every member from factors that exist: one launch.  -7: shape not taken
int qrd_bt_solve(void* stream, const qrd_bt_args* a)
{
    if (!a || a->d.batch <= 0) return 0;
    if (bt_bad_args(a) || !a->d.R || a->d.ldr < a->d.n) return -7;
    const int rc = bt_allow_lds();
    if (rc) return rc;
    hipStream_t s = (hipStream_t) stream;
    const int ntot = a->d.n + 1;
    if (qrd_bd_wave_route(ntot)) {
        const dim3 grid((unsigned) (((size_t) a->d.batch + 3) / 4));
        if (ntot <= 4) hipLaunchKernelGGL(bt_wave_kernel<4>, grid, dim3(256), bt_wave_lds<4>(), s, *a);
        else if (ntot <= 8) hipLaunchKernelGGL(bt_wave_kernel<8>, grid, dim3(256), bt_wave_lds<8>(), s, *a);
        else if (ntot <= 16) hipLaunchKernelGGL(bt_wave_kernel<16>, grid, dim3(256), bt_wave_lds<16>(), s, *a);
        else hipLaunchKernelGGL(bt_wave_kernel<32>, grid, dim3(256), bt_wave_lds<32>(), s, *a);
    } else {
        hipLaunchKernelGGL(bt_wg_kernel, dim3((unsigned) a->d.batch), dim3(256), bd_wg_lds(a->d.n, ntot), s, *a);
    }
    return (int) hipGetLastError();
}

// factor [A | b] (m <= 64 rows, n + 1 <= 32 columns) and search in one launch: A, tau as qrd_b_geqrf leaves them, b <- Q^T b in all
// rows.  a->d.Z is not referenced (B, a->d.ldz >= m and a->d.sZ describe the right-hand side); a->d.R, rss, jpvt and flip must be unset.
// -7: shape not taken
int qrd_bt_fused(void* stream, double* A, int m, int lda, size_t strideA, double* tau, size_t stridetau, double* B, const qrd_bt_args* a)
{
    if (!a || a->d.batch <= 0) return 0;
    qrd_bt_args b = *a;
    b.d.Z = B;
    b.d.zrows = b.d.n;
    if (bt_bad_args(&b) || !A || !tau || !B || m < a->d.n || m > 64 || !qrd_bd_wave_route(a->d.n + 1) || lda < m || a->d.ldz < m || a->d.R ||
        a->d.rss || a->d.jpvt || a->d.flip)
        return -7;
    const int rc = bt_allow_lds();
    if (rc) return rc;
    hipStream_t s = (hipStream_t) stream;
    const int ntot = a->d.n + 1;
    const dim3 grid((unsigned) (((size_t) a->d.batch + 3) / 4));
#define BT_FUSED(W) hipLaunchKernelGGL(bt_fused_wave_kernel<W>, grid, dim3(256), bt_wave_lds<W>(), s, A, m, lda, strideA, tau, stridetau, B, b)
    if (ntot <= 4) BT_FUSED(4);
    else if (ntot <= 8) BT_FUSED(8);
    else if (ntot <= 16) BT_FUSED(16);
    else BT_FUSED(32);
#undef BT_FUSED
    return (int) hipGetLastError();
}

}   // extern "C"
