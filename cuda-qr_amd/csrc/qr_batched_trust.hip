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
#include <cfloat>

#include "qr_batched_dev.h"

static_assert(QRD_B_MAX_N == 64, "one lane per row of the triangle");

// a radius the search can run on
__device__ __forceinline__ bool bt_delta_ok(double delta) { return delta > 0.0 && delta <= DBL_MAX; }

// the bounds and the start of the iteration from the Gauss-Newton step (the same values in every thread): fp > rtol * delta on entry
struct bt_state {
    double par, parl, paru, fp;
};

// wnorm: |w| with R^T w = D^2 x / |D x| when R has full rank, else unused
__device__ __forceinline__ void bt_start(bt_state& S, bool fullrank, double wnorm, double gnorm, double dxnorm, double delta, double lam0)
{
    S.parl = fullrank ? ((S.fp / delta) / wnorm) / wnorm : 0.0;
    S.paru = gnorm / delta;
    if (S.paru == 0.0) S.paru = DBL_MIN / fmin(delta, 0.1);
    S.par = fmin(fmax(lam0 * lam0, S.parl), S.paru);
    if (S.par == 0.0) S.par = gnorm / dxnorm;
}

// after an elimination and its solve: 0, 1 (never here), 2, 3, or -1 to go on
__device__ __forceinline__ int bt_leave(const bt_state& S, double fpprev, double delta, double rtol, int it, int maxit)
{
    if (fabs(S.fp) <= rtol * delta) return 0;
    if (S.parl == 0.0 && S.fp <= fpprev && fpprev < 0.0) return 2;
    if (it >= maxit) return 3;
    return -1;
}

// the Newton correction: wnorm = |w| with R~^T w = D^2 x / |D x|
__device__ __forceinline__ void bt_update(bt_state& S, double wnorm, double delta)
{
    const double parc = ((S.fp / delta) / wnorm) / wnorm;
    if (S.fp > 0.0) S.parl = fmax(S.parl, S.par);
    if (S.fp < 0.0) S.paru = fmin(S.paru, S.par);
    S.par = fmax(S.parl, S.par + parc);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// wave route.  r[]: lane i < n holds row i of the master [R | z] (z in column n), zeros below the diagonal and in lanes >= n.  Rs: this
// wave's image of the triangle (W x (W + 1) doubles); Xs: x, then W + 1 doubles on, the vector of the forward substitution.
// ---------------------------------------------------------------------------------------------------------------------------------

// the triangle (columns < n of w) into Rs and column n, rows < rows, into Xs (zeros from there to n); lane 0 solves the leading block
template <int W>
__device__ __forceinline__ double bt_wave_solve(const double (&w)[W], int n, int rows, int lane, double* Rs, double* Xs)
{
    constexpr int LW = W + 1;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        if (c < n) {
            if (lane < n) Rs[c * LW + lane] = w[c];
        } else if (c == n) {
            if (lane < n) Xs[lane] = lane < rows ? w[c] : 0.0;
        }
    }
    QB_WAVE_SYNC();
    if (lane == 0) qb_trsv(Rs, LW, rows, Xs);
    QB_WAVE_SYNC();
    return lane < n ? Xs[lane] : 0.0;
}

// |D x| as bd_wave_lams forms it
__device__ __forceinline__ double bt_wave_dxnorm(double dsc, double xi)
{
    const double dx = dsc * xi;
    return sqrt(bd_wave_dot(dx, dx));
}

// |w|, R^T w = D (D x / |D x|) over the image in Rs
template <int W>
__device__ __forceinline__ double bt_wave_wnorm(int n, int lane, double dsc, double xi, double dxnorm, const double* Rs, double* Us)
{
    constexpr int LW = W + 1;
    if (lane < n) Us[lane] = dsc * ((dsc * xi) / dxnorm);
    QB_WAVE_SYNC();
    if (lane == 0) qb_trsv_t(Rs, LW, n, Us);
    QB_WAVE_SYNC();
    const double wl = lane < n ? Us[lane] : 0.0;
    const double s2 = qb_wave_sum(wl * wl);
    QB_WAVE_SYNC();                           // (Rs and Us are read no more)
    return sqrt(s2);
}

template <int W>
__device__ __forceinline__ void bt_wave_search(const double (&r)[W], const qrd_bt_args& a, size_t q, int lane, const bd_lane& L, double* Rs,
                                               double* Xs)
{
    constexpr int LW = W + 1;
    const qrd_bd_args& d = a.d;
    const int n = d.n;
    const double delta = a.delta[q * a.sdelta], rtol = a.rtol;
    if (!bt_delta_ok(delta)) {                // (wave-uniform)
        if (lane == 0) d.info[q] = -1;
        return;
    }
    const double lam0 = a.lam0 ? a.lam0[q * a.slam0] : 0.0;
    double zl = 0.0, diag = 1.0;              // lane i: z_i and R(i, i)
#pragma unroll
    for (int c = 0; c < W; ++c) {
        zl = c == n ? r[c] : zl;
        if (c < n && lane == c) diag = r[c];
    }
    const int inf0 = qb_info_wave(diag, n, lane);
    const int nsing = inf0 ? inf0 - 1 : n;
    // the Gauss-Newton step: the leading nsing x nsing system, zeros below
    double xi = bt_wave_solve<W>(r, n, nsing, lane, Rs, Xs);
    double dxnorm = bt_wave_dxnorm(L.dsc, xi);
    bt_state S;
    S.fp = dxnorm - delta;
    int it = 0, status = 1;
    double lam = 0.0;
    if (!(S.fp <= rtol * delta)) {
        const double wnorm = nsing == n ? bt_wave_wnorm<W>(n, lane, L.dsc, xi, dxnorm, Rs, Xs + LW) : 0.0;
        double gl = 0.0;                      // lane j: (sum over i <= j of R(i, j) z_i) / d_j
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (c < n) {
                const double t = qb_wave_sum(r[c] * zl);
                if (lane == c) gl = t;
            }
        }
        gl = (lane < n && L.dsc != 0.0) ? gl / L.dsc : 0.0;
        const double gnorm = sqrt(qb_wave_sum(gl * gl));
        bt_start(S, nsing == n, wnorm, gnorm, dxnorm, delta, lam0);
        for (it = 1;; ++it) {
            if (S.par == 0.0) S.par = fmax(DBL_MIN, 0.001 * S.paru);
            lam = sqrt(S.par);
            double w[W];
            bd_wave_elim<W>(r, lam * L.dsc, n, n + 1, lane, w);
            double dg = 1.0;
#pragma unroll
            for (int c = 0; c < W; ++c)
                if (c < n && lane == c) dg = w[c];
            const int inf = qb_info_wave(dg, n, lane);
            if (inf) {                        // (wave-uniform: nothing else is written for this member)
                if (lane == 0) d.info[q] = inf;
                return;
            }
            xi = bt_wave_solve<W>(w, n, n, lane, Rs, Xs);
            dxnorm = bt_wave_dxnorm(L.dsc, xi);
            const double fpprev = S.fp;
            S.fp = dxnorm - delta;
            status = bt_leave(S, fpprev, delta, rtol, it, a.maxit);
            if (status >= 0) break;           // (butterfly results: the same decision in every lane)
            bt_update(S, bt_wave_wnorm<W>(n, lane, L.dsc, xi, dxnorm, Rs, Xs + LW), delta);
        }
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
        a.lam[q] = lam;
        if (d.xnorm) d.xnorm[q] = dxnorm;
        if (a.iter) a.iter[q] = it;
        if (a.status) a.status[q] = status;
    }
}

template <int W>
static constexpr size_t bt_wave_lds() { return sizeof(double) * 4 * 2 * W * (W + 1); }

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

// ---------------------------------------------------------------------------------------------------------------------------------
// workgroup route: the images and words of bd_wg_lds with one right-hand side.  x lives in column n of the working copy, the vector of
// the forward substitution (and g before the loop) in column n of the block, which the elimination leaves unused.
// ---------------------------------------------------------------------------------------------------------------------------------

// every thread: |D x| from the same LDS words, as bd_wg_kernel forms it
__device__ __forceinline__ double bt_wg_dxnorm(const double* dsc, const double* xs, int n, int lane)
{
    const double xi = lane < n ? xs[lane] : 0.0;
    const double dx = lane < n ? dsc[lane] * xi : 0.0;
    return sqrt(bd_wave_dot(dx, dx));
}

// every thread: |w|, R^T w = D (D x / |D x|) over the image T; two barriers inside, one in front
__device__ __forceinline__ double bt_wg_wnorm(const double* T, int ld, int n, const double* dsc, const double* xs, double dxnorm, double* us, int t)
{
    const int lane = t & 63;
    __syncthreads();                          // (us is read no more)
    if (t < n) us[t] = dsc[t] * ((dsc[t] * xs[t]) / dxnorm);
    __syncthreads();
    if (t == 0) qb_trsv_t(T, ld, n, us);
    __syncthreads();
    const double wl = lane < n ? us[lane] : 0.0;
    return sqrt(qb_wave_sum(wl * wl));
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
    double* sdec = rssv + 1;                  // the decisions, published by thread 0 (one right-hand side: only rssv[0] is taken):
                                              // [0] the Gauss-Newton step is accepted, [1] lambda of the coming elimination, [2] status
    double* xs = Ws + (size_t) n * ld;
    double* us = Ss + (size_t) n * ld;
    const double delta = a.delta[q * a.sdelta], rtol = a.rtol;
    if (!bt_delta_ok(delta)) {                // (the same word in every thread)
        if (t == 0) d.info[q] = -1;
        return;
    }
    const double lam0 = a.lam0 ? a.lam0[q * a.slam0] : 0.0;
    bd_wg_load(d, q, t, Ms, ld, dsc, rssv, perm);
    // the Gauss-Newton step: the leading nsing x nsing system of a copy of the master, zeros below
    for (int idx = t; idx < ntot * n; idx += 256) {
        const int c = idx / n, i = idx - c * n;
        Ws[c * ld + i] = Ms[c * ld + i];
    }
    __syncthreads();
    if (t == 0) {
        const int inf0 = qb_info_serial(Ws, ld, n);
        const int ns = inf0 ? inf0 - 1 : n;
        sinfo[1] = ns;
        for (int i = ns; i < n; ++i) xs[i] = 0.0;
        qb_trsv(Ws, ld, ns, xs);
    }
    __syncthreads();
    const int nsing = sinfo[1];
    double dxnorm = bt_wg_dxnorm(dsc, xs, n, lane);
    bt_state S;
    S.fp = dxnorm - delta;
    int it = 0, status = 1;
    double lam = 0.0;
    // Every wave forms the norms below from the same LDS words, but the search runs on thread 0's copy alone: it publishes each
    // decision, and all 256 threads read that word after a barrier.  (With every wave deciding for itself, one member of the tests
    // came back with X one unit in the last place off the damped solve of the lambda returned, from the row down whose diagonal entry
    // of the block another wave had written: the block must hold one lambda, so one thread chooses it.)
    if (t == 0) sdec[0] = S.fp <= rtol * delta ? 1.0 : 0.0;
    __syncthreads();
    if (sdec[0] == 0.0) {
        const double wnorm = nsing == n ? bt_wg_wnorm(Ws, ld, n, dsc, xs, dxnorm, us, t) : 0.0;
        __syncthreads();                      // (us is read no more)
        for (int j = wv; j < n; j += 4) {     // wave wv: g_j = (sum over i <= j of R(i, j) z_i) / d_j for j = wv, wv + 4, ..
            const double p = lane <= j ? Ms[j * ld + lane] * Ms[n * ld + lane] : 0.0;
            const double g = qb_wave_sum(p);
            if (lane == 0) us[j] = dsc[j] != 0.0 ? g / dsc[j] : 0.0;
        }
        __syncthreads();
        const double gl = lane < n ? us[lane] : 0.0;
        const double gnorm = sqrt(qb_wave_sum(gl * gl));
        bt_start(S, nsing == n, wnorm, gnorm, dxnorm, delta, lam0);
        for (it = 1;; ++it) {
            if (S.par == 0.0) S.par = fmax(DBL_MIN, 0.001 * S.paru);
            if (t == 0) sdec[1] = sqrt(S.par);
            __syncthreads();
            lam = sdec[1];
            bd_wg_elim(Ms, Ws, Ss, dsc, lam, n, ntot, ld, t);
            if (t == 0) sinfo[0] = qb_info_serial(Ws, ld, n);
            __syncthreads();
            if (sinfo[0]) {                   // (the same word in every thread: nothing else is written for this member)
                if (t == 0) d.info[q] = sinfo[0];
                return;
            }
            if (t == 0) qb_trsv(Ws, ld, n, xs);
            __syncthreads();
            dxnorm = bt_wg_dxnorm(dsc, xs, n, lane);
            const double fpprev = S.fp;
            S.fp = dxnorm - delta;
            if (t == 0) sdec[2] = (double) bt_leave(S, fpprev, delta, rtol, it, a.maxit);
            __syncthreads();
            status = (int) sdec[2];
            if (status >= 0) break;           // (the same word in every thread)
            bt_update(S, bt_wg_wnorm(Ws, ld, n, dsc, xs, dxnorm, us, t), delta);
        }
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
            a.lam[q] = lam;
            if (d.xnorm) d.xnorm[q] = dxnorm;
            if (a.iter) a.iter[q] = it;
            if (a.status) a.status[q] = status;
        }
    }
}

// the kernels that may ask for more than 64 KiB of LDS (qb_allow_lds)
static int bt_allow_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(bt_wg_kernel), reinterpret_cast<const void*>(bt_wave_kernel<32>),
                               reinterpret_cast<const void*>(bt_fused_wave_kernel<32>)};
    return qb_allow_lds(fns, done);
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
