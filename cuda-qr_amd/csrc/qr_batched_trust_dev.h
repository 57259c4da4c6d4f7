// qr_batched_trust_dev.h -- the trust-region search (MINPACK lmpar with par = lambda^2) that qr_batched_trust.hip (mi355x_qr.h section 8g)
// and qr_batched_lm.hip (section 8m) both run: bt_state, bt_start, bt_leave, bt_update and the search bodies of the wave route and of the
// workgroup route with their helpers.  No kernels, no entry points.  The bodies are parametrised by where the scaling (dsc), the radius
// (delta) and the starting par come from and by where the step goes: they take the three as values and leave the step, its norm, par and
// the counters in a bt_found, the step also in LDS; what is read from and written to memory is the calling kernel's business.  Both
// files run the code below, so the step of section 8m is bitwise the step section 8g returns on the same factors, scaling, radius and start.
//
// Every elimination is bd_wave_elim / bd_wg_elim of qr_batched_dev.h (the code qr_batched_damped.hip runs).
#ifndef QR_BATCHED_TRUST_DEV_H
#define QR_BATCHED_TRUST_DEV_H

#include <cfloat>

#include "qr_batched_dev.h"

// a radius the search can run on
__device__ __forceinline__ bool bt_delta_ok(double delta) { return delta > 0.0 && delta <= DBL_MAX; }

// the bounds and the start of the iteration from the Gauss-Newton step (the same values in every thread): fp > rtol * delta on entry
struct bt_state {
    double par, parl, paru, fp;
};

// what a search leaves (the same values in every lane of the wave route; thread 0's in the workgroup route, published through LDS):
// info = 0, or i + 1 for the smallest i with R~(i,i) == 0 exactly in an elimination, and then nothing else holds.  lam = sqrt(par), the
// lambda of the last elimination (0: the Gauss-Newton step); dxnorm = |D x|; it: the eliminations run; status: 0 converged, 1 Gauss-Newton
// step accepted, 2 left by the lower-bound clause, 3 maxit reached
struct bt_found {
    double par, lam, dxnorm;
    int it, status, info;
};

// wnorm: |w| with R^T w = D^2 x / |D x| when R has full rank, else unused.  par0: the starting guess of par
__device__ __forceinline__ void bt_start(bt_state& S, bool fullrank, double wnorm, double gnorm, double dxnorm, double delta, double par0)
{
    S.parl = fullrank ? ((S.fp / delta) / wnorm) / wnorm : 0.0;
    S.paru = gnorm / delta;
    if (S.paru == 0.0) S.paru = DBL_MIN / fmin(delta, 0.1);
    S.par = fmin(fmax(par0, S.parl), S.paru);
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

// |g| of the scaled gradient, lane j holding g_j = (R^T z)_j / d_j (0 in lanes >= n): a product of two data quantities, whose square
// leaves the double range where g itself is far inside it (MINPACK's enorm).  The largest |g_j| by a butterfly (the same word in every
// lane, and in every wave that reads the same g); inside BT_G_LO .. BT_G_HI the plain sum, bit for bit what the search always formed.
// Outside it g is scaled by the power of two that brings the largest entry into [1, 2) -- exact, so wherever no term of the plain sum
// overflows or goes subnormal the result keeps the plain sum's bits as well.  A largest entry that is no finite number takes the plain sum.
#define BT_G_LO 0x1p-256
#define BT_G_HI 0x1p+256
__device__ __forceinline__ double bt_wave_gnorm(double gl)
{
    double gmax = fabs(gl);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gmax = fmax(gmax, __shfl_xor(gmax, o));
    if (gmax == 0.0 || (gmax >= BT_G_LO && gmax <= BT_G_HI) || !(gmax <= DBL_MAX)) return sqrt(qb_wave_sum(gl * gl));
    const int e = ilogb(gmax);
    const double gs = ldexp(gl, -e);
    return ldexp(sqrt(qb_wave_sum(gs * gs)), e);
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

// The search of one member: dsc is the lane's d (of column `lane` of the triangle), delta a radius that bt_delta_ok takes, par0 the
// starting par.  Returns the lane's x (lane i: x_i in the triangle's column order, 0 in lanes >= n), which Xs holds as well; zl: the
// lane's z.  F.info != 0: wave-uniform, and nothing else holds.
template <int W>
__device__ __forceinline__ double bt_wave_core(const double (&r)[W], int n, int lane, double dsc, double delta, double par0, double rtol,
                                               int maxit, double* Rs, double* Xs, double& zl, bt_found& F)
{
    constexpr int LW = W + 1;
    double diag = 1.0;                        // lane i: z_i and R(i, i)
    zl = 0.0;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        zl = c == n ? r[c] : zl;
        if (c < n && lane == c) diag = r[c];
    }
    const int inf0 = qb_info_wave(diag, n, lane);
    const int nsing = inf0 ? inf0 - 1 : n;
    // the Gauss-Newton step: the leading nsing x nsing system, zeros below
    double xi = bt_wave_solve<W>(r, n, nsing, lane, Rs, Xs);
    double dxnorm = bt_wave_dxnorm(dsc, xi);
    bt_state S;
    S.fp = dxnorm - delta;
    S.par = 0.0;
    int it = 0, status = 1;
    double lam = 0.0;
    F.info = 0;
    if (!(S.fp <= rtol * delta)) {
        const double wnorm = nsing == n ? bt_wave_wnorm<W>(n, lane, dsc, xi, dxnorm, Rs, Xs + LW) : 0.0;
        double gl = 0.0;                      // lane j: (sum over i <= j of R(i, j) z_i) / d_j
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (c < n) {
                const double t = qb_wave_sum(r[c] * zl);
                if (lane == c) gl = t;
            }
        }
        gl = (lane < n && dsc != 0.0) ? gl / dsc : 0.0;
        const double gnorm = bt_wave_gnorm(gl);
        bt_start(S, nsing == n, wnorm, gnorm, dxnorm, delta, par0);
        for (it = 1;; ++it) {
            if (S.par == 0.0) S.par = fmax(DBL_MIN, 0.001 * S.paru);
            lam = sqrt(S.par);
            double w[W];
            bd_wave_elim<W>(r, lam * dsc, n, n + 1, lane, w);
            double dg = 1.0;
#pragma unroll
            for (int c = 0; c < W; ++c)
                if (c < n && lane == c) dg = w[c];
            const int inf = qb_info_wave(dg, n, lane);
            if (inf) {                        // (wave-uniform)
                F.info = inf;
                return 0.0;
            }
            xi = bt_wave_solve<W>(w, n, n, lane, Rs, Xs);
            dxnorm = bt_wave_dxnorm(dsc, xi);
            const double fpprev = S.fp;
            S.fp = dxnorm - delta;
            status = bt_leave(S, fpprev, delta, rtol, it, maxit);
            if (status >= 0) break;           // (butterfly results: the same decision in every lane)
            bt_update(S, bt_wave_wnorm<W>(n, lane, dsc, xi, dxnorm, Rs, Xs + LW), delta);
        }
    }
    F.par = it ? S.par : 0.0;
    F.lam = lam;
    F.dxnorm = dxnorm;
    F.it = it;
    F.status = status;
    return xi;
}

template <int W>
static constexpr size_t bt_wave_lds() { return sizeof(double) * 4 * 2 * W * (W + 1); }

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

// The search of one member by all 256 threads.  Ms: the master [R | z] (column n: z), Ws and Ss the two other images of bd_wg_lds,
// dsc[i] the d of column i, all in LDS and visible to every thread on entry.  sdec: four doubles and sinfo: two ints of LDS, the words
// through which thread 0 publishes: sdec[0] the Gauss-Newton step is accepted, [1] lambda of the coming elimination, [2] status, [3] par
// of the coming elimination; sinfo[0] the info of an elimination, sinfo[1] nsing.  On return x is column n of Ws (xs), visible to every
// thread; F.info != 0: the same word in every thread, and nothing else holds.
__device__ __forceinline__ void bt_wg_core(const double* Ms, double* Ws, double* Ss, const double* dsc, double* sdec, int* sinfo, int n, int ld,
                                           double delta, double par0, double rtol, int maxit, int t, bt_found& F)
{
    const int lane = t & 63, wv = t >> 6, ntot = n + 1;
    double* xs = Ws + (size_t) n * ld;
    double* us = Ss + (size_t) n * ld;
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
    F.info = 0;
    // Every wave forms the norms below from the same LDS words, but the search runs on thread 0's copy alone: it publishes each
    // decision, and all 256 threads read that word after a barrier.  (With every wave deciding for itself, one member of the tests
    // came back with X one unit in the last place off the damped solve of the lambda returned, from the row down whose diagonal entry
    // of the block another wave had written: the block must hold one lambda, so one thread chooses it.)
    if (t == 0) {
        sdec[0] = S.fp <= rtol * delta ? 1.0 : 0.0;
        sdec[3] = 0.0;
    }
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
        const double gnorm = bt_wave_gnorm(gl);
        bt_start(S, nsing == n, wnorm, gnorm, dxnorm, delta, par0);
        for (it = 1;; ++it) {
            if (S.par == 0.0) S.par = fmax(DBL_MIN, 0.001 * S.paru);
            if (t == 0) {
                sdec[1] = sqrt(S.par);
                sdec[3] = S.par;
            }
            __syncthreads();
            lam = sdec[1];
            bd_wg_elim(Ms, Ws, Ss, dsc, lam, n, ntot, ld, t);
            if (t == 0) sinfo[0] = qb_info_serial(Ws, ld, n);
            __syncthreads();
            if (sinfo[0]) {                   // (the same word in every thread)
                F.info = sinfo[0];
                return;
            }
            if (t == 0) qb_trsv(Ws, ld, n, xs);
            __syncthreads();
            dxnorm = bt_wg_dxnorm(dsc, xs, n, lane);
            const double fpprev = S.fp;
            S.fp = dxnorm - delta;
            if (t == 0) sdec[2] = (double) bt_leave(S, fpprev, delta, rtol, it, maxit);
            __syncthreads();
            status = (int) sdec[2];
            if (status >= 0) break;           // (the same word in every thread)
            bt_update(S, bt_wg_wnorm(Ws, ld, n, dsc, xs, dxnorm, us, t), delta);
        }
    }
    F.par = sdec[3];
    F.lam = lam;
    F.dxnorm = dxnorm;
    F.it = it;
    F.status = status;
}

#endif
