// qr_batched_lm.hip -- kernels of the batched Levenberg-Marquardt solver (qr_batched_lm.c, mi355x_qr.h section 8m): MINPACK lmder's outer
// loop per member, split by reverse communication into a step (from the pivoted factors of the Jacobian and Q^T f: the norms, the
// scaling D, the gradient test, the trust-region search of section 8g, the trial point and the predicted reduction) and an update (from
// f at the trial point: the gain ratio, the radius, par, accept or reject, the stopping tests).  Written from lmder's description
// (More 1978; More, Garbow, Hillstrom, ANL-80-74); the MINPACK variable names are kept.
//
//   blm_start_kernel          a thread per member: x <- X0, D <- D0 (mode 2) or 1, the counters and the scalars
//   blm_step_wave_kernel<W>   n + 1 <= W <= 32: one wave per member, four per workgroup, no barrier.  bt_wave_kernel's layout; the search is
//                             bt_wave_core of qr_batched_trust_dev.h, the code qr_batched_trust.hip runs
//   blm_step_wg_kernel        n <= 63 otherwise: one workgroup per member on bd_wg_lds's three images; wave 0 forms every scalar and lane 0
//                             publishes the decision and the radius in LDS words that all threads read after a barrier; the search is
//                             bt_wg_core
//   blm_update_kernel         one wave per member, four per workgroup, f at the trial point read strided by lane
//
// A member whose status or info word is not 0 is skipped by the step and by the update: nothing of its state is written.  Every sum runs
// in a fixed order; no atomics.  Every scalar rule is compiled with contraction off, so that each rounding is the one written.
#include "qr_batched_trust_dev.h"

static_assert(QRD_B_MAX_N == 64, "one lane per row of the triangle");

__device__ __forceinline__ double blm_wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// the scalars of a member that a step reads and forms; the same values in every lane that runs blm_scalars
struct blm_head {
    double Dk, xk, delta, xnorm, gnorm;
    int iter, stop;                           // stop: 0 go on to the search, 1 the member is done or has an info word
};

// Rules c, d and e for one member, by one wave: lane k < n holds acn = |R(0:k, k)|, gk = sum over i <= k of R(i, k) (z_i / fnorm) and
// perm = jpvt[k].  Writes D, fnorm, gnorm, xnorm, njev and, where the member ends here, delta and status (or info alone for a D of mode 2
// that is not positive).
__device__ __forceinline__ void blm_scalars(const qrd_blm_state& s, const qrd_blm_opts& o, size_t q, int n, int lane, int perm, double acn,
                                            double gk, double fnorm, blm_head& h)
{
#pragma clang fp contract(off)
    const bool in = lane < n;
    const size_t qn = q * (size_t) n;
    const bool first = s.njev[q] == 0;
    h.iter = s.iter[q];
    h.Dk = in ? s.D[qn + perm] : 1.0;
    h.xk = in ? s.x[qn + perm] : 0.0;
    h.delta = s.delta[q];
    h.xnorm = s.xnorm[q];
    h.stop = 0;
    if (first) {                              // (the same word in every lane)
        if (o.mode != 2) {
            h.Dk = (in && acn != 0.0) ? acn : 1.0;
        } else if (__ballot(in && !(h.Dk > 0.0))) {
            if (lane == 0) s.info[q] = -1;
            h.stop = 1;
            return;
        }
        const double dx = in ? h.Dk * h.xk : 0.0;
        h.xnorm = sqrt(bd_wave_dot(dx, dx));
        h.delta = o.factor * h.xnorm;
        if (h.delta == 0.0) h.delta = o.factor;
    }
    h.gnorm = 0.0;
    if (fnorm != 0.0) h.gnorm = blm_wave_max((in && acn != 0.0) ? fabs(gk / acn) : 0.0);
    const bool done = h.gnorm <= o.gtol;
    if (!done && o.mode != 2) h.Dk = fmax(h.Dk, acn);
    if (in && o.mode != 2) s.D[qn + perm] = h.Dk;
    if (lane == 0) {
        s.fnorm[q] = fnorm;
        s.gnorm[q] = h.gnorm;
        s.xnorm[q] = h.xnorm;
        s.njev[q] += 1;
        if (done) {
            s.delta[q] = h.delta;
            s.status[q] = 4;
        }
    }
    if (done) h.stop = 1;
}

// Rules g, h and i: pk the lane's entry of the step (column order of the triangle), rp the lane's row of R P^T p
__device__ __forceinline__ void blm_finish(const qrd_blm_state& s, size_t q, int n, int lane, int perm, const blm_head& h, double pk, double rp,
                                           double fnorm, const bt_found& F)
{
#pragma clang fp contract(off)
    const double pnorm = F.dxnorm;
    if (lane < n) s.xtrial[q * (size_t) n + perm] = h.xk - pk;
    const double delta = h.iter == 1 ? fmin(h.delta, pnorm) : h.delta;
    const double t = lane < n ? rp : 0.0;
    const double temp1 = sqrt(bd_wave_dot(t, t)) / fnorm;
    const double temp2 = (sqrt(F.par) * pnorm) / fnorm;
    const double t1 = temp1 * temp1, t2 = temp2 * temp2;
    if (lane == 0) {
        s.delta[q] = delta;
        s.par[q] = F.par;
        s.pnorm[q] = pnorm;
        s.prered[q] = t1 + t2 / 0.5;
        s.dirder[q] = -(t1 + t2);
        s.par_status[q] = F.status;
    }
}

// the search refused the member: a radius that is no finite positive number (-1) or a zero on a damped diagonal (i + 1)
__device__ __forceinline__ void blm_fail(const qrd_blm_state& s, size_t q, int info)
{
    s.info[q] = info;
    s.status[q] = -1;
}

template <int W>
__global__ void __launch_bounds__(256) blm_step_wave_kernel(const qrd_blm_step_args a)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) a.d.batch) return;      // (no workgroup barrier below: the waves of a workgroup are independent)
    const qrd_blm_state& s = a.s;
    if (s.status[q] != 0 || s.info[q] != 0) return;
    const int n = a.d.n;
    bd_lane L;
    bd_lane_setup(a.d, q, lane, L);
    double r[W];
    bd_wave_load<W>(a.d, q, lane, r, L);
    double zl = 0.0;
#pragma unroll
    for (int c = 0; c < W; ++c) zl = c == n ? r[c] : zl;
    const double fnorm = sqrt(bd_wave_dot(zl, zl) + qb_bcast(L.rss, 0));
    const double zs = zl / fnorm;
    double acn = 0.0, gk = 0.0;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        if (c < n) {
            const double ss = bd_wave_dot(r[c], r[c]);
            const double g = qb_wave_sum(r[c] * zs);
            if (lane == c) { acn = sqrt(ss); gk = g; }
        }
    }
    blm_head h;
    blm_scalars(s, a.o, q, n, lane, L.perm, acn, gk, fnorm, h);
    if (h.stop) return;                       // (wave-uniform)
    if (!bt_delta_ok(h.delta)) {
        if (lane == 0) blm_fail(s, q, -1);
        return;
    }
    constexpr int LW = W + 1;
    double* Rs = sm + (size_t) wv * 2 * W * LW;
    double* Xs = Rs + W * LW;
    double z2;
    bt_found F;
    const double pk = bt_wave_core<W>(r, n, lane, h.Dk, h.delta, s.par[q], a.o.par_rtol, a.o.par_maxit, Rs, Xs, z2, F);
    if (F.info) {                             // (wave-uniform)
        if (lane == 0) blm_fail(s, q, F.info);
        return;
    }
    double rp = 0.0;                          // row lane of R P^T p, the sum over the columns ascending (zeros below the diagonal)
#pragma unroll
    for (int cc = 0; cc < W; ++cc)
        if (cc < n) rp = fma(r[cc], Xs[cc], rp);
    blm_finish(s, q, n, lane, L.perm, h, pk, rp, fnorm, F);
}

// LDS of the workgroup route: bd_wg_lds, then acn[64], gs[64] and eight words
__host__ __device__ constexpr size_t blm_wg_lds(int n) { return bd_wg_lds(n, n + 1) + sizeof(double) * (64 + 64 + 8); }
static_assert(blm_wg_lds(63) <= QB_LDS_CAP, "the three images and the words fit");

__global__ void __launch_bounds__(256) blm_step_wg_kernel(const qrd_blm_step_args a)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const qrd_blm_state& s = a.s;
    if (s.status[q] != 0 || s.info[q] != 0) return;      // (the same words in every thread)
    const int n = a.d.n, ntot = n + 1, ld = bd_ld(n);
    double* Ms = sm;
    double* Ws = Ms + (size_t) ntot * ld;
    double* Ss = Ws + (size_t) ntot * ld;
    double* dsc = Ss + (size_t) ntot * ld;
    double* rssv = dsc + 64;
    int* perm = (int*) (rssv + 64);
    int* sinfo = perm + 64;
    double* sdec = rssv + 1;                  // (one right-hand side: only rssv[0] is taken)
    double* acn = (double*) sinfo + 2;        // past bd_wg_lds's two words
    double* gs = acn + 64;
    double* pub = gs + 64;                    // [0] the member stops here, [1] the radius of the search
    const double* xs = Ws + (size_t) n * ld;
    bd_wg_load(a.d, q, t, Ms, ld, dsc, rssv, perm);
    __syncthreads();
    const double zl = lane < n ? Ms[n * ld + lane] : 0.0;
    const double fnorm = sqrt(bd_wave_dot(zl, zl) + rssv[0]);         // (every wave, from the same LDS words)
    const double zs = zl / fnorm;
    for (int k = wv; k < n; k += 4) {         // wave wv: columns wv, wv + 4, ..
        const double v = lane <= k ? Ms[k * ld + lane] : 0.0;
        const double ss = bd_wave_dot(v, v);
        const double g = qb_wave_sum(v * zs);
        if (lane == 0) { acn[k] = sqrt(ss); gs[k] = g; }
    }
    __syncthreads();
    blm_head h;
    h.stop = 0;
    if (wv == 0) {
        const bool in = lane < n;
        blm_scalars(s, a.o, q, n, lane, perm[lane], in ? acn[lane] : 0.0, in ? gs[lane] : 0.0, fnorm, h);
        if (!h.stop && !bt_delta_ok(h.delta)) {
            if (lane == 0) blm_fail(s, q, -1);
            h.stop = 1;
        }
        if (in) dsc[lane] = h.Dk;
        if (lane == 0) {
            pub[0] = h.stop ? 1.0 : 0.0;
            pub[1] = h.delta;
        }
    }
    __syncthreads();
    if (pub[0] != 0.0) return;                // (the same word in every thread)
    bt_found F;
    bt_wg_core(Ms, Ws, Ss, dsc, sdec, sinfo, n, ld, pub[1], s.par[q], a.o.par_rtol, a.o.par_maxit, t, F);
    if (F.info) {                             // (the same word in every thread)
        if (t == 0) blm_fail(s, q, F.info);
        return;
    }
    if (wv == 0) {
        const double pk = lane < n ? xs[lane] : 0.0;
        double rp = 0.0;
        if (lane < n)
            for (int cc = lane; cc < n; ++cc) rp = fma(Ms[cc * ld + lane], xs[cc], rp);
        blm_finish(s, q, n, lane, perm[lane], h, pk, rp, fnorm, F);
    }
}

__global__ void __launch_bounds__(256) blm_update_kernel(const double* __restrict__ Ft, int m, int ldf, size_t sF, int n, int batch,
                                                         const qrd_blm_state s, const qrd_blm_opts o)
{
#pragma clang fp contract(off)
    (void) ldf;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) batch) return;
    if (s.status[q] != 0 || s.info[q] != 0) return;
    const double* f = Ft + q * sF;
    double t = 0.0;
    for (int i = lane; i < m; i += 64) t = fma(f[i], f[i], t);
    const double fnorm1 = sqrt(qb_wave_sum(t));
    double fnorm = s.fnorm[q], delta = s.delta[q], par = s.par[q], xnorm = s.xnorm[q];
    const double prered = s.prered[q], dirder = s.dirder[q], pnorm = s.pnorm[q], gnorm = s.gnorm[q];
    const double eps = DBL_EPSILON;
    const bool finite = fnorm1 <= DBL_MAX;    // (false for NaN and inf: an addition to MINPACK, such a point counts as no reduction)
    const bool worse = !finite || 0.1 * fnorm1 >= fnorm;
    double actred = -1.0;
    if (finite && 0.1 * fnorm1 < fnorm) {
        const double fr = fnorm1 / fnorm;
        actred = 1.0 - fr * fr;
    }
    const double ratio = prered != 0.0 ? actred / prered : 0.0;
    if (ratio <= 0.25) {
        double temp = actred >= 0.0 ? 0.5 : 0.5 * dirder / (dirder + 0.5 * actred);
        if (worse || temp < 0.1) temp = 0.1;
        delta = temp * fmin(delta, pnorm / 0.1);
        par = par / temp;
    } else if (par == 0.0 || ratio >= 0.75) {
        delta = pnorm / 0.5;
        par = 0.5 * par;
    }
    const bool accept = ratio >= 1.0e-4;
    int iter = s.iter[q];
    if (accept) {                             // (wave-uniform)
        const size_t qn = q * (size_t) n;
        const double xv = lane < n ? s.xtrial[qn + lane] : 0.0;
        const double dx = lane < n ? s.D[qn + lane] * xv : 0.0;
        if (lane < n) s.x[qn + lane] = xv;
        xnorm = sqrt(bd_wave_dot(dx, dx));
        fnorm = fnorm1;
        iter += 1;
    }
    const int nfev = s.nfev[q] + 1;
    const bool small = 0.5 * ratio <= 1.0;
    int st = 0;
    if (fabs(actred) <= o.ftol && prered <= o.ftol && small) st = 1;
    if (delta <= o.xtol * xnorm) st = st == 1 ? 3 : 2;
    if (st == 0) {
        if (nfev >= o.maxfev) st = 5;
        if (fabs(actred) <= eps && prered <= eps && small) st = 6;
        if (delta <= eps * xnorm) st = 7;
        if (gnorm <= eps) st = 8;
    }
    if (lane == 0) {
        s.delta[q] = delta;
        s.par[q] = par;
        s.fnorm[q] = fnorm;
        s.xnorm[q] = xnorm;
        s.iter[q] = iter;
        s.nfev[q] = nfev;
        s.accepted[q] = accept ? 1 : 0;
        s.status[q] = st;
    }
}

__global__ void __launch_bounds__(256) blm_start_kernel(const double* __restrict__ X0, size_t sX, const double* __restrict__ D0, size_t sD, int n,
                                                        int batch, const qrd_blm_state s, int mode)
{
    const size_t q = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t) batch) return;
    const size_t qn = q * (size_t) n;
    for (int i = 0; i < n; ++i) {
        const double x = X0[q * sX + i];
        s.x[qn + i] = x;
        s.xtrial[qn + i] = x;
        s.D[qn + i] = mode == 2 ? D0[q * sD + i] : 1.0;
    }
    s.delta[q] = 0.0; s.par[q] = 0.0; s.fnorm[q] = 0.0; s.xnorm[q] = 0.0; s.pnorm[q] = 0.0; s.gnorm[q] = 0.0; s.prered[q] = 0.0; s.dirder[q] = 0.0;
    s.iter[q] = 1; s.nfev[q] = 1; s.njev[q] = 0; s.accepted[q] = 0; s.status[q] = 0; s.info[q] = 0; s.par_status[q] = 0;
}

// the kernels that may ask for more than 64 KiB of LDS (qb_allow_lds)
static int blm_allow_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(blm_step_wg_kernel), reinterpret_cast<const void*>(blm_step_wave_kernel<32>)};
    return qb_allow_lds(fns, done);
}

static int blm_bad_state(const qrd_blm_state* s)
{
    return !s->x || !s->xtrial || !s->D || !s->delta || !s->par || !s->fnorm || !s->xnorm || !s->pnorm || !s->gnorm || !s->prered || !s->dirder ||
           !s->iter || !s->nfev || !s->njev || !s->accepted || !s->status || !s->info || !s->par_status;
}

extern "C" {

int qrd_blm_start(void* stream, const double* X0, int ldx, size_t sX, const double* D0, size_t sD, int n, int batch, const qrd_blm_state* s,
                  int mode)
{
    if (batch <= 0) return 0;
    if (!s || blm_bad_state(s) || !X0 || n < 1 || n + 1 > QRD_B_MAX_N || ldx < n || (mode == 2 && !D0)) return -7;
    hipLaunchKernelGGL(blm_start_kernel, dim3((unsigned) (((size_t) batch + 255) / 256)), dim3(256), 0, (hipStream_t) stream, X0, sX, D0, sD, n,
                       batch, *s, mode);
    return (int) hipGetLastError();
}

// the step of every running member from factors that exist: one launch.  -7: shape not taken
int qrd_blm_step(void* stream, const qrd_blm_step_args* a)
{
    if (!a || a->d.batch <= 0) return 0;
    const qrd_bd_args* d = &a->d;
    if (d->n < 1 || d->n + 1 > QRD_B_MAX_N || d->nrhs != 1 || d->nlam != 1 || !d->R || !d->Z || d->ldr < d->n || d->zrows < d->n ||
        d->ldz < d->zrows || d->flip || d->D || blm_bad_state(&a->s) || !(a->o.par_rtol > 0.0 && a->o.par_rtol < 1.0) || a->o.par_maxit < 1)
        return -7;
    const int rc = blm_allow_lds();
    if (rc) return rc;
    hipStream_t s = (hipStream_t) stream;
    const int ntot = d->n + 1;
    if (qrd_bd_wave_route(ntot)) {
        const dim3 grid((unsigned) (((size_t) d->batch + 3) / 4));
        if (ntot <= 4) hipLaunchKernelGGL(blm_step_wave_kernel<4>, grid, dim3(256), bt_wave_lds<4>(), s, *a);
        else if (ntot <= 8) hipLaunchKernelGGL(blm_step_wave_kernel<8>, grid, dim3(256), bt_wave_lds<8>(), s, *a);
        else if (ntot <= 16) hipLaunchKernelGGL(blm_step_wave_kernel<16>, grid, dim3(256), bt_wave_lds<16>(), s, *a);
        else hipLaunchKernelGGL(blm_step_wave_kernel<32>, grid, dim3(256), bt_wave_lds<32>(), s, *a);
    } else {
        hipLaunchKernelGGL(blm_step_wg_kernel, dim3((unsigned) d->batch), dim3(256), blm_wg_lds(d->n), s, *a);
    }
    return (int) hipGetLastError();
}

int qrd_blm_update(void* stream, const double* Ft, int m, int ldf, size_t sF, int n, int batch, const qrd_blm_state* s, const qrd_blm_opts* o)
{
    if (batch <= 0) return 0;
    if (!s || !o || blm_bad_state(s) || !Ft || n < 1 || n + 1 > QRD_B_MAX_N || m < 1 || ldf < m) return -7;
    hipLaunchKernelGGL(blm_update_kernel, dim3((unsigned) (((size_t) batch + 3) / 4)), dim3(256), 0, (hipStream_t) stream, Ft, m, ldf, sF, n, batch,
                       *s, *o);
    return (int) hipGetLastError();
}

}   // extern "C"
