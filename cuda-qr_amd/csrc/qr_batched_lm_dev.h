// qr_batched_lm_dev.h -- the rules of MINPACK lmder's outer loop that the kernels of qr_batched_lm.hip run for mi355x_qr.h section 8m and
// for section 8n (the same loop with box bounds on x): the scalars of a step (rules c, d and e), the end of a step (rules g, h and i),
// the refusal of a search, the update and the start.  No kernels, no entry points.  Both sections run the code below, so the bounded
// solver with every bound infinite returns the bits of section 8m.
//
// Every sum runs in a fixed order; every scalar rule is compiled with contraction off, so that each rounding is the one written.
#ifndef QR_BATCHED_LM_DEV_H
#define QR_BATCHED_LM_DEV_H

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

// The update of member q by one wave: f the member's residuals at the trial point (m of them, read strided by lane).  noftol (the same
// word in every lane): the two tests on the reductions (status 1 and 6) are left out -- section 8n's rule for a step that a bound cut
// short; section 8m passes false.
__device__ __forceinline__ void blm_update_member(const double* __restrict__ f, int m, int n, size_t q, int lane, const qrd_blm_state& s,
                                                  const qrd_blm_opts& o, bool noftol)
{
#pragma clang fp contract(off)
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
    if (!noftol && fabs(actred) <= o.ftol && prered <= o.ftol && small) st = 1;
    if (delta <= o.xtol * xnorm) st = st == 1 ? 3 : 2;
    if (st == 0) {
        if (nfev >= o.maxfev) st = 5;
        if (!noftol && fabs(actred) <= eps && prered <= eps && small) st = 6;
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

// 8m's start of member q by one thread
__device__ __forceinline__ void blm_start_member(const double* __restrict__ X0, size_t sX, const double* __restrict__ D0, size_t sD, int n,
                                                 size_t q, const qrd_blm_state& s, int mode)
{
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

// LDS of the workgroup route of a step: bd_wg_lds, then acn[64], gs[64] and eight words
__host__ __device__ constexpr size_t blm_wg_lds(int n) { return bd_wg_lds(n, n + 1) + sizeof(double) * (64 + 64 + 8); }
static_assert(blm_wg_lds(63) <= QB_LDS_CAP, "the three images and the words fit");

static inline int blm_bad_state(const qrd_blm_state* s)
{
    return !s->x || !s->xtrial || !s->D || !s->delta || !s->par || !s->fnorm || !s->xnorm || !s->pnorm || !s->gnorm || !s->prered || !s->dirder ||
           !s->iter || !s->nfev || !s->njev || !s->accepted || !s->status || !s->info || !s->par_status;
}

#endif
