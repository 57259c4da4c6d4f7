// qr_batched_lm.hip -- kernels of the batched Levenberg-Marquardt solvers (qr_batched_lm.c, mi355x_qr.h sections 8m and 8n): MINPACK
// lmder's outer loop per member, split by reverse communication into a step (from the pivoted factors of the Jacobian and Q^T f: the
// norms, the scaling D, the gradient test, the trust-region search of section 8g, the trial point and the predicted reduction) and an
// update (from f at the trial point: the gain ratio, the radius, par, accept or reject, the stopping tests).  Written from lmder's
// description (More 1978; More, Garbow, Hillstrom, ANL-80-74); the MINPACK variable names are kept.  Section 8n is the same loop with
// MPFIT's rules for lo <= x <= hi (Markwardt 2009, "Non-linear least squares fitting in IDL with MPFIT"), and two corrections to them
// (DESIGN section 7w).
//
// One step kernel pair, two instantiations: the step kernels are templates on the argument struct, qrd_blm_step_args (8m) or
// qrd_blmb_step_args (8n), and rule S of section 8n is a block under `if constexpr (bounded)` between the search and blm_finish.  So a
// member whose bounds are all infinite gets the bits section 8m gives it by construction.
//
//   blm_start_kernel             a thread per member: x <- X0, D <- D0 (mode 2) or 1, the counters and the scalars
//   blm_step_wave_kernel<W, A>   n + 1 <= W <= 32: one wave per member, four per workgroup, no barrier.  bt_wave_kernel's layout; the search
//                                is bt_wave_core of qr_batched_trust_dev.h, the code qr_batched_trust.hip runs
//   blm_step_wg_kernel<A>        n <= 63 otherwise: one workgroup per member on bd_wg_lds's three images; wave 0 forms every scalar and lane
//                                0 publishes the decision and the radius in LDS words that all threads read after a barrier; the search is
//                                bt_wg_core; rule S by wave 0
//   blm_update_kernel            one wave per member, four per workgroup, f at the trial point read strided by lane
//   blmb_start_kernel            a thread per member: the bounds checked (info -2, nothing else written), then 8m's start, lo, hi, peg = 0
//   blmb_peg_kernel              rule P, before the factorisation: a wave per member, four per workgroup; g_j = sum_i J(i, j) f_i for the
//                                columns whose x_j is exactly on a bound (lane l: rows l, l + 64, .. ascending by fma, then the wave sum),
//                                peg_j from its sign, the held columns of J cleared.  J is read and cleared down the columns, a lane a row
//   blmb_update_kernel           blm_update_kernel; the two tests on the reductions are left out while the member's clipped word is set
//
// A member whose status or info word is not 0 is skipped by every kernel but the starts: nothing of its state, and no column of its J, is
// written.  Every sum runs in a fixed order; no atomics.  Every scalar rule is compiled with contraction off, so that each rounding is the
// one written.
#include <cmath>
#include <type_traits>

#include "qr_batched_trust_dev.h"
#include "qr_batched_lm_dev.h"      // blm_scalars, blm_finish, blm_fail, the update and the start

// ---- section 8n: rule S and what it leaves ----
__device__ __forceinline__ double blmb_wave_min(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}

// what rule S leaves: pt the lane's entry of the step taken p~ = -alpha s (column order of the triangle), xt the lane's entry of the trial
// point; alpha and plain (nothing was zeroed and alpha == 1: rules g, h and i hold verbatim) are the same in every lane
struct blmb_cut_t {
    double pt, xt, alpha;
    int plain;
};

// Rule S for one member, by one wave: lane k < n holds xk = x[perm] and pk, its entry of the search's step (0 in lanes >= n)
__device__ __forceinline__ void blmb_cut(const qrd_blmb_state& s, size_t q, int n, int lane, int perm, double xk, double pk, blmb_cut_t& c)
{
#pragma clang fp contract(off)
    const bool in = lane < n;
    const size_t j = q * (size_t) n + (in ? perm : 0);
    const double lo = in ? s.lo[j] : -HUGE_VAL, hi = in ? s.hi[j] : HUGE_VAL;
    const int pg = in ? s.peg[j] : 0;
    double sj = in ? -pk : 0.0;
    const bool hold = in && (pg != 0 || (xk <= lo && sj < 0.0) || (xk >= hi && sj > 0.0));
    const bool zeroed = hold && sj != 0.0;
    if (hold) sj = 0.0;
    double r = HUGE_VAL, bound = 0.0;         // the lane's ratio, where x + s leaves the box
    if (in && sj != 0.0) {
        const double t = xk + sj;
        if (t < lo) {
            r = (lo - xk) / sj;
            bound = lo;
        } else if (t > hi) {
            r = (hi - xk) / sj;
            bound = hi;
        }
    }
    c.alpha = fmin(1.0, blmb_wave_min(r));
    c.plain = !__ballot(zeroed) && c.alpha == 1.0;
    c.pt = -(c.alpha * sj);
    double xt = xk - c.pt;
    if (xt < lo) xt = lo;
    if (xt > hi) xt = hi;
    if (r == c.alpha) xt = bound;             // the bound itself, bitwise
    c.xt = xt;
}

// After blm_finish on p~ (xtrial = x - p~, delta, par, pnorm = the search's |D p|, par_status, and 8m's prered and dirder): the trial point
// inside the box, alpha and clipped, and for a step that is not plain the linear model's own reduction for the step taken.  rp: the lane's
// row of R P^T p~, gk: the lane's gradient entry of rule d
__device__ __forceinline__ void blmb_finish(const qrd_blmb_state& s, size_t q, int n, int lane, int perm, const blmb_cut_t& c, double rp, double gk,
                                            double fnorm)
{
#pragma clang fp contract(off)
    const bool in = lane < n;
    if (in) s.b.xtrial[q * (size_t) n + perm] = c.xt;
    const double t = in ? rp : 0.0;
    const double temp1 = sqrt(bd_wave_dot(t, t)) / fnorm;
    const double t1 = temp1 * temp1;
    const double pg = qb_wave_sum(in ? c.pt * gk : 0.0) / fnorm;
    if (lane == 0) {
        s.alpha[q] = c.alpha;
        s.clipped[q] = c.alpha < 1.0 ? 1 : 0;
        if (!c.plain) {
            s.b.prered[q] = fmax(0.0, 2.0 * pg - t1);
            s.b.dirder[q] = -pg;
        }
    }
}

// ---- the step: one kernel pair for both sections ----
__device__ __forceinline__ const qrd_blm_state& blm_state_of(const qrd_blm_state& s) { return s; }
__device__ __forceinline__ const qrd_blm_state& blm_state_of(const qrd_blmb_state& s) { return s.b; }

template <int W, class A>
__global__ void __launch_bounds__(256) blm_step_wave_kernel(const A a)
{
#pragma clang fp contract(off)
    constexpr bool bounded = std::is_same<A, qrd_blmb_step_args>::value;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) a.d.batch) return;      // (no workgroup barrier below: the waves of a workgroup are independent)
    const qrd_blm_state& s = blm_state_of(a.s);
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
    double pk = bt_wave_core<W>(r, n, lane, h.Dk, h.delta, s.par[q], a.o.par_rtol, a.o.par_maxit, Rs, Xs, z2, F);
    if (F.info) {                             // (wave-uniform)
        if (lane == 0) blm_fail(s, q, F.info);
        return;
    }
    blmb_cut_t c;
    if constexpr (bounded) {
        blmb_cut(a.s, q, n, lane, L.perm, h.xk, pk, c);
        if (!c.plain) {                       // (wave-uniform) the step taken in the search's place
            if (lane < n) Xs[lane] = c.pt;
            QB_WAVE_SYNC();
        }
        pk = c.pt;
    }
    double rp = 0.0;                          // row lane of R P^T p, the sum over the columns ascending (zeros below the diagonal)
#pragma unroll
    for (int cc = 0; cc < W; ++cc)
        if (cc < n) rp = fma(r[cc], Xs[cc], rp);
    blm_finish(s, q, n, lane, L.perm, h, pk, rp, fnorm, F);
    if constexpr (bounded) blmb_finish(a.s, q, n, lane, L.perm, c, rp, gk, fnorm);
}

template <class A>
__global__ void __launch_bounds__(256) blm_step_wg_kernel(const A a)
{
#pragma clang fp contract(off)
    constexpr bool bounded = std::is_same<A, qrd_blmb_step_args>::value;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const qrd_blm_state& s = blm_state_of(a.s);
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
    double* xs = Ws + (size_t) n * ld;
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
    if (wv == 0) {                            // (no workgroup barrier below: wave 0 alone reads and writes xs from here on)
        const bool in = lane < n;
        double pk = in ? xs[lane] : 0.0;
        blmb_cut_t c;
        if constexpr (bounded) {
            blmb_cut(a.s, q, n, lane, perm[lane], h.xk, pk, c);
            if (!c.plain) {                   // (wave-uniform)
                QB_WAVE_SYNC();               // (every lane has read its pk)
                if (in) xs[lane] = c.pt;
                QB_WAVE_SYNC();
            }
            pk = c.pt;
        }
        double rp = 0.0;
        if (in)
            for (int cc = lane; cc < n; ++cc) rp = fma(Ms[cc * ld + lane], xs[cc], rp);
        blm_finish(s, q, n, lane, perm[lane], h, pk, rp, fnorm, F);
        if constexpr (bounded) blmb_finish(a.s, q, n, lane, perm[lane], c, rp, in ? gs[lane] : 0.0, fnorm);
    }
}

// ---- the updates, rule P and the starts ----
__global__ void __launch_bounds__(256) blm_update_kernel(const double* __restrict__ Ft, int m, int ldf, size_t sF, int n, int batch,
                                                         const qrd_blm_state s, const qrd_blm_opts o)
{
#pragma clang fp contract(off)
    (void) ldf;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) batch) return;
    if (s.status[q] != 0 || s.info[q] != 0) return;
    blm_update_member(Ft + q * sF, m, n, q, lane, s, o, false);
}

__global__ void __launch_bounds__(256) blmb_update_kernel(const double* __restrict__ Ft, int m, size_t sF, int n, int batch, const qrd_blmb_state s,
                                                          const qrd_blm_opts o)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) batch) return;
    if (s.b.status[q] != 0 || s.b.info[q] != 0) return;
    blm_update_member(Ft + q * sF, m, n, q, lane, s.b, o, s.clipped[q] != 0);
}

__global__ void __launch_bounds__(256) blmb_peg_kernel(double* __restrict__ J, int m, int ldj, size_t sJ, const double* __restrict__ Fv, size_t sF,
                                                       int n, int batch, const qrd_blmb_state s)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) batch) return;
    if (s.b.status[q] != 0 || s.b.info[q] != 0) return;
    const size_t qn = q * (size_t) n;
    double* Jq = J + q * sJ;
    const double* f = Fv + q * sF;
    for (int j = 0; j < n; ++j) {
        const double x = s.b.x[qn + j];       // (the same words in every lane: the branches below are wave-uniform)
        const bool atlo = x == s.lo[qn + j], athi = x == s.hi[qn + j];
        int pg = 0;
        if (atlo || athi) {
            double* col = Jq + (size_t) j * ldj;
            double acc = 0.0;
            for (int i = lane; i < m; i += 64) acc = fma(col[i], f[i], acc);
            const double g = qb_wave_sum(acc);
            if (atlo && g > 0.0) pg = -1;
            else if (athi && g < 0.0) pg = 1;
            if (pg != 0)
                for (int i = lane; i < m; i += 64) col[i] = 0.0;
        }
        if (lane == 0) s.peg[qn + j] = pg;
    }
}

__global__ void __launch_bounds__(256) blm_start_kernel(const double* __restrict__ X0, size_t sX, const double* __restrict__ D0, size_t sD, int n,
                                                        int batch, const qrd_blm_state s, int mode)
{
    const size_t q = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t) batch) return;
    blm_start_member(X0, sX, D0, sD, n, q, s, mode);
}

__global__ void __launch_bounds__(256) blmb_start_kernel(const double* __restrict__ X0, size_t sX, const double* __restrict__ D0, size_t sD,
                                                         const double* __restrict__ Lo, size_t sLo, const double* __restrict__ Hi, size_t sHi, int n,
                                                         int batch, const qrd_blmb_state s, int mode)
{
    const size_t q = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t) batch) return;
    const size_t qn = q * (size_t) n;
    bool bad = false;
    for (int i = 0; i < n; ++i) {
        const double lo = Lo ? Lo[q * sLo + i] : -HUGE_VAL, hi = Hi ? Hi[q * sHi + i] : HUGE_VAL, x = X0[q * sX + i];
        bad = bad || !(lo <= hi) || x < lo || x > hi;
    }
    if (bad) {
        s.b.info[q] = -2;
        return;
    }
    blm_start_member(X0, sX, D0, sD, n, q, s.b, mode);
    for (int i = 0; i < n; ++i) {
        s.lo[qn + i] = Lo ? Lo[q * sLo + i] : -HUGE_VAL;
        s.hi[qn + i] = Hi ? Hi[q * sHi + i] : HUGE_VAL;
        s.peg[qn + i] = 0;
    }
    s.alpha[q] = 1.0;
    s.clipped[q] = 0;
}

static int blmb_bad_state(const qrd_blmb_state* s) { return blm_bad_state(&s->b) || !s->lo || !s->hi || !s->alpha || !s->peg || !s->clipped; }

// the kernels of one instantiation that may ask for more than 64 KiB of LDS (qr_allow_lds)
template <class A>
static int blm_allow_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(blm_step_wg_kernel<A>), reinterpret_cast<const void*>(blm_step_wave_kernel<32, A>)};
    return qr_allow_lds(fns, QB_LDS_CAP, done);
}

// the step of every running member from factors that exist: one launch.  -7: shape not taken.  bad_state: the refusal of A's state struct
template <class A, class S>
static int blm_step_launch(void* stream, const A* a, int (*bad_state)(const S*))
{
    if (!a || a->d.batch <= 0) return 0;
    const qrd_bd_args* d = &a->d;
    if (d->n < 1 || d->n + 1 > QRD_B_MAX_N || d->nrhs != 1 || d->nlam != 1 || !d->R || !d->Z || d->ldr < d->n || d->zrows < d->n ||
        d->ldz < d->zrows || d->flip || d->D || bad_state(&a->s) || !(a->o.par_rtol > 0.0 && a->o.par_rtol < 1.0) || a->o.par_maxit < 1)
        return -7;
    const int rc = blm_allow_lds<A>();
    if (rc) return rc;
    hipStream_t s = (hipStream_t) stream;
    const int ntot = d->n + 1;
    if (qrd_bd_wave_route(ntot)) {
        const dim3 grid((unsigned) (((size_t) d->batch + 3) / 4));
        if (ntot <= 4) hipLaunchKernelGGL((blm_step_wave_kernel<4, A>), grid, dim3(256), bt_wave_lds<4>(), s, *a);
        else if (ntot <= 8) hipLaunchKernelGGL((blm_step_wave_kernel<8, A>), grid, dim3(256), bt_wave_lds<8>(), s, *a);
        else if (ntot <= 16) hipLaunchKernelGGL((blm_step_wave_kernel<16, A>), grid, dim3(256), bt_wave_lds<16>(), s, *a);
        else hipLaunchKernelGGL((blm_step_wave_kernel<32, A>), grid, dim3(256), bt_wave_lds<32>(), s, *a);
    } else {
        hipLaunchKernelGGL(blm_step_wg_kernel<A>, dim3((unsigned) d->batch), dim3(256), blm_wg_lds(d->n), s, *a);
    }
    return (int) hipGetLastError();
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

int qrd_blm_step(void* stream, const qrd_blm_step_args* a) { return blm_step_launch(stream, a, blm_bad_state); }

int qrd_blm_update(void* stream, const double* Ft, int m, int ldf, size_t sF, int n, int batch, const qrd_blm_state* s, const qrd_blm_opts* o)
{
    if (batch <= 0) return 0;
    if (!s || !o || blm_bad_state(s) || !Ft || n < 1 || n + 1 > QRD_B_MAX_N || m < 1 || ldf < m) return -7;
    hipLaunchKernelGGL(blm_update_kernel, dim3((unsigned) (((size_t) batch + 3) / 4)), dim3(256), 0, (hipStream_t) stream, Ft, m, ldf, sF, n, batch,
                       *s, *o);
    return (int) hipGetLastError();
}

int qrd_blmb_start(void* stream, const double* X0, int ldx, size_t sX, const double* D0, size_t sD, const double* Lo, size_t sLo,
                   const double* Hi, size_t sHi, int n, int batch, const qrd_blmb_state* s, int mode)
{
    if (batch <= 0) return 0;
    if (!s || blmb_bad_state(s) || !X0 || n < 1 || n + 1 > QRD_B_MAX_N || ldx < n || (mode == 2 && !D0)) return -7;
    hipLaunchKernelGGL(blmb_start_kernel, dim3((unsigned) (((size_t) batch + 255) / 256)), dim3(256), 0, (hipStream_t) stream, X0, sX, D0, sD, Lo,
                       sLo, Hi, sHi, n, batch, *s, mode);
    return (int) hipGetLastError();
}

int qrd_blmb_peg(void* stream, double* J, int m, int ldj, size_t sJ, const double* F, size_t sF, int n, int batch, const qrd_blmb_state* s)
{
    if (batch <= 0) return 0;
    if (!s || blmb_bad_state(s) || !J || !F || n < 1 || n + 1 > QRD_B_MAX_N || m < 1 || ldj < m || sJ < (size_t) ldj * (size_t) n || sF < (size_t) m)
        return -7;
    hipLaunchKernelGGL(blmb_peg_kernel, dim3((unsigned) (((size_t) batch + 3) / 4)), dim3(256), 0, (hipStream_t) stream, J, m, ldj, sJ, F, sF, n,
                       batch, *s);
    return (int) hipGetLastError();
}

int qrd_blmb_step(void* stream, const qrd_blmb_step_args* a) { return blm_step_launch(stream, a, blmb_bad_state); }

int qrd_blmb_update(void* stream, const double* Ft, int m, int ldf, size_t sF, int n, int batch, const qrd_blmb_state* s, const qrd_blm_opts* o)
{
    if (batch <= 0) return 0;
    if (!s || !o || blmb_bad_state(s) || !Ft || n < 1 || n + 1 > QRD_B_MAX_N || m < 1 || ldf < m) return -7;
    hipLaunchKernelGGL(blmb_update_kernel, dim3((unsigned) (((size_t) batch + 3) / 4)), dim3(256), 0, (hipStream_t) stream, Ft, m, sF, n, batch, *s,
                       *o);
    return (int) hipGetLastError();
}

}   // extern "C"
