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
#include "qr_batched_lm_dev.h"      // blm_scalars, blm_finish, blm_fail, the update and the start: shared with qr_batched_lmb.hip

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
    blm_update_member(Ft + q * sF, m, n, q, lane, s, o, false);
}

__global__ void __launch_bounds__(256) blm_start_kernel(const double* __restrict__ X0, size_t sX, const double* __restrict__ D0, size_t sD, int n,
                                                        int batch, const qrd_blm_state s, int mode)
{
    const size_t q = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t) batch) return;
    blm_start_member(X0, sX, D0, sD, n, q, s, mode);
}

// the kernels that may ask for more than 64 KiB of LDS (qb_allow_lds)
static int blm_allow_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(blm_step_wg_kernel), reinterpret_cast<const void*>(blm_step_wave_kernel<32>)};
    return qb_allow_lds(fns, done);
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
