// qr_batched_update.hip -- kernels of the batched row append / removal (qr_batched_update.c, mi355x_qr.h section 8d): for every member of
// a batch the n x n triangle R stacked on a block of p rows whose first p_add rows are added and whose last p - p_add rows are removed,
// R'^T R' = R^T R + B^T S B, S = diag(+1 .. +1, -1 .. -1), with nrhs right-hand sides riding along as extra columns [Z ; C2].
//
//   bu_wave_kernel<W>  n + nrhs <= W <= 32, p <= 64: one wave per member, four members per workgroup.  Lane i holds row i of [B | C2] in W
//                      registers, lane j < n holds row j of [R | Z] in W more; sums are wave butterflies; no LDS, no barrier
//   bu_wg_kernel       everything else within qr_tpqrt_batched_max_rows: one workgroup per member, [B | C2] resident in LDS at a leading
//                      dimension of 2 mod 32 and [R | Z] beside it at an odd one; thread t owns block row t (th_panel_kernel,
//                      qr_update.hip, without T); the trailing update is rank-1, one wave per column
//   bu_apply_kernel    the stored reflectors applied to later right-hand sides [C1 ; C2], V and tau resident in LDS, one wave per column
//   bu_solve_prep_kernel   X <- Z and resid <- sqrt(rss) per member, ahead of qrd_b_trsm
//
// Per column the arithmetic is th_panel_kernel's: with sa / sd the sums of squares of the added / removed rows, h = hypot(alpha,
// sqrt(sa)) (bu_hypot below), nd = sqrt(sd), d = (h - nd) (h + nd), beta = -sign(alpha) sqrt(d), tau = (beta - alpha) / beta,
// v = b / (alpha - beta); a block column that is exactly zero gives tau = 0 and touches nothing; d <= 0 or not finite is the failure.
// Reflector j is Theta_j = I - tau_j u_j u_j^T Phi, u_j = [e_j ; v_j], Phi = diag(I, S): only the products that contract over the
// block's rows see S (the operand is negated by the row index: row >= p_add); the rank-one corrections along u_j do not.
//
// A member is all or nothing: everything is held in registers or LDS until its last column went through, and a member that fails (or,
// in the accumulator mode, would be left with fewer than n rows) writes its info word and nothing else.
//
// The two modes.  Primitive (acc == 0): V goes back over the block, tau (n per member) is written.  Accumulator (acc != 0): the block is
// read only -- rows [0, p_add) from one pair of buffers, rows [p_add, p) from another, so a slide needs no staging copy --, nothing but
// R, Z, the residual sums rss <- max(0, rss + |E_add|^2 - |E_del|^2) (E = what is left in the block rows of the right-hand sides) and the
// row count is written.
//
// Every sum runs in a fixed order that (n, nrhs, p_add, p_del) alone fix (wave butterflies, waves added in wave order, serial loops):
// repeated launches are bitwise equal and a member's result does not depend on the batch count or its index.  No atomics.
//
// From qr_batched_dev.h: the wave helpers, the leading dimension and the LDS cap (the opt-in is qr_common.h's).  The column step and its scalars are this file's
// own: the signed sums and bu_hypot are another formula than dlarfg's, on purpose.
#include "qr_batched_dev.h"

#define BU_MAXN QRD_B_MAX_N
#define BU_P QRD_BU_MAXROWS              // one block row per thread
#define BU_P_WIDE QRD_BU_MAXROWS_WIDE    // what 33 .. 64 columns leave

// the block image is at qb_ld(p); the triangle's leading dimension: the smallest odd value >= n
__host__ __device__ constexpr int bu_lr(int n) { return n | 1; }
// doubles of LDS of the workgroup route: the two images, tau[64], red[8]
__host__ __device__ constexpr size_t bu_wg_doubles(int n, int ntot, int p) { return (size_t) ntot * (qb_ld(p) + bu_lr(n)) + BU_MAXN + 8; }

static_assert(QRD_B_MAX_N == 64 && BU_P == 256, "at most 64 columns, one block row per thread of a 256-thread workgroup");
static_assert(sizeof(double) * bu_wg_doubles(32, 32, BU_P) <= QB_LDS_CAP, "256 rows fit beside 32 columns");
static_assert(sizeof(double) * bu_wg_doubles(64, 64, BU_P_WIDE) <= QB_LDS_CAP, "BU_P_WIDE rows fit beside the unpacked 64 x 65 triangle");
static_assert(sizeof(double) * bu_wg_doubles(64, 64, BU_P_WIDE + 1) > QB_LDS_CAP, "and no row more: the next leading dimension is 258");

// hypot(x, y) with the sum of squares carried in two doubles and rounded once (error just above half an ulp).  The library function is
// good to an ulp -- on an MI355X it was one ulp off the nearest double on 3 of 9 Gaussian pairs -- which is more than the Gram bound
// n eps leaves at n = 1: there R' IS this value (sqrt(x * x) == |x| on the device, so the rest of the column's chain is exact).  The
// operands are scaled by the power of two of the larger one, so the result is exactly homogeneous under scaling by powers of two, and
// overflow-free.  Contraction is off: fusing q into the sum p + q would leave `se` holding a rounding that never happened.
__device__ __forceinline__ double bu_hypot(double x, double y)
{
#pragma clang fp contract(off)
    double a = fabs(x), b = fabs(y);
    if (a < b) { const double t = a; a = b; b = t; }
    if (!(a < INFINITY)) return a + b;       // (inf or NaN: the caller's test of d sees it)
    if (b == 0.0) return a;
    int e;
    (void) frexp(a, &e);
    a = ldexp(a, -e);
    b = ldexp(b, -e);                         // (a in [1/2, 1), b <= a; a b that underflows here is below a's rounding)
    const double p = a * a, pe = fma(a, a, -p), q = b * b, qe = fma(b, b, -q);
    const double s = p + q, se = q - (s - p);                    // (p >= q: the fast two-sum is exact)
    const double r = sqrt(s);
    const double corr = (fma(-r, r, s) + ((se + pe) + qe)) / (2.0 * r);
    return ldexp(r + corr, e);
}

// entry (i, c) of the member's block image [B | C2]: rows [0, p_add) come from the first pair of buffers, the rest from the second
__device__ __forceinline__ double* bu_src(const qrd_bu_args& a, size_t q, int i, int c)
{
    if (i < a.p_add) return c < a.n ? a.A0 + q * a.sA0 + (size_t) c * a.lda0 + i : a.C0 + q * a.sC0 + (size_t) (c - a.n) * a.ldc0 + i;
    i -= a.p_add;
    return c < a.n ? a.A1 + q * a.sA1 + (size_t) c * a.lda1 + i : a.C1 + q * a.sC1 + (size_t) (c - a.n) * a.ldc1 + i;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// wave route
// ---------------------------------------------------------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(256) bu_wave_kernel(const qrd_bu_args a)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) a.batch) return;        // (no barrier anywhere below: the waves of a workgroup are independent)
    const int n = a.n, ntot = a.n + a.nrhs, p = a.p, p_add = a.p_add;
    int held = 0;
    if (a.acc) {
        held = a.rows[q];
        if (p > p_add && held + p_add - (p - p_add) < n) {       // fewer than n rows would be left: decided before any arithmetic
            if (lane == 0) a.info[q] = -1;
            return;                           // (the whole wave: `held` is the same in every lane)
        }
    }
    double* Rq = a.R + q * a.sR;
    double* Zq = a.nrhs ? a.Z + q * a.sZ : nullptr;
    const bool brow = lane < p, rrow = lane < n, neg = lane >= p_add;
    double b[W], r[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
        b[c] = (brow && c < ntot) ? *bu_src(a, q, lane, c) : 0.0;
        double v = 0.0;
        if (rrow && c < n) v = lane <= c ? Rq[(size_t) c * a.ldr + lane] : 0.0;      // (the strict lower triangle is not read)
        else if (rrow && c < ntot) v = Zq[(size_t) (c - n) * a.ldz + lane];
        r[c] = v;
    }
    double tauv = 0.0;                        // lane j: tau[j]
#pragma unroll
    for (int j = 0; j < W; ++j) {
        if (j < n) {                          // (wave-uniform)
            const double x = b[j], x2 = x * x;                   // (rows >= p hold zeros)
            const double sa = qb_wave_sum(neg ? 0.0 : x2), sd = qb_wave_sum(neg ? x2 : 0.0);
            if (sa != 0.0 || sd != 0.0) {     // (the same values in every lane)
                const double alpha = qb_bcast(r[j], j);
                const double h = bu_hypot(alpha, sqrt(sa)), nd = sqrt(sd), d = (h - nd) * (h + nd);
                if (!(d > 0.0) || !isfinite(d)) {
                    if (lane == 0 && a.info) a.info[q] = j + 1;
                    return;                   // (the whole wave; nothing has been written back)
                }
                const double beta = -copysign(sqrt(d), alpha);
                const double tj = (beta - alpha) / beta, scal = 1.0 / (alpha - beta);
                const double v = x * scal, sv = neg ? -v : v;
#pragma unroll
                for (int c = j + 1; c < W; ++c) {
                    if (c < ntot) {
                        const double tw = tj * (qb_bcast(r[c], j) + qb_wave_sum(sv * b[c]));
                        if (lane == j) r[c] -= tw;
                        b[c] = fma(-tw, v, b[c]);
                    }
                }
                b[j] = v;
                if (lane == j) { r[j] = beta; tauv = tj; }
            }
        }
    }
    // the member went through: only now is anything written.  An accumulator that holds fewer than n rows has rank at most that many:
    // the rows of [R | Z] from its row count on are zero in exact arithmetic and are stored as exact zeros (what the elimination left
    // there is rounding), so the solve's test of the diagonal reports such a member
    const int now = held + p_add - (p - p_add);
    const bool keep = !a.acc || lane < now;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        if (c < n) {
            if (rrow && lane <= c) Rq[(size_t) c * a.ldr + lane] = keep ? r[c] : 0.0;
        } else if (c < ntot) {
            if (rrow) Zq[(size_t) (c - n) * a.ldz + lane] = keep ? r[c] : 0.0;
        }
    }
    if (a.acc) {
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (c >= n && c < ntot) {
                const double e2 = b[c] * b[c];
                const double ea = qb_wave_sum(neg ? 0.0 : e2), ed = qb_wave_sum(neg ? e2 : 0.0);
                double* s = a.rss + q * (size_t) a.nrhs + (c - n);
                if (lane == 0) *s = fmax(0.0, (*s + ea) - ed);
            }
        }
        if (lane == 0) a.rows[q] = now;
    } else {
#pragma unroll
        for (int c = 0; c < W; ++c)
            if (brow && c < ntot) *bu_src(a, q, lane, c) = b[c];
        if (rrow) a.tau[q * a.stau + lane] = tauv;
    }
    if (lane == 0 && a.info) a.info[q] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// workgroup route.  LDS: Bs[c * ld + i] = [B | C2](i, c), ld = qb_ld(p); Rs[c * lr + r] = [R | Z](r, c), lr = bu_lr(n); ts[64]; red[8].
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bu_wg_kernel(const qrd_bu_args a)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const int n = a.n, ntot = a.n + a.nrhs, p = a.p, p_add = a.p_add;
    const int ld = qb_ld(p), lr = bu_lr(n);
    int held = 0;
    if (a.acc) {
        held = a.rows[q];
        // fewer than n rows would be left.  `held` is one word read by every thread of the workgroup, and nothing in this launch writes
        // it before the last barrier: the test is the same in all 256 threads, which leave together, before the first barrier.
        if (p > p_add && held + p_add - (p - p_add) < n) {
            if (t == 0) a.info[q] = -1;
            return;
        }
    }
    double* Bs = sm;
    double* Rs = Bs + (size_t) ntot * ld;
    double* ts = Rs + (size_t) ntot * lr;
    double* red = ts + BU_MAXN;              // 4 partial sums of the added rows, 4 of the removed ones
    double* Rq = a.R + q * a.sR;
    double* Zq = a.nrhs ? a.Z + q * a.sZ : nullptr;
    for (int c = wv; c < ntot; c += 4)
        for (int i = lane; i < p; i += 64) Bs[c * ld + i] = *bu_src(a, q, i, c);
    for (int idx = t; idx < ntot * n; idx += 256) {
        const int c = idx / n, r = idx - c * n;
        Rs[c * lr + r] = c < n ? (r <= c ? Rq[(size_t) c * a.ldr + r] : 0.0) : Zq[(size_t) (c - n) * a.ldz + r];
    }
    if (t < BU_MAXN) ts[t] = 0.0;
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        double* vj = Bs + j * ld;
        // thread t owns row t (p <= 256): its square goes to the sum of its sign
        const double x = t < p ? vj[t] : 0.0, x2 = x * x;
        const double sa_w = qb_wave_sum(t < p_add ? x2 : 0.0), sd_w = qb_wave_sum(t < p_add ? 0.0 : x2);
        if (lane == 0) { red[wv] = sa_w; red[4 + wv] = sd_w; }
        __syncthreads();
        const double sa = ((red[0] + red[1]) + red[2]) + red[3], sd = ((red[4] + red[5]) + red[6]) + red[7];
        if (sa != 0.0 || sd != 0.0) {        // (the same values in every thread)
            const double alpha = Rs[j * lr + j];
            const double h = bu_hypot(alpha, sqrt(sa)), nd = sqrt(sd), d = (h - nd) * (h + nd);
            // The failure exit.  sa, sd and alpha were read from LDS words that no thread writes between the barrier above and this
            // point (red is rewritten only after the barrier that ends the column, Rs(j, j) only after the one below), so d is the
            // same double in all 256 threads: either every thread of the workgroup returns here or none does, and no thread is left
            // waiting at a later barrier.  Nothing has been written to global memory yet -- R, Z, V, tau, rss and the row count are
            // written after the column loop -- so the member stays bitwise what it was.
            if (!(d > 0.0) || !isfinite(d)) {
                if (t == 0 && a.info) a.info[q] = j + 1;
                return;
            }
            const double beta = -copysign(sqrt(d), alpha);
            const double tau = (beta - alpha) / beta, scal = 1.0 / (alpha - beta);
            if (t < p) vj[t] = x * scal;
            __syncthreads();
            if (t == 0) { Rs[j * lr + j] = beta; ts[j] = tau; }
            // wave wv: columns j + 1 + wv, + 4, ..: the signed dot product with v_j, then that column's update
            for (int c = j + 1 + wv; c < ntot; c += 4) {
                double* bc = Bs + c * ld;
                double dt = 0.0;
                for (int i = lane; i < p; i += 64) dt = fma(i < p_add ? vj[i] : -vj[i], bc[i], dt);
                dt = qb_wave_sum(dt);
                const double tw = tau * (Rs[c * lr + j] + dt);
                for (int i = lane; i < p; i += 64) bc[i] = fma(-tw, vj[i], bc[i]);
                if (lane == 0) Rs[c * lr + j] -= tw;     // (read by every lane above: the wave runs in lock step up to the butterfly)
            }
        }
        __syncthreads();                     // (red and column j are read no more)
    }
    // the member went through: only now is anything written.  (The rows of [R | Z] from an accumulator's row count on: exact zeros, as
    // in bu_wave_kernel.)
    const int now = held + p_add - (p - p_add);
    for (int idx = t; idx < ntot * n; idx += 256) {
        const int c = idx / n, r = idx - c * n;
        const double v = (!a.acc || r < now) ? Rs[c * lr + r] : 0.0;
        if (c >= n) Zq[(size_t) (c - n) * a.ldz + r] = v;
        else if (r <= c) Rq[(size_t) c * a.ldr + r] = v;
    }
    if (a.acc) {
        for (int c = n + wv; c < ntot; c += 4) {
            const double* bc = Bs + c * ld;
            double ea = 0.0, ed = 0.0;
            for (int i = lane; i < p; i += 64) {
                const double e2 = bc[i] * bc[i];
                if (i < p_add) ea += e2;
                else ed += e2;
            }
            ea = qb_wave_sum(ea);
            ed = qb_wave_sum(ed);
            double* s = a.rss + q * (size_t) a.nrhs + (c - n);
            if (lane == 0) *s = fmax(0.0, (*s + ea) - ed);
        }
        if (t == 0) a.rows[q] = now;
    } else {
        for (int c = wv; c < ntot; c += 4)
            for (int i = lane; i < p; i += 64) *bu_src(a, q, i, c) = Bs[c * ld + i];
        if (t < n) a.tau[q * a.stau + t] = ts[t];
    }
    if (t == 0 && a.info) a.info[q] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// [C1 ; C2] <- Theta_{n-1} .. Theta_0 [C1 ; C2] (tr != 0: the transformation that took [R ; B] to [R' ; 0]) or, for p_add == p only,
// its inverse H_0 .. H_{n-1} (tr == 0).  LDS: Vs[c * ld + i] = V(i, c), then tau[64].  A wave takes a column: lane j < n holds C1(j), row
// lane + 64 k of C2 is in register k -- RR = 1, 2 or 4, the smallest that holds p rows.  (A register beyond p adds exact zeros.)
// ---------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr size_t bu_apply_doubles(int n, int p) { return (size_t) n * qb_ld(p) + BU_MAXN; }
static_assert(sizeof(double) * bu_apply_doubles(32, BU_P) <= QB_LDS_CAP && sizeof(double) * bu_apply_doubles(64, BU_P_WIDE) <= QB_LDS_CAP,
              "V fits wherever the update that wrote it did");

template <int RR>
__global__ void __launch_bounds__(256) bu_apply_kernel(int tr, const double* __restrict__ V, int p, int p_add, int n, int ldv, size_t strideV,
                                                       const double* __restrict__ tau, size_t stridetau, double* __restrict__ C1, int ldc1,
                                                       size_t strideC1, double* __restrict__ C2, int ldc2, size_t strideC2, int nrhs)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const int ld = qb_ld(p);
    double* Vs = sm;
    double* ts = Vs + (size_t) n * ld;
    const double* Vq = V + q * strideV;
    for (int c = wv; c < n; c += 4)
        for (int i = lane; i < p; i += 64) Vs[c * ld + i] = Vq[(size_t) c * ldv + i];
    if (t < n) ts[t] = tau[q * stridetau + t];
    __syncthreads();
    for (int col = (int) blockIdx.y * 4 + wv; col < nrhs; col += (int) gridDim.y * 4) {       // (wave-uniform)
        double* c1p = C1 + q * strideC1 + (size_t) col * ldc1;
        double* c2p = C2 + q * strideC2 + (size_t) col * ldc2;
        double c1 = lane < n ? c1p[lane] : 0.0;
        double c[RR];
#pragma unroll
        for (int k = 0; k < RR; ++k) {
            const int i = lane + 64 * k;
            c[k] = i < p ? c2p[i] : 0.0;
        }
        for (int jj = 0; jj < n; ++jj) {
            const int j = tr ? jj : n - 1 - jj;
            const double tj = ts[j];
            if (tj == 0.0) continue;          // (Theta = I; wave-uniform)
            const double* vj = Vs + j * ld;
            double v[RR];
            double d = 0.0;
#pragma unroll
            for (int k = 0; k < RR; ++k) {
                const int i = lane + 64 * k;
                v[k] = i < p ? vj[i] : 0.0;
                d = fma(i < p_add ? v[k] : -v[k], c[k], d);
            }
            const double tw = tj * (qb_bcast(c1, j) + qb_wave_sum(d));
            if (lane == j) c1 -= tw;
#pragma unroll
            for (int k = 0; k < RR; ++k) c[k] = fma(-tw, v[k], c[k]);
        }
        if (lane < n) c1p[lane] = c1;
#pragma unroll
        for (int k = 0; k < RR; ++k) {
            const int i = lane + 64 * k;
            if (i < p) c2p[i] = c[k];
        }
    }
}

// X_q <- Z_q (n x nrhs, packed at ld n) and resid[q, :] <- sqrt(rss[q, :]) (resid may be NULL)
__global__ void __launch_bounds__(256) bu_solve_prep_kernel(const double* __restrict__ Z, int n, int nrhs, double* __restrict__ X, int ldx,
                                                            size_t strideX, const double* __restrict__ rss, double* __restrict__ resid,
                                                            size_t strideresid)
{
    const size_t q = blockIdx.x;
    const double* Zq = Z + q * (size_t) n * nrhs;
    double* Xq = X + q * strideX;
    for (int idx = threadIdx.x; idx < n * nrhs; idx += 256) {
        const int c = idx / n, r = idx - c * n;
        Xq[(size_t) c * ldx + r] = Zq[idx];
    }
    if (resid)
        for (int c = threadIdx.x; c < nrhs; c += 256) resid[q * strideresid + c] = sqrt(rss[q * (size_t) nrhs + c]);
}

// the kernels that may ask for more than 64 KiB of LDS (qr_allow_lds)
static int bu_allow_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(bu_wg_kernel), reinterpret_cast<const void*>(bu_apply_kernel<1>),
                               reinterpret_cast<const void*>(bu_apply_kernel<2>), reinterpret_cast<const void*>(bu_apply_kernel<4>)};
    return qr_allow_lds(fns, QB_LDS_CAP, done);
}

extern "C" {

int qrd_bu_max_rows(int ncols)
{
    if (ncols < 1 || ncols > QRD_B_MAX_N) return 0;
    return ncols <= 32 ? BU_P : BU_P_WIDE;
}

int qrd_bu_wave_route(int ncols, int p) { return ncols <= 32 && p <= 64; }

int qrd_bu_update(void* stream, const qrd_bu_args* a)
{
    if (!a || a->batch <= 0) return 0;
    const int ntot = a->n + a->nrhs, p = a->p;
    if (a->n < 1 || a->nrhs < 0 || ntot > QRD_B_MAX_N || p < 1 || p > qrd_bu_max_rows(ntot) || a->p_add < 0 || a->p_add > p || !a->R ||
        a->ldr < a->n || (a->nrhs && (!a->Z || a->ldz < a->n)) || (a->acc ? (!a->rows || (a->nrhs && !a->rss)) : !a->tau) ||
        (!a->info && (a->p_add < p)))
        return -7;
    if (a->p_add > 0 && (!a->A0 || a->lda0 < a->p_add || (a->nrhs && (!a->C0 || a->ldc0 < a->p_add)))) return -7;
    if (a->p_add < p && (!a->A1 || a->lda1 < p - a->p_add || (a->nrhs && (!a->C1 || a->ldc1 < p - a->p_add)))) return -7;
    hipStream_t s = (hipStream_t) stream;
    if (qrd_bu_wave_route(ntot, p)) {
        const dim3 grid((unsigned) (((size_t) a->batch + 3) / 4));
        if (ntot <= 4) hipLaunchKernelGGL(bu_wave_kernel<4>, grid, dim3(256), 0, s, *a);
        else if (ntot <= 8) hipLaunchKernelGGL(bu_wave_kernel<8>, grid, dim3(256), 0, s, *a);
        else if (ntot <= 16) hipLaunchKernelGGL(bu_wave_kernel<16>, grid, dim3(256), 0, s, *a);
        else hipLaunchKernelGGL(bu_wave_kernel<32>, grid, dim3(256), 0, s, *a);
    } else {
        const int rc = bu_allow_lds();
        if (rc) return rc;
        hipLaunchKernelGGL(bu_wg_kernel, dim3((unsigned) a->batch), dim3(256), sizeof(double) * bu_wg_doubles(a->n, ntot, p), s, *a);
    }
    return (int) hipGetLastError();
}

int qrd_bu_apply(void* stream, int trans_t, const double* V, int p, int p_add, int n, int ldv, size_t strideV, const double* tau,
                 size_t stridetau, double* C1, int ldc1, size_t strideC1, double* C2, int ldc2, size_t strideC2, int nrhs, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || n > QRD_B_MAX_N || p < 1 || p > qrd_bu_max_rows(n) || p_add < 0 || p_add > p || (!trans_t && p_add != p) || ldv < p || ldc1 < n ||
        ldc2 < p || nrhs < 1)
        return -7;
    const int rc = bu_allow_lds();
    if (rc) return rc;
    int gy = (nrhs + 15) / 16;                // four columns per wave; beyond 1024 workgroups per member the waves loop
    if (gy > 1024) gy = 1024;
    const dim3 grid((unsigned) batch, (unsigned) gy);
    const size_t lds = sizeof(double) * bu_apply_doubles(n, p);
    hipStream_t s = (hipStream_t) stream;
#define BU_APPLY(RR) hipLaunchKernelGGL(bu_apply_kernel<RR>, grid, dim3(256), lds, s, trans_t, V, p, p_add, n, ldv, strideV, tau, stridetau, C1, ldc1, strideC1, C2, ldc2, strideC2, nrhs)
    if (p <= 64) BU_APPLY(1);
    else if (p <= 128) BU_APPLY(2);
    else BU_APPLY(4);
#undef BU_APPLY
    return (int) hipGetLastError();
}

int qrd_bu_solve_prep(void* stream, const double* Z, int n, int nrhs, double* X, int ldx, size_t strideX, const double* rss, double* resid,
                      size_t strideresid, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || nrhs < 1 || ldx < n || !Z || !X || !rss) return -7;
    hipLaunchKernelGGL(bu_solve_prep_kernel, dim3((unsigned) batch), dim3(256), 0, (hipStream_t) stream, Z, n, nrhs, X, ldx, strideX, rss, resid,
                       strideresid);
    return (int) hipGetLastError();
}

}   // extern "C"
