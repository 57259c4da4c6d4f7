// qr_batched_lse.hip -- kernels of the batched equality-constrained least squares (qr_batched_lse.c, mi355x_qr.h section 8h): per member of
// a batch min |A x - b| subject to C x = d (A: m x n, C: p x n, 1 <= p <= n, m + p >= n) by the null-space method, one launch:
//
//   1. C^T = Q_c [R_c ; 0]       the Householder column step of section 8 on C read through the transposed index map (n x p, tall)
//   2. R_c^T y1 = d              forward substitution
//   3. A~ = A Q_c                H_0 .. H_{p-1} from the right: every row of A takes row -= tau_j (row . v_j) v_j^T, rows independent
//   4. r = b - A~(:, 0:p) y1
//   5. the column step on A~2 = A~(:, p:n) (m x (n - p)), A~1 = A~(:, 0:p) and r riding along: G = Q_a^T A~1, t = Q_a^T r; R_a y2 = t(0:n-p)
//   6. x = Q_c [y1 ; y2]         the reflectors p-1 .. 0
//   7. resid = |t(n-p : m)|      which is |A x - b|
//   8. R_c lambda = g            g_i = sum over rows >= n-p of G(row, i) t(row): A^T (A x - b) + C^T lambda = 0
//
// The image of A holds its columns in the order [A~2 | A~1 | rhs]: image column c is A's column c + p for c < n - p and A's column
// c - (n - p) for n - p <= c < n.  Column j of the second factorisation then pivots on row j and the shared column steps
// (qr_batched_dev.h) are called unchanged, with the end of the update at n + nrhs: exactly the columns that ride along.
//
//   bl_wave_kernel<W>  m <= 64 and n + nrhs <= W <= 32: one wave per member, four members per workgroup, no workgroup barrier.  Lane i
//                      holds row i of C^T in W registers, factors it (qb_wave_col), spills the factors to the wave's LDS and reloads the
//                      registers with row i of A.  In the sweep from the right every register index is a constant of the unrolled loop;
//                      only the LDS address of v_j's element is computed at run time, the same in every lane (a broadcast)
//   bl_wg_kernel       everything else that fits: one workgroup per member, [A~2 | A~1 | rhs] in LDS at qb_ld(m), the factors of C^T
//                      beside it at qb_ld(n) (qb_wg_col on both), a thread per row in the sweep from the right.  The two info decisions
//                      are taken by thread 0 and published through an LDS word that all threads read after a barrier
//
// info: 0; i + 1 for the smallest i with R_c(i,i) == 0 exactly; p + i + 1 for the smallest i with R_a(i,i) == 0 exactly.  Such a member's
// X, L and resid are not written at all.  Every sum runs in an order that (m, n, p, nrhs) fix; no atomics.
#include "qr_batched_dev.h"

static_assert(QRD_B_MAX_N == 64, "tau of C^T is kept in 64 doubles of LDS");

// A's column behind image column c < n
__device__ __forceinline__ int bl_src(int c, int k, int p) { return c < k ? c + p : c - k; }

// ---------------------------------------------------------------------------------------------------------------------------------
// wave route.  Dynamic LDS per wave, two regions of W x (W + 1) doubles (LW = W + 1):
//   Vs[c * LW + r]   c < p: the factors of C^T (R_c on and above the diagonal, V_c below); p <= c < n: R_a(r, c - p);
//                    n <= c < n + nrhs: g, then lambda, of right-hand side c - n
//   Xs[kk * LW + r]  kk < nrhs <= W - 1: d, then [y1 ; y2]; the last column holds tau of C^T
// ---------------------------------------------------------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(256) bl_wave_kernel(const qrd_bl_args g)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) g.batch) return;        // (no workgroup barrier below: the waves of a workgroup are independent)
    const int m = g.m, n = g.n, p = g.p, nrhs = g.nrhs, k = n - p, ntot = n + nrhs;
    constexpr int LW = W + 1;
    double* Vs = sm + (size_t) wv * 2 * W * LW;
    double* Xs = Vs + W * LW;
    double* tc = Xs + (W - 1) * LW;
    const double* Aq = g.A + q * g.sA;
    const double* Cq = g.C + q * g.sC;
    const double* Bq = g.B + q * g.sB;
    const double* Dq = g.D + q * g.sD;
    double a[W];
    // 1. lane i: row i of C^T, which is column i of C, contiguous
#pragma unroll
    for (int c = 0; c < W; ++c) a[c] = (lane < n && c < p) ? Cq[(size_t) lane * g.ldc + c] : 0.0;
    double tauv = 0.0, diag = 1.0;            // lane j: tau_c[j] and R_c(j, j)
#pragma unroll
    for (int j = 0; j < W; ++j) {
        if (j < p) qb_wave_col<W>(a, j, p, lane, tauv, diag);         // (wave-uniform)
    }
    const int ic = qb_info_wave(diag, p, lane);
    if (ic) {                                 // (all or nothing: nothing else is written)
        if (lane == 0) g.info[q] = ic;
        return;
    }
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (c < p && lane < n) Vs[c * LW + lane] = a[c];
    if (lane < p) tc[lane] = tauv;
    for (int kk = 0; kk < nrhs; ++kk)
        if (lane < p) Xs[kk * LW + lane] = Dq[(size_t) kk * g.ldd + lane];
    QB_WAVE_SYNC();
    // 2. R_c^T y1 = d
    if (lane < nrhs) qb_trsv_t(Vs, LW, p, Xs + lane * LW);    // (nrhs < W <= 32: one lane per right-hand side)
    QB_WAVE_SYNC();
    // lane i: row i of [A~2 | A~1 | rhs] before the sweep
    const bool row = lane < m;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        double v = 0.0;
        if (row && c < n) v = Aq[(size_t) bl_src(c, k, p) * g.lda + lane];
        else if (row && c < ntot) v = Bq[(size_t) (c - n) * g.ldb + lane];
        a[c] = v;
    }
    // 3. row <- row H_0 .. H_{p-1}: no cross-lane sum; v_j(i) is read at the same address by every lane
    for (int j = 0; j < p; ++j) {
        const double tj = tc[j];
        if (tj == 0.0) continue;              // (H = I; wave-uniform)
        const double* vj = Vs + j * LW;
        double d = 0.0;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (c < n) {
                const int i = bl_src(c, k, p);
                if (i >= j) d = fma(a[c], i == j ? 1.0 : vj[i], d);
            }
        }
        const double w = tj * d;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (c < n) {
                const int i = bl_src(c, k, p);
                if (i >= j) a[c] = fma(-w, i == j ? 1.0 : vj[i], a[c]);
            }
        }
    }
    // 4. r = b - A~1 y1: per right-hand side one sum over A~1's columns ascending, then the one register it belongs to takes it (the
    // loop over kk stays a loop: every index into a[] is a constant of the unrolled loops inside it)
    for (int kk = 0; kk < nrhs; ++kk) {
        const double* y = Xs + kk * LW;
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < W; ++c)
            if (c >= k && c < n) s = fma(a[c], y[c - k], s);
#pragma unroll
        for (int cc = 1; cc < W; ++cc)
            if (cc == n + kk) a[cc] -= s;
    }
    // 5. the column step on A~2; A~1 and r ride along
    double taua = 0.0, da = 1.0;              // lane j: R_a(j, j)
#pragma unroll
    for (int j = 0; j < W; ++j) {
        if (j < k) qb_wave_col<W>(a, j, ntot, lane, taua, da);        // (wave-uniform)
    }
    const int ia = qb_info_wave(da, k, lane);
    if (lane == 0) g.info[q] = ia ? p + ia : 0;
    if (ia) return;
    // R_a and the top of t into LDS; 7. and 8.: resid and g from the rows >= n - p (rows >= m hold zeros)
#pragma unroll
    for (int c = 0; c < W; ++c) {
        if (c < k) {
            if (lane < k) Vs[(p + c) * LW + lane] = a[c];
        } else if (c >= n && c < ntot) {
            if (lane < k) Xs[(c - n) * LW + p + lane] = a[c];
        }
    }
    for (int kk = 0; kk < nrhs; ++kk) {
        double tt = 0.0;
#pragma unroll
        for (int cc = 1; cc < W; ++cc)
            if (cc == n + kk) tt = lane >= k ? a[cc] : 0.0;
        if (g.resid) {
            const double ss = qb_wave_sum(tt * tt);
            if (lane == 0) g.resid[q * g.sres + kk] = sqrt(ss);
        }
        if (g.L) {
#pragma unroll
            for (int c = 0; c < W; ++c) {
                if (c >= k && c < n) {
                    const double gi = qb_wave_sum(tt * a[c]);
                    if (lane == 0) Vs[(n + kk) * LW + (c - k)] = gi;
                }
            }
        }
    }
    QB_WAVE_SYNC();
    if (lane < nrhs) {
        qb_trsv(Vs + p * LW, LW, k, Xs + lane * LW + p);          // R_a y2 = t(0 : n-p)
        if (g.L) qb_trsv(Vs, LW, p, Vs + (n + lane) * LW);        // R_c lambda = g
    }
    QB_WAVE_SYNC();
    // 6. x = Q_c [y1 ; y2]: one butterfly per reflector
    double* Xq = g.X + q * g.sX;
    for (int kk = 0; kk < nrhs; ++kk) {
        double x = lane < n ? Xs[kk * LW + lane] : 0.0;
        for (int j = p - 1; j >= 0; --j) {
            const double tj = tc[j];
            if (tj == 0.0) continue;          // (H = I; wave-uniform)
            const double v = lane > j ? (lane < n ? Vs[j * LW + lane] : 0.0) : (lane == j ? 1.0 : 0.0);
            const double tw = tj * qb_wave_sum(v * x);
            x = fma(-tw, v, x);
        }
        if (lane < n) Xq[(size_t) kk * g.ldx + lane] = x;
        if (g.L && lane < p) g.L[q * g.sL + (size_t) kk * g.ldl + lane] = Vs[(n + kk) * LW + lane];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// workgroup route.  LDS: As[c * ld + i] = [A~2 | A~1 | rhs] (n + nrhs columns, ld = qb_ld(m)); Cs[j * ldn + i] = C^T (p columns,
// ldn = qb_ld(n)); Ys[kk * n + r] = d, then [y1 ; y2], then x (nrhs columns of n); Gs[kk * p + i] = g, then lambda; red[4]; a word for
// info, 3 spare; tc[64] (tau of C^T).
// ---------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr size_t bl_wg_doubles(int m, int n, int p, int nrhs)
{
    return (size_t) (n + nrhs) * qb_ld(m) + (size_t) p * qb_ld(n) + (size_t) nrhs * (n + p) + QB_WG_SMALL;
}

__global__ void __launch_bounds__(256) bl_wg_kernel(const qrd_bl_args g)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const int m = g.m, n = g.n, p = g.p, nrhs = g.nrhs, k = n - p, ntot = n + nrhs;
    const int ld = qb_ld(m), ldn = qb_ld(n);
    double* As = sm;
    double* Cs = As + (size_t) ntot * ld;
    double* Ys = Cs + (size_t) p * ldn;
    double* Gs = Ys + (size_t) nrhs * n;
    double* red = Gs + (size_t) nrhs * p;
    int* sinfo = (int*) (red + 4);
    double* tc = red + 8;
    const double* Aq = g.A + q * g.sA;
    const double* Cq = g.C + q * g.sC;
    const double* Bq = g.B + q * g.sB;
    const double* Dq = g.D + q * g.sD;
    for (int i = wv; i < n; i += 4) {         // row i of C^T is column i of C: read along it, write the image transposed
        const double* src = Cq + (size_t) i * g.ldc;
        for (int j = lane; j < p; j += 64) Cs[j * ldn + i] = src[j];
    }
    for (int c = wv; c < ntot; c += 4) {
        const double* src = c < n ? Aq + (size_t) bl_src(c, k, p) * g.lda : Bq + (size_t) (c - n) * g.ldb;
        for (int i = lane; i < m; i += 64) As[c * ld + i] = src[i];
    }
    for (int idx = t; idx < nrhs * p; idx += 256) {
        const int kk = idx / p, i = idx - kk * p;
        Ys[kk * n + i] = Dq[(size_t) kk * g.ldd + i];
    }
    __syncthreads();
    // 1. C^T = Q_c [R_c ; 0]
    for (int j = 0; j < p; ++j) {
        const double tj = qb_wg_col(Cs, ldn, n, j, p, red, t);
        if (t == 0) tc[j] = tj;
        __syncthreads();                      // (red and column j are read no more)
    }
    if (t == 0) *sinfo = qb_info_serial(Cs, ldn, p);
    __syncthreads();
    if (*sinfo) {                             // (all or nothing: nothing else is written)
        if (t == 0) g.info[q] = *sinfo;
        return;
    }
    // 2. R_c^T y1 = d
    if (t < nrhs) qb_trsv_t(Cs, ldn, p, Ys + t * n);          // (nrhs < 64: one thread per right-hand side)
    // 3. a thread per row: row <- row H_0 .. H_{p-1}, each sum over A's columns j .. n-1 ascending
    for (int r = t; r < m; r += 256) {
        double* ar = As + r;
        for (int j = 0; j < p; ++j) {
            const double tj = tc[j];
            if (tj == 0.0) continue;          // (H = I)
            const double* vj = Cs + j * ldn;
            double d = ar[(k + j) * ld];
            for (int i = j + 1; i < p; ++i) d = fma(vj[i], ar[(k + i) * ld], d);
            for (int i = p; i < n; ++i) d = fma(vj[i], ar[(i - p) * ld], d);
            const double w = tj * d;
            ar[(k + j) * ld] -= w;
            for (int i = j + 1; i < p; ++i) ar[(k + i) * ld] = fma(-w, vj[i], ar[(k + i) * ld]);
            for (int i = p; i < n; ++i) ar[(i - p) * ld] = fma(-w, vj[i], ar[(i - p) * ld]);
        }
    }
    __syncthreads();
    // 4. r = b - A~1 y1
    for (int idx = t; idx < nrhs * m; idx += 256) {
        const int kk = idx / m, r = idx - kk * m;
        const double* y = Ys + kk * n;
        double s = As[(n + kk) * ld + r];
        for (int i = 0; i < p; ++i) s = fma(-As[(k + i) * ld + r], y[i], s);
        As[(n + kk) * ld + r] = s;
    }
    __syncthreads();
    // 5. the column step on A~2; A~1 and r ride along
    for (int j = 0; j < k; ++j) {
        qb_wg_col(As, ld, m, j, ntot, red, t);
        __syncthreads();                      // (red and column j are read no more)
    }
    if (t == 0) {
        const int ia = qb_info_serial(As, ld, k);
        g.info[q] = *sinfo = ia ? p + ia : 0;
    }
    __syncthreads();
    if (*sinfo) return;
    // 7. and 8.: wave wv takes the sums (kk, i), i < p: g_i of right-hand side kk; i == p: its resid -- all over rows >= n - p
    const int per = g.L ? p + 1 : 1;
    for (int item = wv; item < nrhs * per; item += 4) {
        const int kk = item / per, i = g.L ? item - kk * per : p;
        const double* tcol = As + (n + kk) * ld;
        const double* gcol = i < p ? As + (k + i) * ld : tcol;
        double s = 0.0;
        for (int r = k + lane; r < m; r += 64) s = fma(gcol[r], tcol[r], s);
        s = qb_wave_sum(s);
        if (lane == 0) {
            if (i < p) Gs[kk * p + i] = s;
            else if (g.resid) g.resid[q * g.sres + kk] = sqrt(s);
        }
    }
    // R_a y2 = t(0 : n-p) (rows < n - p: none of them is read above)
    if (t < nrhs) {
        double* tcol = As + (n + t) * ld;
        qb_trsv(As, ld, k, tcol);
        for (int r = 0; r < k; ++r) Ys[t * n + p + r] = tcol[r];
    }
    __syncthreads();
    // R_c lambda = g
    if (g.L && t < nrhs) {
        double* lam = Gs + t * p;
        qb_trsv(Cs, ldn, p, lam);
        double* dst = g.L + q * g.sL + (size_t) t * g.ldl;
        for (int i = 0; i < p; ++i) dst[i] = lam[i];
    }
    // 6. x = Q_c [y1 ; y2]: wave wv takes right-hand sides wv, wv + 4, ..
    double* Xq = g.X + q * g.sX;
    for (int kk = wv; kk < nrhs; kk += 4) {
        double* xc = Ys + kk * n;
        for (int j = p - 1; j >= 0; --j) {
            const double tj = tc[j];
            if (tj == 0.0) continue;          // (H = I; wave-uniform)
            qb_col_reflect(Cs + j * ldn, xc, j, n, tj, lane);
            QB_WAVE_SYNC();                   // (the next reflector reads the column under another lane map)
        }
        double* dst = Xq + (size_t) kk * g.ldx;
        for (int i = lane; i < n; i += 64) dst[i] = xc[i];
    }
}

// the kernels that may ask for more than 64 KiB of LDS (qr_allow_lds)
static int bl_allow_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(bl_wg_kernel), reinterpret_cast<const void*>(bl_wave_kernel<32>)};
    return qr_allow_lds(fns, QB_LDS_CAP, done);
}

template <int W>
static void bl_launch_wave(hipStream_t s, const qrd_bl_args& a)
{
    const size_t lds = sizeof(double) * 4 * 2 * W * (W + 1);
    hipLaunchKernelGGL(bl_wave_kernel<W>, dim3((unsigned) (((size_t) a.batch + 3) / 4)), dim3(256), lds, s, a);
}

extern "C" {

int qrd_bl_wave_route(int m, int n, int nrhs) { return m <= 64 && n + nrhs <= 32; }

// the largest m the kernels take for (n, p, nrhs); 0: the shape is not taken at all.  The wave route needs no more than the workgroup
// route holds (64 rows of at most 32 columns), so the workgroup route's LDS budget decides.
int qrd_bl_max_rows(int n, int p, int nrhs)
{
    if (n < 1 || p < 1 || p > n || nrhs < 1 || nrhs > QRD_B_MAX_N - n) return 0;
    int m = QRD_B_MAX_ROWS;
    while (m >= 1 && sizeof(double) * bl_wg_doubles(m, n, p, nrhs) > QB_LDS_CAP) --m;
    return m >= 1 && m >= n - p ? m : 0;
}

int qrd_bl_solve(void* stream, const qrd_bl_args* a)
{
    if (!a) return -7;
    if (a->batch <= 0) return 0;
    const int mr = qrd_bl_max_rows(a->n, a->p, a->nrhs);
    if (!mr || a->m < 1 || a->m > mr || a->m < a->n - a->p || a->lda < a->m || a->ldc < a->p || a->ldb < a->m || a->ldd < a->p || a->ldx < a->n ||
        (a->L && a->ldl < a->p) || !a->A || !a->C || !a->B || !a->D || !a->X || !a->info)
        return -7;
    const int rc = bl_allow_lds();
    if (rc) return rc;
    hipStream_t s = (hipStream_t) stream;
    const int ntot = a->n + a->nrhs;
    if (qrd_bl_wave_route(a->m, a->n, a->nrhs)) {
        if (ntot <= 8) bl_launch_wave<8>(s, *a);
        else if (ntot <= 16) bl_launch_wave<16>(s, *a);
        else bl_launch_wave<32>(s, *a);
    } else {
        hipLaunchKernelGGL(bl_wg_kernel, dim3((unsigned) a->batch), dim3(256), sizeof(double) * bl_wg_doubles(a->m, a->n, a->p, a->nrhs), s, *a);
    }
    return (int) hipGetLastError();
}

}   // extern "C"
