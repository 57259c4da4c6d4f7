// qr_batched_stats.hip -- kernels of the batched covariance, standard errors and leverages (qr_batched_stats.c, mi355x_qr.h section 8k):
// what MINPACK's covar computes from a triangle, the quadratic form a^T (R^T R)^-1 a for arbitrary rows, and the weighted least-squares
// fit of section 8j (QR_LOSS_LS) with all of its statistics in one launch.
//
// The arithmetic lives in the device functions below and is fixed per ENTRY, whichever kernel calls it (R11 the leading r x r block):
//
//   T = R11^-1     along the rows, T R = I:  s = (i == j ? 1 : 0);  s = fma(-T(i,k), R(k,j), s) for k = 0 .. j-1 ascending (T(i,k) = 0 for
//                  k < i: those terms change nothing);  T(i,j) = s / R(j,j) for j >= i                    st_inv_row / st_inv_lds
//   S = T T^T      S(i,j) = sum over k = j .. r-1 ascending of fma(T(i,k), T(j,k), .) from 0, for i <= j   st_cov_entry / st_cov_out_wg
//   C              mult * S(i,j), one rounded product, stored at (jpvt[i], jpvt[j]) and (jpvt[j], jpvt[i]) from the one value; exact
//                  zeros where i >= r or j >= r;  se(jpvt[i]) = sqrt of the stored C
//   h              y = R11^-T a by forward substitution: s = a_k; s = fma(-R(l,k), y_l, s) for l = 0 .. k-1 ascending; y_k = s / R(k,k);
//                  ss = fma(y_k, y_k, ss) for k ascending;  h = p * ss, exactly 0 where p == 0              st_lev_row
//
// R^T R is never formed.  Every operation above is an explicit fma, a division, a square root or one product under contract(off): the
// compiler has nothing to fuse differently from one kernel to the next, which is what makes the results of the fused kernels bitwise
// those of the from-factor kernels on the same triangle.
//
//   bs_cov_wave_kernel<W>   n <= W <= 32: one wave per member, four per workgroup.  Lane i holds row i of T in W registers (every index
//                           a constant once the loops are unrolled); R, then T, in the wave's LDS slice, read wave-uniformly
//   bs_cov_wg_kernel        n <= 64: one workgroup per member; wave 0 inverts R in place in LDS, 256 threads form S
//   bs_lev_kernel<W>        r <= n <= W <= 64, W in steps of 8: one workgroup per (member, chunk of 256 rows), R in LDS, one row of A per
//                           thread in W registers
//   bs_fit_wave_kernel<W>   m <= 64 and n + 1 <= W <= 32: the fit of ir_wave_kernel (qr_batched_irls.hip) at loss 0, then e, sigma2, h, T, C
//   bs_fit_wg_kernel<W>     the rest (n <= W <= 64, W in steps of 8): the image in LDS; R is inverted in place in the top of the image once x, e and h are out
//
// Failure is all or nothing: every info word is decided before the member's first store.  Every sum runs in an order that the shape
// fixes; no atomics.
#include "qr_batched_dev.h"

#define ST_INF __builtin_huge_val()
#define ST_ROWS 256                           // rows of A per workgroup of bs_lev_kernel: one per thread

// a prior weight or a multiplier that is negative, NaN or inf
__device__ __forceinline__ bool st_bad_weight(double p) { return !(p >= 0.0 && p < ST_INF); }

// one wave, jp of lane < n <= 64: whether jp(0 .. n-1) is no permutation of 0 .. n-1 (the same answer in every lane)
__device__ __forceinline__ bool st_bad_perm(int jp, int n, int lane)
{
    bool bad = lane < n && (jp < 0 || jp >= n);
    for (int l = 0; l < n; ++l) {
        const int v = __builtin_amdgcn_readlane(jp, l);
        bad = bad || (lane < n && l < lane && v == jp);
    }
    return __ballot(bad) != 0;
}

// Row `lane` of T = R11^-1 into u (zeros left of the diagonal, past r and in lanes >= r); R(k, j) = R[j * ldr + k], read wave-uniformly
template <int W>
__device__ __forceinline__ void st_inv_row(const double* R, int ldr, int r, int lane, double (&u)[W])
{
#pragma unroll
    for (int j = 0; j < W; ++j) {
        double v = 0.0;
        if (j < r) {                          // (wave-uniform)
            double s = lane == j ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < j; ++k) s = fma(-u[k], R[j * ldr + k], s);
            v = lane <= j ? s / R[j * ldr + j] : 0.0;
        }
        u[j] = v;
    }
}

// The same rows by the lanes of ONE wave (lane = row, r <= 64), in place over the upper triangle of an LDS image: column j of R is read
// by every lane before column j of T is written over it; what lies below the diagonal is neither read nor written
__device__ __forceinline__ void st_inv_lds(double* R, int ldr, int r, int lane)
{
    for (int j = 0; j < r; ++j) {
        double s = lane == j ? 1.0 : 0.0;
        for (int k = 0; k < j; ++k) {
            const double tik = k >= lane ? R[k * ldr + lane] : 0.0;
            s = fma(-tik, R[j * ldr + k], s);
        }
        const double v = s / R[j * ldr + j];
        QB_WAVE_SYNC();
        if (lane <= j) R[j * ldr + lane] = v;
        QB_WAVE_SYNC();
    }
}

// S(lane, j) from the lane's row u and T(j, k) = T[k * ldt + j] (wave-uniform reads); meaningful in lanes <= j
template <int W>
__device__ __forceinline__ double st_cov_entry(const double (&u)[W], const double* T, int ldt, int j, int r)
{
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < W; ++k)
        if (k >= j && k < r) s = fma(u[k], T[k * ldt + j], s);          // (wave-uniform)
    return s;
}

// One wave: C and se of a member from the rows u of T (lane i: row i) and T in LDS.  jp: the lane's target index (checked: a permutation)
template <int W>
__device__ __forceinline__ void st_cov_out_wave(const double (&u)[W], const double* T, int ldt, int n, int r, int lane, int jp, double mult,
                                                double* Cq, int ldc, double* seq)
{
#pragma clang fp contract(off)
    for (int j = 0; j < n; ++j) {
        const double s = st_cov_entry<W>(u, T, ldt, j, r);
        const double c = (lane < r && j < r) ? mult * s : 0.0;
        const int pj = __builtin_amdgcn_readlane(jp, j);
        if (lane < n && j >= lane) {
            if (Cq) {
                Cq[(size_t) pj * ldc + jp] = c;
                Cq[(size_t) jp * ldc + pj] = c;
            }
            if (seq && j == lane) seq[jp] = sqrt(c);
        }
    }
}

// All 256 threads: the same from T in the upper triangle of an LDS image.  jps: the target indices in LDS, or nullptr for the identity
__device__ __forceinline__ void st_cov_out_wg(const double* T, int ldt, int n, int r, const int* jps, double mult, double* Cq, int ldc, double* seq,
                                              int t)
{
#pragma clang fp contract(off)
    for (int idx = t; idx < n * n; idx += 256) {
        const int j = idx / n, i = idx - j * n;
        if (i > j) continue;
        double s = 0.0;
        if (j < r)
            for (int k = j; k < r; ++k) s = fma(T[k * ldt + i], T[k * ldt + j], s);
        const double c = j < r ? mult * s : 0.0;
        const int pi = jps ? jps[i] : i, pj = jps ? jps[j] : j;
        if (Cq) {
            Cq[(size_t) pj * ldc + pi] = c;
            Cq[(size_t) pi * ldc + pj] = c;
        }
        if (seq && i == j) seq[pi] = sqrt(c);
    }
}

// |R11^-T y(0 : r)|^2 for the row in y (overwritten); R(l, k) = R[k * ldr + l], read uniformly by the threads that share R
template <int W>
__device__ __forceinline__ double st_lev_row(const double* R, int ldr, int r, double (&y)[W])
{
    double ss = 0.0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        if (k < r) {                          // (uniform)
            double s = y[k];
#pragma unroll
            for (int l = 0; l < k; ++l) s = fma(-R[k * ldr + l], y[l], s);
            y[k] = s / R[k * ldr + k];
            ss = fma(y[k], y[k], ss);
        }
    }
    return ss;
}

// h of a row from its sum: one rounded product; exactly 0 where the row is excluded
__device__ __forceinline__ double st_lev_scale(double p, double ss)
{
#pragma clang fp contract(off)
    return p > 0.0 ? p * ss : 0.0;
}

// p e^2 of one row, two rounded products
__device__ __forceinline__ double st_wsq(double p, double e)
{
#pragma clang fp contract(off)
    const double w = p * e;
    return w * e;
}

// v again, as a value the compiler knows nothing about: the comparisons of a later phase with it are formed there, not carried in scalar
// registers from the first phase that compared with v to the last (one kernel then needs a stack slot for them)
__device__ __forceinline__ int st_opaque(int v)
{
    asm volatile("" : "+s"(v));
    return v;
}

// the accumulator's multiplier: sigma2 = rss / (rows - n), +inf without a degree of freedom
__device__ __forceinline__ double st_sigma2(double rss, int dof) { return dof > 0 ? rss / (double) dof : ST_INF; }

// ---------------------------------------------------------------------------------------------------------------------------------
// covariance from a triangle.  The checks of one member, by one wave (lane j < n: jpvt[j]); returns the info word (0: go on) and
// leaves r, mult and the sigma2 of the accumulator mode.  The diagonal is read from global memory: nothing is in LDS yet.
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int st_cov_checks(const qrd_bs_args& g, size_t q, int lane, int& r, int& jp, double& mult, double& sig)
{
    const int n = g.n;
    r = g.rank ? g.rank[q] : n;
    jp = lane;
    if (g.jpvt && lane < n) jp = g.jpvt[q * g.sj + lane];
    mult = (!g.acc && g.mult) ? g.mult[q] : 1.0;
    sig = 0.0;
    if (r < 0 || r > n || st_bad_perm(jp, n, lane) || st_bad_weight(mult)) return -1;
    const double* Rq = g.R + q * g.sR;
    const double d = lane < r ? Rq[(size_t) lane * g.ldr + lane] : 1.0;
    const int sing = qb_info_wave(d, r, lane);
    if (sing) return sing;
    if (g.acc) {
        const int dof = g.rows[q] - n;
        if (g.scaled && dof == 0) return -3;
        sig = st_sigma2(g.rss[q * (size_t) g.nrhs + g.rhs], dof);
        if (g.scaled) mult = sig;
        if (st_bad_weight(mult)) return -1;
    }
    return 0;
}

template <int W>
__global__ void __launch_bounds__(256) bs_cov_wave_kernel(const qrd_bs_args g)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) g.batch) return;        // (no workgroup barrier below: the waves of a workgroup are independent)
    constexpr int LW = W + 1;
    const int n = g.n;
    double* Vs = sm + (size_t) wv * (W * LW);
    int r, jp;
    double mult, sig;
    const int inf = st_cov_checks(g, q, lane, r, jp, mult, sig);
    if (inf) {                                // (all or nothing: nothing else is written)
        if (lane == 0) g.info[q] = inf;
        return;
    }
    const double* Rq = g.R + q * g.sR;
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (c < r && lane <= c) Vs[c * LW + lane] = Rq[(size_t) c * g.ldr + lane];          // (the strict lower triangle is not read)
    QB_WAVE_SYNC();
    double u[W];
    st_inv_row<W>(Vs, LW, r, lane, u);
    QB_WAVE_SYNC();                           // (R is read no more)
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (c < r && lane <= c) Vs[c * LW + lane] = u[c];
    QB_WAVE_SYNC();
    st_cov_out_wave<W>(u, Vs, LW, n, r, lane, jp, mult, g.C ? g.C + q * g.sC : nullptr, g.ldc, g.se ? g.se + q * g.sse : nullptr);
    if (lane == 0) {
        if (g.sigma2) g.sigma2[q] = sig;
        g.info[q] = 0;
    }
}

// LDS: Rs (n x n at ld = bd_ld(n)), then mult (one double), then jps[64] and one word (ints)
__host__ __device__ constexpr size_t st_cov_wg_lds(int n) { return sizeof(double) * ((size_t) n * bd_ld(n) + 1) + sizeof(int) * (64 + 2); }

__global__ void __launch_bounds__(256) bs_cov_wg_kernel(const qrd_bs_args g)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const int n = g.n, ld = bd_ld(n);
    double* Rs = sm;
    double* smult = Rs + (size_t) n * ld;
    int* jps = (int*) (smult + 1);
    int* words = jps + 64;                    // the info word, the rank
    if (wv == 0) {
        int r, jp;
        double mult, sig;
        const int inf = st_cov_checks(g, q, lane, r, jp, mult, sig);
        jps[lane] = jp;
        if (lane == 0) {
            words[0] = inf;
            words[1] = r;
            *smult = mult;
            if (inf) g.info[q] = inf;         // (all or nothing: nothing else is written)
            else if (g.sigma2) g.sigma2[q] = sig;
        }
    }
    __syncthreads();
    if (words[0]) return;
    const int r = words[1];
    const double* Rq = g.R + q * g.sR;
    for (int idx = t; idx < r * r; idx += 256) {
        const int c = idx / r, i = idx - c * r;
        if (i <= c) Rs[c * ld + i] = Rq[(size_t) c * g.ldr + i];
    }
    __syncthreads();
    if (wv == 0) st_inv_lds(Rs, ld, r, lane);
    __syncthreads();
    st_cov_out_wg(Rs, ld, n, r, jps, *smult, g.C ? g.C + q * g.sC : nullptr, g.ldc, g.se ? g.se + q * g.sse : nullptr, t);
    if (t == 0) g.info[q] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// leverages of arbitrary rows.  Workgroup (q, chunk): rows chunk * 256 .. of member q, one per thread.  LDS: Rs (n x n at ld = n), then
// jps[64] and two words.  Every workgroup of a member runs the member's checks -- the prior weights of ALL its rows among them -- and
// reaches the same verdict, so a failed member has nothing written by any of them; chunk 0 writes the info word.
// ---------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr size_t st_lev_lds(int n) { return sizeof(double) * (size_t) n * n + sizeof(int) * (64 + 2); }

template <int W>
__global__ void __launch_bounds__(256) bs_lev_kernel(const qrd_bs_lev_args g)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x / (unsigned) g.nchunk;
    const int chunk = (int) (blockIdx.x - q * (unsigned) g.nchunk);
    const int n = g.n, mrows = g.mrows;
    double* Rs = sm;
    int* jps = (int*) (Rs + (size_t) n * n);
    int* words = jps + 64;                    // the info word, the rank
    const double* Rq = g.R + q * g.sR;
    const double* Pq = g.prior ? g.prior + q * g.sprior : nullptr;
    if (t == 0) words[0] = 0;
    __syncthreads();
    if (wv == 0) {
        const int r = g.rank ? g.rank[q] : n;
        int jp = lane;
        if (g.jpvt && lane < n) jp = g.jpvt[q * g.sj + lane];
        const bool bad = r < 0 || r > n || st_bad_perm(jp, n, lane);
        jps[lane] = jp;
        if (lane == 0) {
            words[1] = bad ? 0 : r;
            if (bad) words[0] = -1;
        }
    }
    if (Pq)
        for (int i = t; i < mrows; i += 256)
            if (st_bad_weight(Pq[i])) words[0] = -1;                 // (every writer writes the same value)
    __syncthreads();
    const int r = words[1];
    if (words[0] == 0) {
        for (int idx = t; idx < r * r; idx += 256) {
            const int c = idx / r, i = idx - c * r;
            if (i <= c) Rs[c * n + i] = Rq[(size_t) c * g.ldr + i];
        }
    }
    __syncthreads();
    if (t == 0 && words[0] == 0) words[0] = qb_info_serial(Rs, n, r);
    __syncthreads();
    if (words[0]) {                           // (all or nothing: nothing else is written)
        if (t == 0 && chunk == 0) g.info[q] = words[0];
        return;
    }
    const int i = chunk * ST_ROWS + t;
    if (i < mrows) {
        const double p = Pq ? Pq[i] : 1.0;
        const double* Aq = g.A + q * g.sA;
        double y[W];
#pragma unroll
        for (int c = 0; c < W; ++c) {
            double v = 0.0;
            if (c < r && p > 0.0) v = Aq[(size_t) jps[c] * g.lda + i];       // (an excluded row is not used, whatever it holds)
            y[c] = v;
        }
        const double ss = st_lev_row<W>(Rs, n, r, y);
        g.H[q * g.sH + i] = st_lev_scale(p, ss);
    }
    if (t == 0 && chunk == 0) g.info[q] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the fit and its statistics.  Wave route: ir_wave_kernel's one solve at loss 0 (the same image, the same column steps, the same back
// substitution: x is bitwise qrd_ir_solve's), then the statistics from the untouched inputs and the triangle in the wave's LDS slice.
// Dynamic LDS per wave: Vs[c * LW + r] = R(r, c) (LW = W + 1), then zs[W]: (Q^T b)(0 : n), then x.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(256) bs_fit_wave_kernel(const qrd_bs_fit_args g)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) g.batch) return;        // (no workgroup barrier below: the waves of a workgroup are independent)
    const int m = g.m, n = g.n;
    constexpr int LW = W + 1;
    double* Vs = sm + (size_t) wv * (W * LW + W);
    double* zs = Vs + W * LW;
    const double* Aq = g.A + q * g.sA;
    const double* Bq = g.B + q * g.sB;
    const bool row = lane < m, var = lane < n;
    const double p = !row ? 0.0 : (g.prior ? g.prior[q * g.sprior + lane] : 1.0);
    const bool incl = p > 0.0;                // (false in lanes >= m)
    const int cnt = __popcll(__ballot(incl)), dof = cnt - n;
    int inf = 0;
    if (__ballot(st_bad_weight(p))) inf = -1;
    else if (cnt < n) inf = -2;
    else if (g.scaled && dof == 0) inf = -3;
    if (inf) {                                // (all or nothing: nothing else is written)
        if (lane == 0) g.info[q] = inf;
        return;
    }
    // row i of the untouched [A | b] times sqrt(p_i); an excluded row is zeros whatever it holds
    double a[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
        double v = 0.0;
        if (incl && c < n) v = Aq[(size_t) c * g.lda + lane];
        a[c] = v;
    }
    double bi = 0.0;
    if (incl) bi = Bq[lane];
    const double sq = incl ? sqrt(p) : 0.0;
    const int nf = st_opaque(n);
#pragma unroll
    for (int c = 0; c < W; ++c) a[c] = c == nf ? bi * sq : a[c] * sq;            // (columns past n hold zeros; n < W)
    double tauv = 0.0, diag = 1.0;            // lane j: R(j, j)
#pragma unroll
    for (int j = 0; j < W; ++j) {
        if (j < nf) qb_wave_col<W>(a, j, nf + 1, lane, tauv, diag);              // (wave-uniform; b rides along)
    }
    const int sing = qb_info_wave(diag, n, lane);
    if (sing) {                               // (all or nothing: nothing else is written)
        if (lane == 0) g.info[q] = sing;
        return;
    }
    const int ns = st_opaque(n);
#pragma unroll
    for (int c = 0; c < W; ++c) {
        if (c < ns) {
            if (lane < n) Vs[c * LW + lane] = a[c];
        } else if (c == ns) {
            if (lane < n) zs[lane] = a[c];
        }
    }
    QB_WAVE_SYNC();
    if (lane == 0) qb_trsv(Vs, LW, n, zs);
    QB_WAVE_SYNC();
    const double x = var ? zs[lane] : 0.0;
    if (var) g.X[q * g.sX + lane] = x;
    // the untouched row again: e, p e^2, then h (which overwrites the row)
    const int ne = st_opaque(n);
#pragma unroll
    for (int c = 0; c < W; ++c) {
        double v = 0.0;
        if (incl && c < ne) v = Aq[(size_t) c * g.lda + lane];
        a[c] = v;
    }
    double e = bi;
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (c < ne) e = fma(-a[c], zs[c], e);      // (x from LDS: 2 W readlanes held in scalar registers spill)
    e = incl ? e : 0.0;
    const double sig = st_sigma2(qb_wave_sum(st_wsq(p, e)), dof);
    if (row && g.E) g.E[q * g.sE + lane] = e;
    if (g.H) {                                // (wave-uniform)
        const double ss = st_lev_row<W>(Vs, LW, st_opaque(n), a);
        if (row) g.H[q * g.sH + lane] = st_lev_scale(p, ss);
    }
    if (g.C || g.se) {                        // (wave-uniform)
        const int nc = st_opaque(n);
        QB_WAVE_SYNC();
        st_inv_row<W>(Vs, LW, nc, lane, a);
        QB_WAVE_SYNC();                       // (R is read no more)
#pragma unroll
        for (int c = 0; c < W; ++c)
            if (c < nc && lane <= c) Vs[c * LW + lane] = a[c];
        QB_WAVE_SYNC();
        st_cov_out_wave<W>(a, Vs, LW, nc, nc, lane, lane, g.scaled ? sig : 1.0, g.C ? g.C + q * g.sC : nullptr, g.ldc,
                           g.se ? g.se + q * g.sse : nullptr);
    }
    if (lane == 0) {
        if (g.sigma2) g.sigma2[q] = sig;
        if (g.dof) g.dof[q] = dof;
        g.info[q] = 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// workgroup route.  LDS: As[c * ld + i] = the image (n + 1 columns, ld = qb_ld(m)), xs (n), then QB_WG_SMALL doubles: red[4], sigma2, and
// the words (info, the count of included rows).  Thread 0 takes every decision and publishes it in an LDS word that all threads read
// after a barrier.  The triangle is inverted where it stands, in the top of the image, once x, e and h no longer need R.
// ---------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr size_t st_fit_wg_doubles(int m, int n) { return (size_t) (n + 1) * qb_ld(m) + (size_t) n + QB_WG_SMALL; }
static_assert(sizeof(double) * st_fit_wg_doubles(512, 31) <= QB_LDS_CAP && sizeof(double) * st_fit_wg_doubles(256, 63) <= QB_LDS_CAP,
              "512 x 31 and 256 x 63 are taken");

template <int W>
__global__ void __launch_bounds__(256) bs_fit_wg_kernel(const qrd_bs_fit_args g)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const int m = g.m, n = g.n;
    const int ld = qb_ld(m);
    double* As = sm;
    double* xs = As + (size_t) (n + 1) * ld;
    double* red = xs + n;
    double* ssig = red + 4;
    int* words = (int*) (red + 5);
    int *sinfo = words, *scnt = words + 1;
    const double* Aq = g.A + q * g.sA;
    const double* Bq = g.B + q * g.sB;
    const double* Pq = g.prior ? g.prior + q * g.sprior : nullptr;
    if (t == 0) *sinfo = 0;
    __syncthreads();
    // the checks and the count of included rows
    double pc = 0.0;
    for (int i = t; i < m; i += 256) {
        const double p = Pq ? Pq[i] : 1.0;
        if (st_bad_weight(p)) *sinfo = -1;    // (every writer writes the same value)
        pc += p > 0.0 ? 1.0 : 0.0;
    }
    pc = qb_wave_sum(pc);
    if (lane == 0) red[wv] = pc;
    __syncthreads();
    if (t == 0 && *sinfo == 0) {
        const int cnt = (int) (((red[0] + red[1]) + red[2]) + red[3]);
        *scnt = cnt;
        if (cnt < n) *sinfo = -2;
        else if (g.scaled && cnt == n) *sinfo = -3;
    }
    __syncthreads();
    if (*sinfo) {                             // (all or nothing: nothing else is written)
        if (t == 0) g.info[q] = *sinfo;
        return;
    }
    // the image: row i of [A | b] times sqrt(p_i), coalesced along the rows; an excluded row is zeros whatever it holds
    for (int c = wv; c <= n; c += 4) {
        const double* src = c < n ? Aq + (size_t) c * g.lda : Bq;
        for (int i = lane; i < m; i += 64) {
            const double p = Pq ? Pq[i] : 1.0;
            double v = 0.0;
            if (p > 0.0) v = src[i] * sqrt(p);
            As[c * ld + i] = v;
        }
    }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        qb_wg_col(As, ld, m, j, n + 1, red, t);
        __syncthreads();                      // (red and column j are read no more)
    }
    if (t == 0) {
        const int sing = qb_info_serial(As, ld, n);
        if (sing) *sinfo = sing;
        else {
            double* zc = As + (size_t) n * ld;
            qb_trsv(As, ld, n, zc);
            for (int j = 0; j < n; ++j) xs[j] = zc[j];
        }
    }
    __syncthreads();
    if (*sinfo) {                             // (all or nothing: nothing else is written)
        if (t == 0) g.info[q] = *sinfo;
        return;
    }
    const int dof = *scnt - n;
    for (int j = t; j < n; j += 256) g.X[q * g.sX + j] = xs[j];
    // e, p e^2 and h of row i from the untouched inputs, one row per thread and pass (not run where x alone is wanted)
    const bool rows = g.E || g.H || g.sigma2 || (g.scaled && (g.C || g.se));
    double ss = 0.0;
    for (int i = t; rows && i < m; i += 256) {
        const double p = Pq ? Pq[i] : 1.0;
        const bool incl = p > 0.0;
        double a[W];
#pragma unroll
        for (int c = 0; c < W; ++c) {
            double v = 0.0;
            if (incl && c < n) v = Aq[(size_t) c * g.lda + i];
            a[c] = v;
        }
        double e = 0.0;
        if (incl) e = Bq[i];
#pragma unroll
        for (int c = 0; c < W; ++c)
            if (c < n) e = fma(-a[c], xs[c], e);
        e = incl ? e : 0.0;
        ss += st_wsq(p, e);
        if (g.E) g.E[q * g.sE + i] = e;
        if (g.H) g.H[q * g.sH + i] = st_lev_scale(p, st_lev_row<W>(As, ld, n, a));
    }
    ss = qb_wave_sum(ss);
    if (lane == 0) red[wv] = ss;
    __syncthreads();                          // (R is read no more)
    if (t == 0) {
        const double sig = st_sigma2(((red[0] + red[1]) + red[2]) + red[3], dof);
        *ssig = sig;
        if (g.sigma2) g.sigma2[q] = sig;
        if (g.dof) g.dof[q] = dof;
    }
    if (g.C || g.se) {                        // (the same in every thread)
        if (wv == 0) st_inv_lds(As, ld, n, lane);
        __syncthreads();
        st_cov_out_wg(As, ld, n, n, nullptr, g.scaled ? *ssig : 1.0, g.C ? g.C + q * g.sC : nullptr, g.ldc, g.se ? g.se + q * g.sse : nullptr, t);
    }
    if (t == 0) g.info[q] = 0;
}

// the kernels that may ask for more than 64 KiB of LDS (qr_allow_lds)
static int st_allow_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(bs_fit_wg_kernel<8>),  reinterpret_cast<const void*>(bs_fit_wg_kernel<16>),
                               reinterpret_cast<const void*>(bs_fit_wg_kernel<24>), reinterpret_cast<const void*>(bs_fit_wg_kernel<32>),
                               reinterpret_cast<const void*>(bs_fit_wg_kernel<40>), reinterpret_cast<const void*>(bs_fit_wg_kernel<48>),
                               reinterpret_cast<const void*>(bs_fit_wg_kernel<56>), reinterpret_cast<const void*>(bs_fit_wg_kernel<64>)};
    return qr_allow_lds(fns, QB_LDS_CAP, done);
}

template <int W>
static void st_launch_cov_wave(hipStream_t s, const qrd_bs_args& a)
{
    hipLaunchKernelGGL(bs_cov_wave_kernel<W>, dim3((unsigned) (((size_t) a.batch + 3) / 4)), dim3(256), sizeof(double) * 4 * (W * (W + 1)), s, a);
}

template <int W>
static void st_launch_lev(hipStream_t s, const qrd_bs_lev_args& a)
{
    hipLaunchKernelGGL(bs_lev_kernel<W>, dim3((unsigned) ((size_t) a.batch * a.nchunk)), dim3(256), st_lev_lds(a.n), s, a);
}

template <int W>
static void st_launch_fit_wave(hipStream_t s, const qrd_bs_fit_args& a)
{
    hipLaunchKernelGGL(bs_fit_wave_kernel<W>, dim3((unsigned) (((size_t) a.batch + 3) / 4)), dim3(256), sizeof(double) * 4 * (W * (W + 1) + W), s, a);
}

template <int W>
static void st_launch_fit_wg(hipStream_t s, const qrd_bs_fit_args& a)
{
    hipLaunchKernelGGL(bs_fit_wg_kernel<W>, dim3((unsigned) a.batch), dim3(256), sizeof(double) * st_fit_wg_doubles(a.m, a.n), s, a);
}

extern "C" {

int qrd_bs_cov_wave_route(int n) { return n >= 1 && n <= 32; }
int qrd_bs_fit_wave_route(int m, int n) { return m <= 64 && n + 1 <= 32; }

// the largest m the fit takes for n unknowns; 0: n is not taken at all.  The wave route needs no more than the workgroup route holds, so
// the workgroup route's LDS budget decides.
int qrd_bs_max_rows(int n)
{
    if (n < 1 || n > QRD_B_MAX_N - 1) return 0;
    int m = QRD_B_MAX_ROWS;
    while (m >= n && sizeof(double) * st_fit_wg_doubles(m, n) > QB_LDS_CAP) --m;
    return m >= n ? m : 0;
}

int qrd_bs_covar(void* stream, const qrd_bs_args* a)
{
    if (!a) return -7;
    if (a->batch <= 0) return 0;
    if (a->n < 1 || a->n > QRD_B_MAX_N || a->ldr < a->n || !a->R || !a->info || (!a->C && !a->se) || (a->C && a->ldc < a->n) ||
        (a->acc && (!a->rss || !a->rows || a->rhs < 0 || a->rhs >= a->nrhs)))
        return -7;
    hipStream_t s = (hipStream_t) stream;
    if (qrd_bs_cov_wave_route(a->n)) {
        if (a->n <= 8) st_launch_cov_wave<8>(s, *a);
        else if (a->n <= 16) st_launch_cov_wave<16>(s, *a);
        else st_launch_cov_wave<32>(s, *a);
    } else {
        hipLaunchKernelGGL(bs_cov_wg_kernel, dim3((unsigned) a->batch), dim3(256), st_cov_wg_lds(a->n), s, *a);
    }
    return (int) hipGetLastError();
}

int qrd_bs_lev_chunks(int mrows) { return mrows < 1 ? 0 : (mrows - 1) / ST_ROWS + 1; }

int qrd_bs_leverage(void* stream, const qrd_bs_lev_args* a)
{
    if (!a) return -7;
    if (a->batch <= 0) return 0;
    if (a->n < 1 || a->n > QRD_B_MAX_N || a->ldr < a->n || a->mrows < 1 || a->lda < a->mrows || a->nchunk != qrd_bs_lev_chunks(a->mrows) ||
        (size_t) a->batch * (size_t) a->nchunk > 0x7fffffffu || !a->R || !a->A || !a->H || !a->info)
        return -7;
    hipStream_t s = (hipStream_t) stream;
    switch ((a->n + 7) / 8) {                 // the row of A in W registers: W in steps of 8 keeps the occupancy of a mid-sized n
    case 1: st_launch_lev<8>(s, *a); break;
    case 2: st_launch_lev<16>(s, *a); break;
    case 3: st_launch_lev<24>(s, *a); break;
    case 4: st_launch_lev<32>(s, *a); break;
    case 5: st_launch_lev<40>(s, *a); break;
    case 6: st_launch_lev<48>(s, *a); break;
    case 7: st_launch_lev<56>(s, *a); break;
    default: st_launch_lev<64>(s, *a); break;
    }
    return (int) hipGetLastError();
}

int qrd_bs_fit(void* stream, const qrd_bs_fit_args* a)
{
    if (!a) return -7;
    if (a->batch <= 0) return 0;
    const int mr = qrd_bs_max_rows(a->n);
    if (!mr || a->m < a->n || a->m > mr || a->lda < a->m || !a->A || !a->B || !a->X || !a->info || (a->C && a->ldc < a->n)) return -7;
    hipStream_t s = (hipStream_t) stream;
    if (qrd_bs_fit_wave_route(a->m, a->n)) {
        if (a->n + 1 <= 8) st_launch_fit_wave<8>(s, *a);
        else if (a->n + 1 <= 16) st_launch_fit_wave<16>(s, *a);
        else st_launch_fit_wave<32>(s, *a);
    } else {
        const int rc = st_allow_lds();
        if (rc) return rc;
        switch ((a->n + 7) / 8) {             // (as in qrd_bs_leverage)
        case 1: st_launch_fit_wg<8>(s, *a); break;
        case 2: st_launch_fit_wg<16>(s, *a); break;
        case 3: st_launch_fit_wg<24>(s, *a); break;
        case 4: st_launch_fit_wg<32>(s, *a); break;
        case 5: st_launch_fit_wg<40>(s, *a); break;
        case 6: st_launch_fit_wg<48>(s, *a); break;
        case 7: st_launch_fit_wg<56>(s, *a); break;
        default: st_launch_fit_wg<64>(s, *a); break;
        }
    }
    return (int) hipGetLastError();
}

}   // extern "C"
