// qr_batched_irls.hip -- kernels of the batched robust and weighted least squares (qr_batched_irls.c, mi355x_qr.h section 8j): per member of
// a batch min sum_i p_i rho((b - A x)_i / s) (A: m x n, m >= n, one b, prior weights p_i >= 0) by iteratively reweighted least squares, the
// reweighting loop of every member inside one launch:
//
//   1. checks     a p_i that is negative, NaN or inf, a given scale that is no finite positive number: info -1.  Rows with p_i == 0 are
//                 excluded: loaded as exact zeros by a select (a NaN there is harmless)
//   2. start      w = 1, it = 0.  X0 given (and a robust loss): x = X0, step 4 comes first.  Otherwise step 3
//   3. solve      c_i = p_i w_i; fewer than n rows with c_i > 0: info -2.  it == maxit: status 3, done.  Else ++it, the image is row i of
//                 [A | b] from the untouched inputs times sqrt(c_i), Householder QR with b riding along, R x = (Q^T b)(0 : n); an exactly
//                 zero R(i,i): info i + 1
//   4. residual   r_i = b_i - sum_j A(i,j) x_j (j ascending, one fma per term).  Loss 0: status 0, done.  s = the given scale, else
//                 median{|r_i| : p_i > 0} / 0.6744897501960817 (by ranks, ties broken by the row index; an even count: half the sum of the
//                 two middle values).  s == 0: status 2, w = 1, done.  u_i = |r_i| / s; Huber: w_i = 1 if u_i <= k else k / u_i;
//                 bisquare: w_i = (1 - (u_i / c)^2)^2 if u_i < c else 0
//   5. stopping   once a solve has run and a previous x exists (X0 on a warm start): max_j |x_j - xold_j| <= tol max_j |x_j|: status 0,
//                 done.  Else xold = x, go to 3
//
// Every solve is factored from scratch through the shared column steps (qr_batched_dev.h), called unchanged with the end of the update at
// n + 1: with loss 0 and no prior weights the image is [A | b] itself and x is bitwise qrd_b_geqrf's on the same route.
//
//   ir_wave_kernel<W>  m <= 64 and n + 1 <= W <= 32: one wave per member, four per workgroup, no workgroup barrier.  Lane i holds row i:
//                      its prior weight, residual, robust weight and the row of the image in W registers, refilled from global A per pass
//                      (the same load serves the residual of the last x and the next image); lane j < n also holds x_j and xold_j.  R and
//                      the top of Q^T b go through the wave's LDS for qb_trsv.  The median is m readlane compares per lane and two
//                      ballots.  Every decision is taken on a ballot or a butterfly: wave-uniform by construction
//   ir_wg_kernel       everything else that fits: one workgroup per member, the image in LDS at qb_ld(m), r, w, |r| / sqrt(c) (m each), x
//                      and xold (n each) behind it.  Thread 0 takes every decision and publishes it in an LDS word that all threads read
//                      after a barrier: every thread reaches every barrier the same number of times
//
// `it` counts solves and it <= maxit is the only loop bound.  A comparison with a NaN is false: a NaN in an included row makes every
// weight a NaN, no c_i > 0, and the member leaves at the next count with info -2.  Every sum runs in an order that (m, n) fixes; no atomics.
#include "qr_batched_dev.h"

#define IR_INF __builtin_huge_val()
#define IR_NAN __builtin_nan("")
#define IR_MAD 0.6744897501960817           // the 0.75 quantile of the standard normal

// a prior weight that is negative, NaN or inf; a given scale that is no finite positive number
__device__ __forceinline__ bool ir_bad_prior(double p) { return !(p >= 0.0 && p < IR_INF); }
__device__ __forceinline__ bool ir_bad_scale(double s) { return !(s > 0.0 && s < IR_INF); }

// the robust weight of u = |r| / s; every rounding written out (contraction would fuse 1 - t t)
__device__ __forceinline__ double ir_weight(int loss, double u, double k)
{
#pragma clang fp contract(off)
    if (loss == 1) return u <= k ? 1.0 : k / u;
    const double t = u / k;
    const double h = 1.0 - t * t;
    return u < k ? h * h : 0.0;
}

// the same maximum in every lane (NaN operands are dropped by fmax: the caller's test does not rest on it for them)
__device__ __forceinline__ double ir_wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// the median of v over the lanes of the ballot im (cnt of them), the same value in every lane: rank_i = #{j : v_j < v_i, or v_j == v_i and
// j < i}; half the sum of the values of ranks (cnt - 1) / 2 and cnt / 2.  A NaN among them, or none at all: NaN
__device__ __forceinline__ double ir_wave_median(double v, bool incl, unsigned long long im, int cnt, int m, int lane)
{
    if (cnt == 0 || __ballot(incl && v != v)) return IR_NAN;
    int rank = 0;
    for (int j = 0; j < m; ++j) {
        if (!((im >> j) & 1ull)) continue;    // (wave-uniform)
        const double vj = qb_bcast(v, j);
        rank += (vj < v || (vj == v && j < lane)) ? 1 : 0;
    }
    const unsigned long long b1 = __ballot(incl && rank == ((cnt - 1) >> 1)), b2 = __ballot(incl && rank == (cnt >> 1));
    if (!b1 || !b2) return IR_NAN;            // (the ranks of cnt ordered values are a permutation: not reached)
    return 0.5 * (qb_bcast(v, __ffsll((long long) b1) - 1) + qb_bcast(v, __ffsll((long long) b2) - 1));
}

// ---------------------------------------------------------------------------------------------------------------------------------
// wave route.  Dynamic LDS per wave: Vs[c * LW + r] = R(r, c) (LW = W + 1), then zs[W]: (Q^T b)(0 : n), then x.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(256) ir_wave_kernel(const qrd_ir_args g)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) g.batch) return;        // (no workgroup barrier below: the waves of a workgroup are independent)
    const int m = g.m, n = g.n, maxit = g.maxit;
    constexpr int LW = W + 1;
    double* Vs = sm + (size_t) wv * (W * LW + W);
    double* zs = Vs + W * LW;
    const double* Aq = g.A + q * g.sA;
    const double* Bq = g.B + q * g.sB;
    const bool row = lane < m, var = lane < n;
    const bool robust = g.loss != 0;
    // 1. lane i: the prior weight of row i
    const double p = !row ? 0.0 : (g.prior ? g.prior[q * g.sprior + lane] : 1.0);
    const double sfix = g.scale_in ? g.scale_in[q] : 1.0;
    if (__ballot(ir_bad_prior(p)) || ir_bad_scale(sfix)) {        // (all or nothing: nothing else is written)
        if (lane == 0) g.info[q] = -1;
        return;
    }
    const bool incl = p > 0.0;                // (false in lanes >= m)
    const unsigned long long im = __ballot(incl);
    const int cnt = __popcll(im);
    // 2. the start
    bool havex = robust && g.X0 != nullptr, haveold = havex, solved = false;
    double x = (havex && var) ? g.X0[q * g.sX0 + lane] : 0.0, xold = x;
    double w = 1.0, s = 0.0, rss = 0.0;
    int it = 0, status = 0;
    double a[W];
    for (;;) {                                // (every pass either ends or solves: at most maxit + 1 passes)
        // row i of the untouched [A | b]; an excluded row is zeros whatever it holds
#pragma unroll
        for (int c = 0; c < W; ++c) {
            double v = 0.0;
            if (incl && c < n) v = Aq[(size_t) c * g.lda + lane];
            a[c] = v;
        }
        double bi = 0.0;
        if (incl) bi = Bq[lane];
        if (havex) {
            // 4. the residual of x, the scale and the weights
            double r = bi;
#pragma unroll
            for (int c = 0; c < W; ++c)
                if (c < n) r = fma(-a[c], qb_bcast(x, c), r);
            rss = qb_wave_sum(r * r);
            if (!robust) break;               // (status 0)
            const double v = fabs(r);
            s = g.scale_in ? sfix : ir_wave_median(v, incl, im, cnt, m, lane) / IR_MAD;
            if (s == 0.0) { status = 2; w = 1.0; break; }
            w = ir_weight(g.loss, v / s, g.tune);
            // 5. the stopping test
            if (solved && haveold) {
                const double xm = ir_wave_max(var ? fabs(x) : 0.0);
                if (!__ballot(var && !(fabs(x - xold) <= g.tol * xm))) break;       // (status 0; a NaN never passes)
            }
            xold = x;
            haveold = true;
        }
        // 3. one solve
        const double cw = p * w;
        if (__popcll(__ballot(incl && cw > 0.0)) < n) {           // (all or nothing: nothing else is written)
            if (lane == 0) g.info[q] = -2;
            return;
        }
        if (it == maxit) { status = 3; break; }
        ++it;
        const double sq = incl ? sqrt(cw) : 0.0;
#pragma unroll
        for (int c = 0; c < W; ++c) a[c] = c == n ? bi * sq : a[c] * sq;         // (columns past n hold zeros; n < W)
        double tauv = 0.0, diag = 1.0;        // lane j: R(j, j)
#pragma unroll
        for (int j = 0; j < W; ++j) {
            if (j < n) qb_wave_col<W>(a, j, n + 1, lane, tauv, diag);            // (wave-uniform; b rides along)
        }
        const int sing = qb_info_wave(diag, n, lane);
        if (sing) {                           // (all or nothing: nothing else is written)
            if (lane == 0) g.info[q] = sing;
            return;
        }
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (c < n) {
                if (lane < n) Vs[c * LW + lane] = a[c];
            } else if (c == n) {
                if (lane < n) zs[lane] = a[c];
            }
        }
        QB_WAVE_SYNC();
        if (lane == 0) qb_trsv(Vs, LW, n, zs);
        QB_WAVE_SYNC();
        x = var ? zs[lane] : 0.0;
        QB_WAVE_SYNC();                       // (zs is read no more: the next solve may write it)
        solved = true;
        havex = true;
    }
    if (var) g.X[q * g.sX + lane] = x;
    if (row && g.W) g.W[q * g.sW + lane] = w;
    if (lane == 0) {
        if (g.scale) g.scale[q] = s;
        if (g.resid) g.resid[q] = sqrt(rss);
        if (g.iter) g.iter[q] = it;
        if (g.status) g.status[q] = status;
        g.info[q] = 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// workgroup route.  LDS: As[c * ld + i] = the image (n + 1 columns, ld = qb_ld(m)); rs, ws, vs (m each: r, the robust weights, and |r| on
// the included rows / -1 on the others for the median, then sqrt(c) for the refill); xs, xo (n each); then QB_WG_SMALL doubles: red[4],
// med[2], the scale, |r|^2, and the words (act, info, status, iter, nan, the count of included rows).
// ---------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr size_t ir_wg_doubles(int m, int n) { return (size_t) (n + 1) * qb_ld(m) + 3 * (size_t) m + 2 * (size_t) n + QB_WG_SMALL; }

enum { IR_GO = 1, IR_WRITE, IR_WRITE_ONES, IR_INFO };

__global__ void __launch_bounds__(256) ir_wg_kernel(const qrd_ir_args g)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const int m = g.m, n = g.n, maxit = g.maxit;
    const int ld = qb_ld(m);
    double* As = sm;
    double* rs = As + (size_t) (n + 1) * ld;
    double* ws = rs + m;
    double* vs = ws + m;
    double* xs = vs + m;
    double* xo = xs + n;
    double* red = xo + n;
    double* med = red + 4;
    double* ssc = red + 6;
    double* srss = red + 7;
    int* words = (int*) (red + 8);
    int *sact = words, *sinfo = words + 1, *sstat = words + 2, *siter = words + 3, *snan = words + 4, *scnt = words + 5;
    const double* Aq = g.A + q * g.sA;
    const double* Bq = g.B + q * g.sB;
    const double* Pq = g.prior ? g.prior + q * g.sprior : nullptr;
    const bool robust = g.loss != 0, fixed = g.scale_in != nullptr;
    bool havex = robust && g.X0 != nullptr;   // (the same value in every thread, here and below)
    // what only thread 0 reads and writes
    int it = 0;
    bool solved = false, haveold = havex;
    double sfix = 1.0;
    if (t == 0) {
        *sact = IR_GO; *sinfo = 0; *sstat = 0; *siter = 0; *snan = 0;
        *ssc = 0.0; *srss = 0.0;
    }
    __syncthreads();
    // 1. the checks; w = 1, sqrt(c) = sqrt(p), the count of rows with c > 0
    double pc = 0.0;
    for (int i = t; i < m; i += 256) {
        const double p = Pq ? Pq[i] : 1.0;
        if (ir_bad_prior(p)) *sinfo = -1;     // (every writer writes the same value)
        ws[i] = 1.0;
        vs[i] = p > 0.0 ? sqrt(p) : 0.0;
        pc += p > 0.0 ? 1.0 : 0.0;
    }
    if (t == 0 && fixed) {
        sfix = g.scale_in[q];
        if (ir_bad_scale(sfix)) *sinfo = -1;
    }
    for (int j = t; j < n; j += 256) {
        const double x0 = havex ? g.X0[q * g.sX0 + j] : 0.0;
        xs[j] = x0;
        xo[j] = x0;
    }
    pc = qb_wave_sum(pc);
    if (lane == 0) red[wv] = pc;
    __syncthreads();
    if (*sinfo) {                             // (all or nothing: nothing else is written)
        if (t == 0) g.info[q] = -1;
        return;
    }
    if (t == 0) *scnt = (int) (((red[0] + red[1]) + red[2]) + red[3]);
    if (havex) __syncthreads();               // (a warm start's first pass rewrites red; a cold start's reads this count of it first)
    // a pass: the residual of x and its decisions (once there is an x), then the count and one solve.  At most maxit + 1 passes
    for (int pass = 0; pass < maxit + 2; ++pass) {
        if (havex) {
            // 4. the residual of x from the untouched A
            double ss = 0.0;
            for (int i = t; i < m; i += 256) {
                const bool incl = (Pq ? Pq[i] : 1.0) > 0.0;
                double r = 0.0;
                if (incl) {
                    r = Bq[i];
                    for (int j = 0; j < n; ++j) r = fma(-Aq[(size_t) j * g.lda + i], xs[j], r);
                }
                rs[i] = r;
                vs[i] = incl ? fabs(r) : -1.0;
                if (incl && r != r) *snan = 1;                    // (every writer writes the same value)
                ss = fma(r, r, ss);
            }
            ss = qb_wave_sum(ss);
            if (lane == 0) red[wv] = ss;
            __syncthreads();
            if (robust && !fixed) {
                // the median by ranks: the two middle values go to med
                const int cnt = *scnt, k1 = (cnt - 1) >> 1, k2 = cnt >> 1;
                for (int i = t; i < m; i += 256) {
                    const double v = vs[i];
                    if (!(v >= 0.0)) continue;                    // (excluded, or a NaN: then snan is set)
                    int rank = 0;
                    for (int j = 0; j < m; ++j) {
                        const double vj = vs[j];
                        rank += (vj >= 0.0 && (vj < v || (vj == v && j < i))) ? 1 : 0;
                    }
                    if (rank == k1) med[0] = v;
                    if (rank == k2) med[1] = v;
                }
            }
            __syncthreads();
            if (t == 0) {
                *srss = ((red[0] + red[1]) + red[2]) + red[3];
                int act = IR_GO;
                if (!robust) act = IR_WRITE;  // (status 0)
                else {
                    const double s = fixed ? sfix : ((*snan || *scnt == 0) ? IR_NAN : 0.5 * (med[0] + med[1]) / IR_MAD);
                    *ssc = s;
                    if (s == 0.0) { *sstat = 2; act = IR_WRITE_ONES; }
                    else {
                        // 5. the stopping test
                        if (solved && haveold) {
                            double xm = 0.0;
                            for (int j = 0; j < n; ++j) xm = fmax(xm, fabs(xs[j]));
                            bool conv = true;
                            for (int j = 0; j < n; ++j) conv = conv && (fabs(xs[j] - xo[j]) <= g.tol * xm);     // (a NaN never passes)
                            if (conv) act = IR_WRITE;             // (status 0)
                        }
                        if (act == IR_GO) {
                            for (int j = 0; j < n; ++j) xo[j] = xs[j];
                            haveold = true;
                        }
                    }
                }
                *sact = act;
            }
            __syncthreads();
            const int act = *sact;            // the same word in every thread: the branches below are taken by all 256 or by none
            const double s = *ssc;
            pc = 0.0;
            if (robust) {
                for (int i = t; i < m; i += 256) {
                    const double p = Pq ? Pq[i] : 1.0;
                    const double w = act == IR_WRITE_ONES ? 1.0 : ir_weight(g.loss, fabs(rs[i]) / s, g.tune);
                    const double cw = p * w;
                    ws[i] = w;
                    vs[i] = p > 0.0 ? sqrt(cw) : 0.0;
                    pc += (p > 0.0 && cw > 0.0) ? 1.0 : 0.0;
                }
            }
            if (act != IR_GO) break;
            pc = qb_wave_sum(pc);
            if (lane == 0) red[wv] = pc;      // (thread 0 read red before the last barrier)
        }
        __syncthreads();
        // 3. the count, then one solve
        if (t == 0) {
            const int pos = (int) (((red[0] + red[1]) + red[2]) + red[3]);
            if (pos < n) { *sinfo = -2; *sact = IR_INFO; }
            else if (it == maxit) { *sstat = 3; *sact = IR_WRITE; }
            else { ++it; *sact = IR_GO; }
            *siter = it;
        }
        __syncthreads();
        if (*sact == IR_INFO) {               // (all or nothing: nothing else is written)
            if (t == 0) g.info[q] = *sinfo;
            return;
        }
        if (*sact != IR_GO) break;
        // the image: row i of [A | b] times sqrt(c_i), coalesced along the rows; an excluded row is zeros whatever it holds
        for (int c = wv; c <= n; c += 4) {
            const double* src = c < n ? Aq + (size_t) c * g.lda : Bq;
            for (int i = lane; i < m; i += 64) {
                double v = 0.0;
                if ((Pq ? Pq[i] : 1.0) > 0.0) v = src[i] * vs[i];
                As[c * ld + i] = v;
            }
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            qb_wg_col(As, ld, m, j, n + 1, red, t);
            __syncthreads();                  // (red and column j are read no more)
        }
        if (t == 0) {
            const int sing = qb_info_serial(As, ld, n);
            if (sing) { *sinfo = sing; *sact = IR_INFO; }
            else {
                double* zc = As + (size_t) n * ld;
                qb_trsv(As, ld, n, zc);
                for (int j = 0; j < n; ++j) xs[j] = zc[j];
                solved = true;
            }
        }
        __syncthreads();
        if (*sact == IR_INFO) {               // (all or nothing: nothing else is written)
            if (t == 0) g.info[q] = *sinfo;
            return;
        }
        havex = true;
    }
    __syncthreads();                          // (reached by all 256: both ways out of the loop are taken on a published word)
    for (int j = t; j < n; j += 256) g.X[q * g.sX + j] = xs[j];
    if (g.W)
        for (int i = t; i < m; i += 256) g.W[q * g.sW + i] = ws[i];
    if (t == 0) {
        if (g.scale) g.scale[q] = *ssc;
        if (g.resid) g.resid[q] = sqrt(*srss);
        if (g.iter) g.iter[q] = *siter;
        if (g.status) g.status[q] = *sstat;
        g.info[q] = 0;
    }
}

// the kernel that may ask for more than 64 KiB of LDS (qr_allow_lds)
static int ir_allow_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(ir_wg_kernel)};
    return qr_allow_lds(fns, QB_LDS_CAP, done);
}

template <int W>
static void ir_launch_wave(hipStream_t s, const qrd_ir_args& a)
{
    const size_t lds = sizeof(double) * 4 * (W * (W + 1) + W);
    hipLaunchKernelGGL(ir_wave_kernel<W>, dim3((unsigned) (((size_t) a.batch + 3) / 4)), dim3(256), lds, s, a);
}

extern "C" {

int qrd_ir_wave_route(int m, int n) { return m <= 64 && n + 1 <= 32; }

// the largest m the kernels take for n unknowns; 0: n is not taken at all.  The wave route needs no more than the workgroup route holds
// (64 rows of at most 32 columns), so the workgroup route's LDS budget decides.
int qrd_ir_max_rows(int n)
{
    if (n < 1 || n > QRD_B_MAX_N - 1) return 0;
    int m = QRD_B_MAX_ROWS;
    while (m >= n && sizeof(double) * ir_wg_doubles(m, n) > QB_LDS_CAP) --m;
    return m >= n ? m : 0;
}

int qrd_ir_solve(void* stream, const qrd_ir_args* a)
{
    if (!a) return -7;
    if (a->batch <= 0) return 0;
    const int mr = qrd_ir_max_rows(a->n);
    if (!mr || a->m < a->n || a->m > mr || a->lda < a->m || a->maxit < 1 || a->loss < 0 || a->loss > 2 || !(a->tune > 0.0) || !(a->tol >= 0.0) ||
        !a->A || !a->B || !a->X || !a->info)
        return -7;
    hipStream_t s = (hipStream_t) stream;
    if (qrd_ir_wave_route(a->m, a->n)) {
        if (a->n + 1 <= 8) ir_launch_wave<8>(s, *a);
        else if (a->n + 1 <= 16) ir_launch_wave<16>(s, *a);
        else ir_launch_wave<32>(s, *a);
    } else {
        const int rc = ir_allow_lds();
        if (rc) return rc;
        hipLaunchKernelGGL(ir_wg_kernel, dim3((unsigned) a->batch), dim3(256), sizeof(double) * ir_wg_doubles(a->m, a->n), s, *a);
    }
    return (int) hipGetLastError();
}

}   // extern "C"
