// qr_batched_bvls.hip -- kernels of the batched bound-constrained least squares (qr_batched_bvls.c, mi355x_qr.h section 8i): per member of a
// batch min |A x - b| subject to lo <= x <= hi (A: m x n, m >= n, one b) by bounded-variable least squares (Lawson & Hanson ch. 23, Stark
// & Parker's BVLS), the active-set loop of every member inside one launch:
//
//   1. start      finite lo: at lo (state -1); else finite hi: at hi (+1); else free (0), x = 0.  it = 0, no variable banned
//   2. outer test (skipped on the first pass if a variable is free) w = A^T (b - A x) from the untouched A; among the bound, non-banned
//                 variables with lo < hi the largest of w_j (at lo) / -w_j (at hi), ties to the smallest index; none > 0: done, info 0;
//                 else that variable t is freed
//   3. eliminate  it == maxit: done, info n + 1; else ++it, r = b - A_B x_B, Householder QR of A(:, F) (columns in increasing index order)
//                 with r riding along, R z = (Q^T r)(0 : |F|); an exactly zero R(i,i): info j + 1 (j the column in A), nothing else written
//   4. anti-cycle on the first elimination after t was freed: z_t on or outside the bound it left: t goes back, is banned, go to 2
//   5. accept     lo_F <= z <= hi_F: x_F = z, the bans are lifted, go to 2
//   6. blocked    alpha_j = (bound_j - x_j) / (z_j - x_j) over the free j with z_j outside; the smallest, ties to the smallest index k;
//                 x_F += alpha (z - x_F); x_k = its bound exactly, k bound; every other free variable on or outside a bound is put on it and
//                 bound; go to 3
//
// Every candidate is factored from scratch: the image [A_F | r] is refilled from the untouched A through the column map "image column c is
// A's column with the c-th set bit of the free mask", so that the shared column steps (qr_batched_dev.h) pivot on row j in column j and are
// called unchanged, with the end of the update at |F| + 1: r alone rides along.
//
//   bv_wave_kernel<W>  m <= 64 and n + 1 <= W <= 32: one wave per member, four per workgroup, no workgroup barrier.  Lane i holds row i of
//                      the image in W registers (every register index a constant; the column behind it is a wave-uniform scalar) and, as
//                      lane j < n, variable j: x_j, lo_j, hi_j, its state and w_j.  The free and the ban set are 32-bit ballots.  R and z go
//                      through the wave's LDS for qb_trsv.  Every decision is taken on a ballot or a butterfly: wave-uniform by construction
//   bv_wg_kernel       everything else that fits: one workgroup per member, the image in LDS at qb_ld(m), x, z, w, lo, hi, the states and
//                      the column map packed behind it.  Thread 0 takes every decision and publishes the next action in an LDS word that
//                      all threads read after a barrier: every thread reaches every barrier the same number of times
//
// `it` counts every elimination and it <= maxit is the only loop bound.  A comparison with a NaN is false and leads to the blocked step
// without a blocking variable, which changes nothing and eliminates again: the count ends it.  Every sum runs in an order that (m, n) and
// the free set fix; no atomics.
#include "qr_batched_dev.h"

static_assert(QRD_B_MAX_N == 64, "the workgroup route keeps its sets in 64-bit masks");

#define BV_INF __builtin_huge_val()

// no box: lo > hi, a NaN, lo == +inf or hi == -inf
__device__ __forceinline__ bool bv_bad_bounds(double lo, double hi) { return !(lo <= hi) || lo == BV_INF || hi == -BV_INF; }

// the same extremum in every lane (NaN operands are dropped by fmax / fmin: the callers pass none)
__device__ __forceinline__ double bv_wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double bv_wave_min(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}

// the index of the c-th set bit of mask (c < its population count)
__device__ __forceinline__ int bv_nth_bit(unsigned long long mask, int c)
{
    for (int k = 0; k < c; ++k) mask &= mask - 1;
    return __ffsll((long long) mask) - 1;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// wave route.  Dynamic LDS per wave: Vs[c * LW + r] = R(r, c) (LW = W + 1), then zs[W]: (Q^T r)(0 : |F|), then z.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(256) bv_wave_kernel(const qrd_bv_args g)
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
    const unsigned lbit = var ? 1u << lane : 0u;                  // (n < 32)
    // lane j < n: variable j
    const double lo = (var && g.lo) ? g.lo[q * g.sbnd + lane] : -BV_INF;
    const double hi = (var && g.hi) ? g.hi[q * g.sbnd + lane] : BV_INF;
    if (__ballot(var && bv_bad_bounds(lo, hi))) {                 // (all or nothing: nothing else is written)
        if (lane == 0) g.info[q] = -1;
        return;
    }
    int st = !var ? 2 : (lo != -BV_INF ? -1 : (hi != BV_INF ? 1 : 0));        // (lanes >= n: neither free nor bound)
    double x = st == -1 ? lo : (st == 1 ? hi : 0.0);
    double w = 0.0, z = 0.0, rss = 0.0;
    unsigned ban = 0;
    int it = 0, info = 0, tvar = 0, tfrom = 0;
    bool pend = false, fin = false;
    bool test = (unsigned) __ballot(st == 0) == 0;                // the first pass skips the test if a variable is free
    double a[W];
    for (;;) {                                // (every pass either ends or eliminates: at most maxit + 1 passes)
        if (test || fin) {
            // w = A^T (b - A x) and |A x - b|^2 from the untouched A, the row in identity order
#pragma unroll
            for (int c = 0; c < W; ++c) a[c] = (row && c < n) ? Aq[(size_t) c * g.lda + lane] : 0.0;
            double rf = row ? Bq[lane] : 0.0;
#pragma unroll
            for (int c = 0; c < W; ++c)
                if (c < n) rf = fma(-a[c], qb_bcast(x, c), rf);
            rss = qb_wave_sum(rf * rf);
#pragma unroll
            for (int c = 0; c < W; ++c) {
                if (c < n) {
                    const double s = qb_wave_sum(a[c] * rf);
                    if (lane == c) w = s;
                }
            }
        }
        if (fin) break;
        if (test) {
            // 2. the bound variable that gains most from leaving its bound
            const double cv = st == -1 ? w : -w;
            const bool cand = (st == -1 || st == 1) && !(ban & lbit) && lo < hi && cv > 0.0;
            const double best = bv_wave_max(cand ? cv : 0.0);
            const unsigned long long pick = __ballot(cand && cv == best);
            if (!pick) break;                 // (info 0; a NaN in w leaves no candidate)
            tvar = __ffsll((long long) pick) - 1;
            if (lane == tvar) { tfrom = st; st = 0; }
            tfrom = __shfl(tfrom, tvar);
            pend = true;
        }
        test = true;
        for (;;) {
            // 3. one elimination
            if (it == maxit) { info = n + 1; fin = true; break; }
            ++it;
            const unsigned fm = (unsigned) __ballot(st == 0);
            const int nf = __popc(fm);
            double r = row ? Bq[lane] : 0.0;
            for (int j = 0; j < n; ++j) {
                if (!((fm >> j) & 1u)) {      // (wave-uniform) a bound column, ascending
                    const double av = row ? Aq[(size_t) j * g.lda + lane] : 0.0;
                    r = fma(-av, qb_bcast(x, j), r);
                }
            }
            unsigned rem = fm;
#pragma unroll
            for (int c = 0; c < W; ++c) {
                double v = 0.0;
                if (rem) {                    // (wave-uniform: the column behind register c is a scalar)
                    const int j = __ffs((int) rem) - 1;
                    rem &= rem - 1;
                    if (row) v = Aq[(size_t) j * g.lda + lane];
                }
                a[c] = v;
            }
#pragma unroll
            for (int cc = 0; cc < W; ++cc)
                if (cc == nf) a[cc] = r;      // (nf <= n < W)
            double tauv = 0.0, diag = 1.0;    // lane j: R(j, j)
#pragma unroll
            for (int j = 0; j < W; ++j) {
                if (j < nf) qb_wave_col<W>(a, j, nf + 1, lane, tauv, diag);      // (wave-uniform)
            }
            const int sing = qb_info_wave(diag, nf, lane);
            if (sing) {                       // (all or nothing: nothing else is written)
                if (lane == 0) g.info[q] = bv_nth_bit(fm, sing - 1) + 1;
                return;
            }
#pragma unroll
            for (int c = 0; c < W; ++c) {
                if (c < nf) {
                    if (lane <= c) Vs[c * LW + lane] = a[c];
                } else if (c == nf) {
                    if (lane < nf) zs[lane] = a[c];
                }
            }
            QB_WAVE_SYNC();
            if (lane == 0) qb_trsv(Vs, LW, nf, zs);
            QB_WAVE_SYNC();
            const bool fr = st == 0;
            z = fr ? zs[__popc(fm & (lbit - 1u))] : 0.0;          // variable j's z sits at its rank among the free ones
            QB_WAVE_SYNC();                   // (zs is read no more: the next elimination may write it)
            // 4. the variable just freed must move into its box
            if (pend) {
                pend = false;
                if (__ballot(lane == tvar && ((tfrom == -1 && z <= lo) || (tfrom == 1 && z >= hi)))) {
                    if (lane == tvar) st = tfrom;                 // (x_t never left the bound)
                    ban |= 1u << tvar;
                    break;
                }
            }
            // 5. accept
            if (!__ballot(fr && !(lo <= z && z <= hi))) {
                if (fr) x = z;
                ban = 0;
                break;
            }
            // 6. the longest step towards z that stays in the box
            const bool below = fr && z < lo, out = below || (fr && z > hi);
            const double bnd = below ? lo : hi;
            const double al = out ? (bnd - x) / (z - x) : BV_INF;
            const double amin = bv_wave_min(al);
            const unsigned long long blk = __ballot(out && al == amin);
            if (blk) {                        // (none: a NaN in z; nothing moves and the count ends the loop)
                const int kv = __ffsll((long long) blk) - 1;
                if (fr) x = x + amin * (z - x);
                if (lane == kv) { x = bnd; st = below ? -1 : 1; }
                if (st == 0) {
                    if (x <= lo) { x = lo; st = -1; }
                    else if (x >= hi) { x = hi; st = 1; }
                }
            }
        }
    }
    if (var) {
        g.X[q * g.sX + lane] = x;
        if (g.W) g.W[q * g.sW + lane] = w;
        if (g.state) g.state[q * g.sstate + lane] = st;
    }
    if (lane == 0) {
        if (g.resid) g.resid[q] = sqrt(rss);
        if (g.iter) g.iter[q] = it;
        g.info[q] = info;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// workgroup route.  LDS: As[c * ld + i] = [A_F | r] (at most n + 1 columns, ld = qb_ld(m); column 0 also takes b - A x for w); xs, zs, ws,
// los, his (n each); st and cmap (n ints each: the states, A's column behind image column c); red[4]; the words (act, nf, info, iter).
// ---------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr size_t bv_wg_doubles(int m, int n) { return (size_t) (n + 1) * qb_ld(m) + 6 * (size_t) n + QB_WG_SMALL; }

enum { BV_TEST = 1, BV_COUNT, BV_ELIM, BV_WRITE, BV_INFO };

// thread 0: the column map of the free set; returns |F|
__device__ __forceinline__ int bv_wg_map(const int* st, int* cmap, int n)
{
    int nf = 0;
    for (int j = 0; j < n; ++j)
        if (st[j] == 0) cmap[nf++] = j;
    return nf;
}

__global__ void __launch_bounds__(256) bv_wg_kernel(const qrd_bv_args g)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const int m = g.m, n = g.n, maxit = g.maxit;
    const int ld = qb_ld(m);
    double* As = sm;
    double* xs = As + (size_t) (n + 1) * ld;
    double* zv = xs + n;
    double* ws = zv + n;
    double* los = ws + n;
    double* his = los + n;
    int* st = (int*) (his + n);
    int* cmap = st + n;
    double* red = his + 2 * n;                // (2 n ints take n doubles)
    int* words = (int*) (red + 4);
    int *sact = words, *snf = words + 1, *sinfo = words + 2, *siter = words + 3;
    const double* Aq = g.A + q * g.sA;
    const double* Bq = g.B + q * g.sB;
    // what only thread 0 reads and writes
    unsigned long long ban = 0;
    int it = 0, tvar = 0, tfrom = 0;
    bool pend = false;
    for (int j = t; j < n; j += 256) {
        los[j] = g.lo ? g.lo[q * g.sbnd + j] : -BV_INF;
        his[j] = g.hi ? g.hi[q * g.sbnd + j] : BV_INF;
    }
    __syncthreads();
    if (t == 0) {
        // 1. the start
        bool bad = false;
        for (int j = 0; j < n; ++j) {
            const double lo = los[j], hi = his[j];
            bad = bad || bv_bad_bounds(lo, hi);
            st[j] = lo != -BV_INF ? -1 : (hi != BV_INF ? 1 : 0);
            xs[j] = st[j] == -1 ? lo : (st[j] == 1 ? hi : 0.0);
            ws[j] = 0.0;
        }
        const int nf = bv_wg_map(st, cmap, n);
        *snf = nf;
        *sinfo = bad ? -1 : 0;
        if (bad) *sact = BV_INFO;
        else if (nf) { *sact = BV_ELIM; it = 1; }                 // the first pass skips the test if a variable is free (maxit >= 1)
        else *sact = BV_TEST;
    }
    // every action below ends in a decision of thread 0; an elimination is followed by a test, a count or an elimination, a test by an
    // elimination or the end: at most 2 maxit + 3 actions
    for (int guard = 0; guard < 2 * maxit + 4; ++guard) {
        __syncthreads();                      // (thread 0's decision is written; the LDS of the last action is read no more)
        const int act = *sact;                // the same word in every thread: the branches below are taken by all 256 or by none
        const int nf = *snf;
        if (act == BV_INFO) {                 // (all or nothing: nothing else is written)
            if (t == 0) g.info[q] = *sinfo;
            return;
        }
        if (act == BV_WRITE) {
            for (int j = t; j < n; j += 256) {
                g.X[q * g.sX + j] = xs[j];
                if (g.W) g.W[q * g.sW + j] = ws[j];
                if (g.state) g.state[q * g.sstate + j] = st[j];
            }
            if (t == 0) {
                if (g.resid) g.resid[q] = sqrt(((red[0] + red[1]) + red[2]) + red[3]);
                if (g.iter) g.iter[q] = *siter;
                g.info[q] = *sinfo;
            }
            return;
        }
        if (act == BV_TEST || act == BV_COUNT) {
            // w = A^T (b - A x) and |A x - b|^2 from the untouched A; b - A x in column 0 of the (dead) image
            double ss = 0.0;
            for (int i = t; i < m; i += 256) {
                double rf = Bq[i];
                for (int j = 0; j < n; ++j) rf = fma(-Aq[(size_t) j * g.lda + i], xs[j], rf);
                As[i] = rf;
                ss = fma(rf, rf, ss);
            }
            ss = qb_wave_sum(ss);
            if (lane == 0) red[wv] = ss;
            __syncthreads();
            for (int j = wv; j < n; j += 4) {
                const double* aj = Aq + (size_t) j * g.lda;
                double s = 0.0;
                for (int i = lane; i < m; i += 64) s = fma(aj[i], As[i], s);
                s = qb_wave_sum(s);
                if (lane == 0) ws[j] = s;
            }
            __syncthreads();
            if (t == 0) {
                *siter = it;
                if (act == BV_COUNT) {
                    *sinfo = n + 1;
                    *sact = BV_WRITE;
                } else {
                    // 2. the bound variable that gains most from leaving its bound; ties to the smallest index
                    int best = -1;
                    double bv = 0.0;
                    for (int j = 0; j < n; ++j) {
                        if (st[j] == 0 || ((ban >> j) & 1ull) || !(los[j] < his[j])) continue;
                        const double cv = st[j] == -1 ? ws[j] : -ws[j];
                        if (cv > bv) { bv = cv; best = j; }
                    }
                    if (best < 0) {
                        *sinfo = 0;
                        *sact = BV_WRITE;
                    } else if (it == maxit) {                     // (x has not moved: w and the sum are those of the iterate returned)
                        tfrom = st[best];
                        st[best] = 0;
                        *sinfo = n + 1;
                        *sact = BV_WRITE;
                    } else {
                        tvar = best;
                        tfrom = st[best];
                        st[best] = 0;
                        pend = true;
                        ++it;
                        *snf = bv_wg_map(st, cmap, n);
                        *sact = BV_ELIM;
                    }
                }
            }
            continue;
        }
        // 3. act == BV_ELIM: the image [A_F | r], refilled through the column map
        for (int c = wv; c < nf; c += 4) {
            const double* src = Aq + (size_t) cmap[c] * g.lda;
            for (int i = lane; i < m; i += 64) As[c * ld + i] = src[i];
        }
        for (int i = t; i < m; i += 256) {
            double r = Bq[i];
            for (int j = 0; j < n; ++j)
                if (st[j] != 0) r = fma(-Aq[(size_t) j * g.lda + i], xs[j], r);         // the bound columns, ascending
            As[nf * ld + i] = r;
        }
        __syncthreads();
        for (int j = 0; j < nf; ++j) {
            qb_wg_col(As, ld, m, j, nf + 1, red, t);
            __syncthreads();                  // (red and column j are read no more)
        }
        if (t == 0) {
            double* zc = As + (size_t) nf * ld;
            const int sing = qb_info_serial(As, ld, nf);
            bool decided = false;
            if (sing) {
                *sinfo = cmap[sing - 1] + 1;
                *sact = BV_INFO;
                decided = true;
            } else {
                qb_trsv(As, ld, nf, zc);
                for (int c = 0; c < nf; ++c) zv[cmap[c]] = zc[c];
            }
            // 4. the variable just freed must move into its box
            if (!decided && pend) {
                pend = false;
                const double z = zv[tvar];
                if ((tfrom == -1 && z <= los[tvar]) || (tfrom == 1 && z >= his[tvar])) {
                    st[tvar] = tfrom;         // (x_t never left the bound)
                    ban |= 1ull << tvar;
                    *sact = BV_TEST;
                    decided = true;
                }
            }
            if (!decided) {
                bool ok = true;
                for (int c = 0; c < nf; ++c) {
                    const int j = cmap[c];
                    ok = ok && (los[j] <= zv[j] && zv[j] <= his[j]);
                }
                if (ok) {                     // 5. accept
                    for (int c = 0; c < nf; ++c) xs[cmap[c]] = zv[cmap[c]];
                    ban = 0;
                    *sact = BV_TEST;
                } else {                      // 6. the longest step towards z that stays in the box
                    int kv = -1;
                    double amin = BV_INF, kb = 0.0;
                    for (int c = 0; c < nf; ++c) {
                        const int j = cmap[c];
                        const double z = zv[j];
                        const bool below = z < los[j];
                        if (!(below || z > his[j])) continue;
                        const double bnd = below ? los[j] : his[j];
                        const double al = (bnd - xs[j]) / (z - xs[j]);
                        if (kv < 0 ? al <= amin : al < amin) { amin = al; kv = j; kb = bnd; }
                    }
                    if (kv >= 0) {            // (none: a NaN in z; nothing moves and the count ends the loop)
                        const int sk = zv[kv] < los[kv] ? -1 : 1;
                        for (int c = 0; c < nf; ++c) {
                            const int j = cmap[c];
                            xs[j] = xs[j] + amin * (zv[j] - xs[j]);
                        }
                        xs[kv] = kb;
                        st[kv] = sk;
                        for (int c = 0; c < nf; ++c) {
                            const int j = cmap[c];
                            if (st[j] != 0) continue;
                            if (xs[j] <= los[j]) { xs[j] = los[j]; st[j] = -1; }
                            else if (xs[j] >= his[j]) { xs[j] = his[j]; st[j] = 1; }
                        }
                    }
                    if (it == maxit) *sact = BV_COUNT;
                    else {
                        ++it;
                        *snf = bv_wg_map(st, cmap, n);
                        *sact = BV_ELIM;
                    }
                }
            }
        }
    }
}

// the kernel that may ask for more than 64 KiB of LDS (qr_allow_lds)
static int bv_allow_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(bv_wg_kernel)};
    return qr_allow_lds(fns, QB_LDS_CAP, done);
}

template <int W>
static void bv_launch_wave(hipStream_t s, const qrd_bv_args& a)
{
    const size_t lds = sizeof(double) * 4 * (W * (W + 1) + W);
    hipLaunchKernelGGL(bv_wave_kernel<W>, dim3((unsigned) (((size_t) a.batch + 3) / 4)), dim3(256), lds, s, a);
}

extern "C" {

int qrd_bv_wave_route(int m, int n) { return m <= 64 && n + 1 <= 32; }

// the largest m the kernels take for n unknowns; 0: n is not taken at all.  The wave route needs no more than the workgroup route holds
// (64 rows of at most 32 columns), so the workgroup route's LDS budget decides.
int qrd_bv_max_rows(int n)
{
    if (n < 1 || n > QRD_B_MAX_N - 1) return 0;
    int m = QRD_B_MAX_ROWS;
    while (m >= n && sizeof(double) * bv_wg_doubles(m, n) > QB_LDS_CAP) --m;
    return m >= n ? m : 0;
}

int qrd_bv_solve(void* stream, const qrd_bv_args* a)
{
    if (!a) return -7;
    if (a->batch <= 0) return 0;
    const int mr = qrd_bv_max_rows(a->n);
    if (!mr || a->m < a->n || a->m > mr || a->lda < a->m || a->maxit < 1 || !a->A || !a->B || !a->X || !a->info) return -7;
    hipStream_t s = (hipStream_t) stream;
    if (qrd_bv_wave_route(a->m, a->n)) {
        if (a->n + 1 <= 8) bv_launch_wave<8>(s, *a);
        else if (a->n + 1 <= 16) bv_launch_wave<16>(s, *a);
        else bv_launch_wave<32>(s, *a);
    } else {
        const int rc = bv_allow_lds();
        if (rc) return rc;
        hipLaunchKernelGGL(bv_wg_kernel, dim3((unsigned) a->batch), dim3(256), sizeof(double) * bv_wg_doubles(a->m, a->n), s, *a);
    }
    return (int) hipGetLastError();
}

}   // extern "C"
