// qr_batched_lsei.hip -- kernels of the batched inequality-constrained least squares (qr_batched_lsei.c, mi355x_qr.h section 8l): per member
// of a batch min |A x - b| subject to G(0:neq, :) x = h(0:neq), G(neq:mg, :) x >= h(neq:mg) (A: m x n, G: mg x n, mg <= 64, one b; Lawson &
// Hanson's LSEI) by a dual active-set loop, the loop of every member inside one launch.  The state is the working set W (a 64-bit mask; rows
// < neq are in it for good), mu (mg), x, the ban mask and the count `it`.  A candidate of a row set S is the solution of min |A x - b|
// subject to G_S x = h_S by steps 1 to 8 of qr_batched_lse.hip (a plain factorisation of [A | b] for an empty S): x_S and zeta = -lambda_S,
// A^T (A x_S - b) = G_S^T zeta; the rows of S in ascending order, a pending row t last.
//
//   1. start      W = {0 .. neq-1}, it = 1, (x, mu_W) = candidate(W).  An exactly zero R_c(i,i): info -3; an exactly zero R_a(i,i), here or
//                 in any later candidate: info i + 1; nothing else is written for either
//   2. outer test s = G x - h from the untouched G; among the rows i >= neq outside W and not banned the most negative s_i, ties to the
//                 smallest index; none < 0: done, info 0; else t is that row, mu_t = 0, pend = true
//   3. count      it == maxit: done, info n + 1, the last accepted (x, mu) is written; else ++it
//   4. dependence [G_W^T | G_t^T] is factored over its first |W| columns, the last riding along; rho = the norm of its rows |W| .. n-1.
//                 |W| == n or rho <= rcond |G_t|: c = R_c^-1 (its top |W| entries); theta = min mu_i / c_i over the inequalities i of W with
//                 c_i > 0, ties to the smallest index k; none: info -2 (infeasible), nothing else written; else mu_W -= theta c,
//                 mu_t += theta, mu_k = 0 and k leaves W, every other inequality of W with mu <= 0 is set to 0 and leaves; pend = false;
//                 go to 3.  Otherwise the same factorisation is completed with t's column
//   5. candidate  (x_c, zeta) = candidate(W + {t})
//   6. anti-cycle only with pend set, which it clears: zeta_t <= 0: t is banned, mu_t = 0, go to 2
//   7. accept     zeta_i > 0 for every inequality i of W + {t}: W gains t, mu = zeta on W and 0 elsewhere, x = x_c, the bans are lifted, go to 2
//   8. blocked    alpha = min mu_i / (mu_i - zeta_i) over the inequalities i of W + {t} with zeta_i <= 0, ties to the smallest index k.
//                 k == t (not in exact arithmetic): nothing moves -- W and mu are the accepted pair's again --, t is banned, go to 2.  Else
//                 mu_i += alpha (zeta_i - mu_i) over W + {t}, mu_k = 0 and k leaves W, every other inequality of W with mu <= 0 is set to 0
//                 and leaves; go to 3 (t stays pending)
//
// At the end x is the accepted candidate's; s = G x - h and resid = |A x - b| are recomputed from the untouched A, G and x.
//
// Every candidate is factored from scratch from the untouched inputs: the image of G_S^T is refilled through the row map "image column c is
// G's row with the c-th set bit of W, t last", the image of A is [A~2 | A~1 | r] as in qr_batched_lse.hip, so that the shared column steps
// (qr_batched_dev.h) are called unchanged.
//
//   le_wave_kernel<W>  m <= 64 and n + 1 <= W <= 32: one wave per member, four per workgroup, no workgroup barrier.  Lane i < mg owns
//                      constraint i (h_i, s_i, mu_i and the accepted mu_i), lane j < n row j of G_S^T and x_j, lane i < m row i of the image
//                      of A, in W registers; the factors of G_S^T are spilled to the wave's LDS.  W and the ban set are 64-bit ballots,
//                      every decision comes from a ballot or a butterfly
//   le_wg_kernel       everything else that fits: one workgroup per member, the image of A in LDS at qb_ld(m), the factors of G_S^T beside
//                      it at qb_ld(n), mu, the accepted mu, zeta, s, h, the row map and the action words packed behind them.  Thread 0 takes
//                      every decision and publishes the next action in an LDS word that all threads read after a barrier: every thread
//                      reaches every barrier the same number of times
//
// `it` counts every candidate and it <= maxit is the only loop bound.  A comparison with a NaN is false and leads towards the count.  Every
// sum runs in an order that the shape and the set fix; no atomics.
#include "qr_batched_dev.h"

static_assert(QRD_B_MAX_N == 64, "the sets are 64-bit masks and tau of G_S^T is kept in 64 doubles of LDS");

#define LE_INF __builtin_huge_val()

// A's column behind image column c < n (k = n - p)
__device__ __forceinline__ int le_src(int c, int k, int p) { return c < k ? c + p : c - k; }

// the same minimum in every lane (NaN operands are dropped by fmin)
__device__ __forceinline__ double le_wave_min(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// wave route.  Dynamic LDS per wave (LW = W + 1):
//   Vs[c * LW + r]   c < p: the factors of G_S^T (R_c on and above the diagonal, V_c below); p <= c < n: R_a(r, c - p); c == n: g, then lambda
//   Xs[r]            h_S, then [y1 ; y2] (in the dependence step: the riding column, then c)
//   tc[j]            tau of G_S^T
// ---------------------------------------------------------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(256) le_wave_kernel(const qrd_le_args g)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) g.batch) return;        // (no workgroup barrier below: the waves of a workgroup are independent)
    const int m = g.m, n = g.n, mg = g.mg, neq = g.neq, maxit = g.maxit;
    constexpr int LW = W + 1;
    double* Vs = sm + (size_t) wv * (W * LW + LW + W);
    double* Xs = Vs + W * LW;
    double* tc = Xs + LW;
    const double* Aq = g.A + q * g.sA;
    const double* Bq = g.B + q * g.sB;
    const double* Gq = g.G + q * g.sG;
    const double* Hq = g.H + q * g.sH;
    const bool row = lane < m, var = lane < n, con = lane < mg, ineq = con && lane >= neq;
    const unsigned long long lbit = 1ull << lane;
    const double h = con ? Hq[lane] : 0.0;
    double mu = 0.0, muacc = 0.0, x = 0.0, s = 0.0;
    unsigned long long Wm = neq >= 64 ? ~0ull : (1ull << neq) - 1ull, Wacc = Wm, ban = 0;
    int it = 1, info = 0, tt = 0;
    bool havet = false, pend = false;
    double a[W];
    for (;;) {                                // (every pass is one candidate or one dependence step: at most maxit passes)
        const int pw = __popcll(Wm), p = pw + (havet ? 1 : 0), k = n - p;
        const bool inW = (Wm & lbit) != 0, inS = inW || (havet && lane == tt);
        const int rank = inW ? __popcll(Wm & (lbit - 1ull)) : pw;           // the column of constraint `lane` in the image of G_S^T
        bool dep = false;
        if (p > 0) {
            // lane i: row i of G_S^T, which is column i of G through the row map
            unsigned long long rem = Wm;
#pragma unroll
            for (int c = 0; c < W; ++c) {
                double v = 0.0;
                if (c < p) {                  // (wave-uniform: the row behind register c is a scalar)
                    int i = tt;
                    if (rem) {
                        i = __ffsll((long long) rem) - 1;
                        rem &= rem - 1ull;
                    }
                    if (var) v = Gq[(size_t) lane * g.ldg + i];
                }
                a[c] = v;
            }
            double gn = 0.0;
            if (havet) {
                double col = 0.0;
#pragma unroll
                for (int cc = 0; cc < W; ++cc)
                    if (cc == pw) col = a[cc];
                gn = sqrt(qb_wave_sum(col * col));
            }
            double tauv = 0.0, diag = 1.0;    // lane j: tau_c[j] and R_c(j, j)
#pragma unroll
            for (int j = 0; j < W; ++j) {
                if (havet && j == pw) {       // 4. (wave-uniform) what is left of t's column below the rows of W
                    const double y = lane >= pw ? a[j] : 0.0;             // (lanes >= n hold zeros)
                    const double rho = sqrt(qb_wave_sum(y * y));
                    dep = pw == n || rho <= g.rcond * gn;
                }
                if (j < p && !dep) qb_wave_col<W>(a, j, p, lane, tauv, diag);       // (wave-uniform)
            }
            if (dep) {
                // c = R_c^-1 (the top |W| entries of the riding column)
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    if (c < pw) {
                        if (lane <= c) Vs[c * LW + lane] = a[c];
                    } else if (c == pw) {
                        if (lane < pw) Xs[lane] = a[c];
                    }
                }
                QB_WAVE_SYNC();
                if (lane == 0) qb_trsv(Vs, LW, pw, Xs);
                QB_WAVE_SYNC();
                const double cv = inW ? Xs[rank] : 0.0;
                QB_WAVE_SYNC();               // (Xs is read no more: the next pass may write it)
                const bool el = inW && ineq && cv > 0.0;
                const double ratio = el ? mu / cv : LE_INF;
                const double theta = le_wave_min(ratio);
                const unsigned long long pick = __ballot(el && ratio == theta);
                if (!pick) {                  // (infeasible; all or nothing: nothing else is written)
                    if (lane == 0) g.info[q] = -2;
                    return;
                }
                const int kv = __ffsll((long long) pick) - 1;
                if (inW) mu = mu - theta * cv;
                if (lane == tt) mu = mu + theta;
                const unsigned long long leave = __ballot(inW && ineq && (lane == kv || mu <= 0.0));
                if (leave & lbit) mu = 0.0;
                Wm &= ~leave;
                pend = false;
                if (it == maxit) { info = n + 1; break; }                 // 3.
                ++it;
                continue;
            }
            if (qb_info_wave(diag, p, lane)) {                            // (all or nothing: nothing else is written)
                if (lane == 0) g.info[q] = -3;
                return;
            }
#pragma unroll
            for (int c = 0; c < W; ++c)
                if (c < p && var) Vs[c * LW + lane] = a[c];
            if (lane < p) tc[lane] = tauv;
            if (inS) Xs[rank] = h;
            QB_WAVE_SYNC();
            if (lane == 0) qb_trsv_t(Vs, LW, p, Xs);                      // R_c^T y1 = h_S
            QB_WAVE_SYNC();
        }
        // lane i: row i of [A~2 | A~1 | b] before the sweep
#pragma unroll
        for (int c = 0; c < W; ++c) {
            double v = 0.0;
            if (row && c < n) v = Aq[(size_t) le_src(c, k, p) * g.lda + lane];
            else if (row && c == n) v = Bq[lane];
            a[c] = v;
        }
        // row <- row H_0 .. H_{p-1}: no cross-lane sum; v_j(i) is read at the same address by every lane
        for (int j = 0; j < p; ++j) {
            const double tj = tc[j];
            if (tj == 0.0) continue;          // (H = I; wave-uniform)
            const double* vj = Vs + j * LW;
            double d = 0.0;
#pragma unroll
            for (int c = 0; c < W; ++c) {
                if (c < n) {
                    const int i = le_src(c, k, p);
                    if (i >= j) d = fma(a[c], i == j ? 1.0 : vj[i], d);
                }
            }
            const double w = tj * d;
#pragma unroll
            for (int c = 0; c < W; ++c) {
                if (c < n) {
                    const int i = le_src(c, k, p);
                    if (i >= j) a[c] = fma(-w, i == j ? 1.0 : vj[i], a[c]);
                }
            }
        }
        // r = b - A~1 y1: one sum over A~1's columns ascending, then the one register it belongs to takes it
        if (p > 0) {
            double sy = 0.0;
#pragma unroll
            for (int c = 0; c < W; ++c)
                if (c >= k && c < n) sy = fma(a[c], Xs[c - k], sy);
#pragma unroll
            for (int cc = 1; cc < W; ++cc)
                if (cc == n) a[cc] -= sy;
        }
        // the column step on A~2; A~1 and r ride along
        double taua = 0.0, da = 1.0;          // lane j: R_a(j, j)
#pragma unroll
        for (int j = 0; j < W; ++j) {
            if (j < k) qb_wave_col<W>(a, j, n + 1, lane, taua, da);       // (wave-uniform)
        }
        const int ia = qb_info_wave(da, k, lane);
        if (ia) {                             // (all or nothing: nothing else is written)
            if (lane == 0) g.info[q] = ia;
            return;
        }
        // R_a and the top of t into LDS; g from the rows >= n - p (rows >= m hold zeros)
        double tl = 0.0;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (c < k) {
                if (lane < k) Vs[(p + c) * LW + lane] = a[c];
            } else if (c == n) {
                if (lane < k) Xs[p + lane] = a[c];
                tl = lane >= k ? a[c] : 0.0;
            }
        }
        if (p > 0) {
#pragma unroll
            for (int c = 0; c < W; ++c) {
                if (c >= k && c < n) {
                    const double gi = qb_wave_sum(tl * a[c]);
                    if (lane == 0) Vs[n * LW + (c - k)] = gi;
                }
            }
        }
        QB_WAVE_SYNC();
        if (lane == 0) {
            qb_trsv(Vs + p * LW, LW, k, Xs + p);                          // R_a y2 = t(0 : n-p)
            if (p > 0) qb_trsv(Vs, LW, p, Vs + n * LW);                   // R_c lambda = g
        }
        QB_WAVE_SYNC();
        // x_c = Q_c [y1 ; y2]: one butterfly per reflector
        double xc = var ? Xs[lane] : 0.0;
        for (int j = p - 1; j >= 0; --j) {
            const double tj = tc[j];
            if (tj == 0.0) continue;          // (H = I; wave-uniform)
            const double v = lane > j ? (var ? Vs[j * LW + lane] : 0.0) : (lane == j ? 1.0 : 0.0);
            const double tw = tj * qb_wave_sum(v * xc);
            xc = fma(-tw, v, xc);
        }
        const double zeta = inS ? -Vs[n * LW + rank] : 0.0;
        QB_WAVE_SYNC();                       // (the LDS of this candidate is read no more: the next pass may write it)
        bool accept = !havet, test = !havet;  // 1. the start is accepted as it is
        if (havet) {
            // 6. the row just taken must come out with a positive multiplier
            if (pend) {
                pend = false;
                if (__ballot(lane == tt && zeta <= 0.0)) {
                    ban |= 1ull << tt;
                    if (lane == tt) mu = 0.0;
                    test = true;
                }
            }
            // 7. accept
            if (!test && !__ballot(inS && ineq && !(zeta > 0.0))) accept = test = true;
        }
        if (accept) {
            if (havet) Wm |= 1ull << tt;
            mu = inS ? zeta : 0.0;
            x = xc;
            muacc = mu;
            Wacc = Wm;
            ban = 0;
        } else if (!test) {
            // 8. the longest step towards zeta that keeps the multipliers of the inequalities non-negative
            const bool out = inS && ineq && zeta <= 0.0;
            const double al = out ? mu / (mu - zeta) : LE_INF;
            const double amin = le_wave_min(al);
            const unsigned long long blk = __ballot(out && al == amin && al < LE_INF);
            if (blk) {                        // (none: a NaN in zeta; nothing moves and the count ends the loop)
                const int kv = __ffsll((long long) blk) - 1;
                if (kv == tt) {               // (not in exact arithmetic) nothing moves
                    Wm = Wacc;
                    mu = muacc;
                    ban |= 1ull << tt;
                    test = true;
                } else {
                    if (inS) mu = mu + amin * (zeta - mu);
                    const unsigned long long leave = __ballot(inW && ineq && (lane == kv || mu <= 0.0));
                    if (leave & lbit) mu = 0.0;
                    Wm &= ~leave;
                }
            }
        }
        if (test) {
            // 2. s = G x - h from the untouched G; the most violated row outside the set
            havet = false;
            s = -h;
            for (int j = 0; j < n; ++j) {
                const double gv = con ? Gq[(size_t) j * g.ldg + lane] : 0.0;
                s = fma(gv, qb_bcast(x, j), s);
            }
            const bool cand = ineq && !(Wm & lbit) && !(ban & lbit) && s < 0.0;
            const double best = le_wave_min(cand ? s : 0.0);
            const unsigned long long pick = __ballot(cand && s == best);
            if (!pick) break;                 // (info 0; a NaN in s leaves no candidate)
            tt = __ffsll((long long) pick) - 1;
            if (lane == tt) mu = 0.0;
            havet = pend = true;
        }
        if (it == maxit) { info = n + 1; break; }                         // 3.
        ++it;
    }
    // the accepted pair; s and |A x - b| from the untouched G, A and x
    s = -h;
    for (int j = 0; j < n; ++j) {
        const double gv = con ? Gq[(size_t) j * g.ldg + lane] : 0.0;
        s = fma(gv, qb_bcast(x, j), s);
    }
    double rf = row ? Bq[lane] : 0.0;
    for (int j = 0; j < n; ++j) {
        const double av = row ? Aq[(size_t) j * g.lda + lane] : 0.0;
        rf = fma(-av, qb_bcast(x, j), rf);
    }
    const double rss = qb_wave_sum(rf * rf);
    if (var) g.X[q * g.sX + lane] = x;
    if (con) {
        if (g.MU) g.MU[q * g.sMU + lane] = muacc;
        if (g.S) g.S[q * g.sS + lane] = s;
        if (g.state) g.state[q * g.sstate + lane] = (int) ((Wacc >> lane) & 1ull);
    }
    if (lane == 0) {
        if (g.resid) g.resid[q] = sqrt(rss);
        if (g.iter) g.iter[q] = it;
        g.info[q] = info;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// workgroup route.  LDS: As[c * ld + i] = [A~2 | A~1 | r] (n + 1 columns, ld = qb_ld(m); column 0 also takes b - A x at the end);
// Cs[c * ldn + i] = the factors of G_S^T (at most n + 1 columns, ldn = qb_ld(n)); ys (h_S, then [y1 ; y2], then x_c), xs (the accepted x),
// gs (g, then lambda; c in the dependence step) and the row map (n + 1 ints), n doubles each; mus, mua (the accepted mu), zet, sv, hs (mg
// each); red[4]; eight words (the action, p, whether t rides, info, iter, whether t was dependent, the accepted set in two); tc[64]
// ---------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr size_t le_wg_doubles(int m, int n, int mg)
{
    return (size_t) (n + 1) * qb_ld(m) + (size_t) (n + 1) * qb_ld(n) + 5 * (size_t) mg + 4 * (size_t) n + QB_WG_SMALL;
}

enum { LE_TEST = 1, LE_CAND, LE_WRITE, LE_INFO };

// thread 0: the row map of W, t last where it rides; returns p
__device__ __forceinline__ int le_wg_map(unsigned long long Wm, bool havet, int tt, int* map)
{
    int p = 0;
    while (Wm) {
        map[p++] = __ffsll((long long) Wm) - 1;
        Wm &= Wm - 1ull;
    }
    if (havet) map[p++] = tt;
    return p;
}

__global__ void __launch_bounds__(256) le_wg_kernel(const qrd_le_args g)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const int m = g.m, n = g.n, mg = g.mg, neq = g.neq, maxit = g.maxit;
    const int ld = qb_ld(m), ldn = qb_ld(n);
    double* As = sm;
    double* Cs = As + (size_t) (n + 1) * ld;
    double* ys = Cs + (size_t) (n + 1) * ldn;
    double* xs = ys + n;
    double* gs = xs + n;
    int* map = (int*) (gs + n);               // (n + 1 ints take at most n doubles)
    double* mus = gs + 2 * n;
    double* mua = mus + mg;
    double* zet = mua + mg;
    double* sv = zet + mg;
    double* hs = sv + mg;
    double* red = hs + mg;
    int* words = (int*) (red + 4);
    int *sact = words, *sp = words + 1, *sht = words + 2, *sinfo = words + 3, *siter = words + 4, *sdep = words + 5;
    unsigned* sacc = (unsigned*) (words + 6);
    double* tc = red + 8;
    const double* Aq = g.A + q * g.sA;
    const double* Bq = g.B + q * g.sB;
    const double* Gq = g.G + q * g.sG;
    const double* Hq = g.H + q * g.sH;
    // what only thread 0 reads and writes
    unsigned long long Wm = neq >= 64 ? ~0ull : (1ull << neq) - 1ull, Wacc = Wm, ban = 0;
    int it = 1, tt = 0;
    bool pend = false, ht = false;
    for (int i = t; i < mg; i += 256) {
        hs[i] = Hq[i];
        mus[i] = mua[i] = zet[i] = sv[i] = 0.0;
    }
    for (int j = t; j < n; j += 256) xs[j] = 0.0;
    if (t == 0) {
        *sp = le_wg_map(Wm, false, 0, map);
        *sht = 0;
        *sinfo = 0;
        *sdep = 0;
        *sact = LE_CAND;
    }
    // every action ends in a decision of thread 0; a candidate is followed by a test or a candidate, a test by a candidate or the end: at
    // most 2 maxit + 3 actions
    for (int guard = 0; guard < 2 * maxit + 4; ++guard) {
        __syncthreads();                      // (thread 0's decision is written; the LDS of the last action is read no more)
        const int act = *sact;                // the same word in every thread: the branches below are taken by all 256 or by none
        const int p = *sp, havet = *sht, k = n - p, pw = p - havet;
        if (act == LE_INFO) {                 // (all or nothing: nothing else is written)
            if (t == 0) g.info[q] = *sinfo;
            return;
        }
        if (act == LE_TEST || act == LE_WRITE) {
            // s = G x - h from the untouched G
            for (int i = t; i < mg; i += 256) {
                double s = -hs[i];
                for (int j = 0; j < n; ++j) s = fma(Gq[(size_t) j * g.ldg + i], xs[j], s);
                sv[i] = s;
            }
            if (act == LE_WRITE) {
                // the accepted pair and |A x - b| from the untouched A
                double ss = 0.0;
                for (int i = t; i < m; i += 256) {
                    double rf = Bq[i];
                    for (int j = 0; j < n; ++j) rf = fma(-Aq[(size_t) j * g.lda + i], xs[j], rf);
                    ss = fma(rf, rf, ss);
                }
                ss = qb_wave_sum(ss);
                if (lane == 0) red[wv] = ss;
                __syncthreads();
                const unsigned long long wa = ((unsigned long long) sacc[1] << 32) | sacc[0];
                for (int j = t; j < n; j += 256) g.X[q * g.sX + j] = xs[j];
                for (int i = t; i < mg; i += 256) {
                    if (g.MU) g.MU[q * g.sMU + i] = mua[i];
                    if (g.S) g.S[q * g.sS + i] = sv[i];
                    if (g.state) g.state[q * g.sstate + i] = (int) ((wa >> i) & 1ull);
                }
                if (t == 0) {
                    if (g.resid) g.resid[q] = sqrt(((red[0] + red[1]) + red[2]) + red[3]);
                    if (g.iter) g.iter[q] = *siter;
                    g.info[q] = *sinfo;
                }
                return;
            }
            __syncthreads();
            if (t == 0) {
                // 2. the most violated row outside the set; ties to the smallest index
                int best = -1;
                double bs = 0.0;
                for (int i = neq; i < mg; ++i) {
                    if (((Wm >> i) & 1ull) || ((ban >> i) & 1ull)) continue;
                    if (sv[i] < bs) { bs = sv[i]; best = i; }
                }
                *siter = it;
                sacc[0] = (unsigned) Wacc;
                sacc[1] = (unsigned) (Wacc >> 32);
                if (best < 0) {
                    *sinfo = 0;
                    *sact = LE_WRITE;
                } else if (it == maxit) {     // 3.
                    *sinfo = n + 1;
                    *sact = LE_WRITE;
                } else {
                    ++it;
                    tt = best;
                    mus[tt] = 0.0;
                    ht = pend = true;
                    *sp = le_wg_map(Wm, true, tt, map);
                    *sht = 1;
                    *sact = LE_CAND;
                }
            }
            continue;
        }
        // act == LE_CAND
        if (p > 0) {
            // row i of G_S^T is column i of G through the row map: the image is written transposed
            for (int i = wv; i < n; i += 4) {
                const double* src = Gq + (size_t) i * g.ldg;
                for (int c = lane; c < p; c += 64) Cs[c * ldn + i] = src[map[c]];
            }
            __syncthreads();
            for (int j = 0; j < pw; ++j) {
                const double tj = qb_wg_col(Cs, ldn, n, j, p, red, t);
                if (t == 0) tc[j] = tj;
                __syncthreads();              // (red and column j are read no more)
            }
            if (havet) {
                if (t == 0) {
                    // 4. what is left of t's column below the rows of W
                    const double* col = Cs + (size_t) pw * ldn;
                    double gn = 0.0, rho = 0.0;
                    for (int j = 0; j < n; ++j) {
                        const double v = Gq[(size_t) j * g.ldg + tt];
                        gn = fma(v, v, gn);
                    }
                    for (int j = pw; j < n; ++j) rho = fma(col[j], col[j], rho);
                    const bool dep = pw == n || sqrt(rho) <= g.rcond * sqrt(gn);
                    *sdep = dep ? 1 : 0;
                    if (dep) {
                        for (int c = 0; c < pw; ++c) gs[c] = col[c];
                        qb_trsv(Cs, ldn, pw, gs);
                        int kv = -1;
                        double theta = LE_INF;
                        for (int c = 0; c < pw; ++c) {
                            const int i = map[c];
                            if (i >= neq && gs[c] > 0.0) {
                                const double r = mus[i] / gs[c];
                                if (r < theta) { theta = r; kv = i; }
                            }
                        }
                        if (kv < 0) {         // (infeasible)
                            *sinfo = -2;
                            *sact = LE_INFO;
                        } else {
                            for (int c = 0; c < pw; ++c) mus[map[c]] = mus[map[c]] - theta * gs[c];
                            mus[tt] = mus[tt] + theta;
                            for (int c = 0; c < pw; ++c) {
                                const int i = map[c];
                                if (i >= neq && (i == kv || mus[i] <= 0.0)) {
                                    mus[i] = 0.0;
                                    Wm &= ~(1ull << i);
                                }
                            }
                            pend = false;
                            if (it == maxit) {                            // 3.
                                *siter = it;
                                *sinfo = n + 1;
                                sacc[0] = (unsigned) Wacc;
                                sacc[1] = (unsigned) (Wacc >> 32);
                                *sact = LE_WRITE;
                            } else {
                                ++it;
                                *sp = le_wg_map(Wm, true, tt, map);
                            }
                        }
                    }
                }
                __syncthreads();
                if (*sdep) continue;          // (the same word in every thread)
                const double tj = qb_wg_col(Cs, ldn, n, pw, p, red, t);
                if (t == 0) tc[pw] = tj;
                __syncthreads();              // (red and column pw are read no more)
            }
            if (t == 0) {
                const int ic = qb_info_serial(Cs, ldn, p);
                if (ic) {
                    *sinfo = -3;
                    *sact = LE_INFO;
                } else {
                    for (int c = 0; c < p; ++c) ys[c] = hs[map[c]];
                    qb_trsv_t(Cs, ldn, p, ys);                            // R_c^T y1 = h_S
                }
            }
            __syncthreads();
            if (*sact == LE_INFO) continue;   // (the same word in every thread)
        }
        for (int c = wv; c <= n; c += 4) {
            const double* src = c < n ? Aq + (size_t) le_src(c, k, p) * g.lda : Bq;
            for (int i = lane; i < m; i += 64) As[c * ld + i] = src[i];
        }
        __syncthreads();
        // a thread per row: row <- row H_0 .. H_{p-1}, each sum over A's columns j .. n-1 ascending
        for (int r = t; r < m; r += 256) {
            double* ar = As + r;
            for (int j = 0; j < p; ++j) {
                const double tj = tc[j];
                if (tj == 0.0) continue;      // (H = I)
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
        // r = b - A~1 y1
        if (p > 0) {
            for (int r = t; r < m; r += 256) {
                double s = As[n * ld + r];
                for (int i = 0; i < p; ++i) s = fma(-As[(k + i) * ld + r], ys[i], s);
                As[n * ld + r] = s;
            }
        }
        __syncthreads();
        // the column step on A~2; A~1 and r ride along
        for (int j = 0; j < k; ++j) {
            qb_wg_col(As, ld, m, j, n + 1, red, t);
            __syncthreads();                  // (red and column j are read no more)
        }
        if (t == 0) {
            const int ia = qb_info_serial(As, ld, k);
            if (ia) {
                *sinfo = ia;
                *sact = LE_INFO;
            }
        }
        __syncthreads();
        if (*sact == LE_INFO) continue;       // (the same word in every thread)
        // wave wv takes the sums g_i, i < p, over rows >= n - p
        {
            const double* tcol = As + n * ld;
            for (int i = wv; i < p; i += 4) {
                const double* gcol = As + (k + i) * ld;
                double s = 0.0;
                for (int r = k + lane; r < m; r += 64) s = fma(gcol[r], tcol[r], s);
                s = qb_wave_sum(s);
                if (lane == 0) gs[i] = s;
            }
        }
        // R_a y2 = t(0 : n-p) (rows < n - p: none of them is read above)
        if (t == 0) {
            double* tcol = As + n * ld;
            qb_trsv(As, ld, k, tcol);
            for (int r = 0; r < k; ++r) ys[p + r] = tcol[r];
        }
        __syncthreads();
        if (t == 0 && p > 0) qb_trsv(Cs, ldn, p, gs);                      // R_c lambda = g
        // x_c = Q_c [y1 ; y2]
        if (wv == 0) {
            for (int j = p - 1; j >= 0; --j) {
                const double tj = tc[j];
                if (tj == 0.0) continue;      // (H = I; wave-uniform)
                qb_col_reflect(Cs + j * ldn, ys, j, n, tj, lane);
                QB_WAVE_SYNC();               // (the next reflector reads the column under another lane map)
            }
        }
        __syncthreads();
        if (t == 0) {
            for (int c = 0; c < p; ++c) zet[map[c]] = -gs[c];
            bool accept = !ht, test = !ht;    // 1. the start is accepted as it is
            if (ht) {
                // 6. the row just taken must come out with a positive multiplier
                if (pend) {
                    pend = false;
                    if (zet[tt] <= 0.0) {
                        ban |= 1ull << tt;
                        mus[tt] = 0.0;
                        test = true;
                    }
                }
                // 7. accept
                if (!test) {
                    bool ok = true;
                    for (int c = 0; c < p; ++c) ok = ok && (map[c] < neq || zet[map[c]] > 0.0);
                    accept = test = ok;
                }
            }
            if (accept) {
                if (ht) Wm |= 1ull << tt;
                for (int i = 0; i < mg; ++i) mus[i] = 0.0;
                for (int c = 0; c < p; ++c) mus[map[c]] = zet[map[c]];
                for (int i = 0; i < mg; ++i) mua[i] = mus[i];
                for (int j = 0; j < n; ++j) xs[j] = ys[j];
                Wacc = Wm;
                ban = 0;
            } else if (!test) {
                // 8. the longest step towards zeta that keeps the multipliers of the inequalities non-negative
                int kv = -1;
                double amin = LE_INF;
                for (int c = 0; c < p; ++c) {
                    const int i = map[c];
                    if (i < neq || !(zet[i] <= 0.0)) continue;
                    const double al = mus[i] / (mus[i] - zet[i]);
                    if (al < amin || (al == amin && i < kv)) { amin = al; kv = i; }          // (t comes last in the map: ties to the smallest index)
                }
                if (kv >= 0) {                // (none: a NaN in zeta; nothing moves and the count ends the loop)
                    if (kv == tt) {           // (not in exact arithmetic) nothing moves
                        Wm = Wacc;
                        for (int i = 0; i < mg; ++i) mus[i] = mua[i];
                        ban |= 1ull << tt;
                        test = true;
                    } else {
                        for (int c = 0; c < p; ++c) {
                            const int i = map[c];
                            mus[i] = mus[i] + amin * (zet[i] - mus[i]);
                        }
                        for (int c = 0; c < pw; ++c) {
                            const int i = map[c];
                            if (i >= neq && (i == kv || mus[i] <= 0.0)) {
                                mus[i] = 0.0;
                                Wm &= ~(1ull << i);
                            }
                        }
                    }
                }
            }
            if (test) {
                ht = false;
                *sht = 0;
                *sact = LE_TEST;
            } else if (it == maxit) {         // 3.
                *siter = it;
                *sinfo = n + 1;
                sacc[0] = (unsigned) Wacc;
                sacc[1] = (unsigned) (Wacc >> 32);
                *sact = LE_WRITE;
            } else {
                ++it;
                *sp = le_wg_map(Wm, true, tt, map);
            }
        }
    }
}

// the kernel that may ask for more than 64 KiB of LDS (qr_allow_lds)
static int le_allow_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(le_wg_kernel)};
    return qr_allow_lds(fns, QB_LDS_CAP, done);
}

template <int W>
static void le_launch_wave(hipStream_t s, const qrd_le_args& a)
{
    const size_t lds = sizeof(double) * 4 * (W * (W + 1) + (W + 1) + W);
    hipLaunchKernelGGL(le_wave_kernel<W>, dim3((unsigned) (((size_t) a.batch + 3) / 4)), dim3(256), lds, s, a);
}

extern "C" {

int qrd_le_wave_route(int m, int n) { return m <= 64 && n + 1 <= 32; }

// the largest m the kernels take for n unknowns and mg constraints; 0: (n, mg) is not taken at all.  The wave route needs no more than the
// workgroup route holds (64 rows of at most 32 columns), so the workgroup route's LDS budget decides.
int qrd_le_max_rows(int n, int mg)
{
    if (n < 1 || n > QRD_B_MAX_N - 1 || mg < 1 || mg > 64) return 0;
    int m = QRD_B_MAX_ROWS;
    while (m >= 1 && sizeof(double) * le_wg_doubles(m, n, mg) > QB_LDS_CAP) --m;
    return m >= 1 ? m : 0;
}

int qrd_le_solve(void* stream, const qrd_le_args* a)
{
    if (!a) return -7;
    if (a->batch <= 0) return 0;
    const int mr = qrd_le_max_rows(a->n, a->mg);
    if (!mr || a->m < 1 || a->m > mr || a->neq < 0 || a->neq > a->n || a->neq > a->mg || a->m + a->neq < a->n || a->lda < a->m || a->ldg < a->mg ||
        a->maxit < 1 || !(a->rcond > 0.0) || !a->A || !a->B || !a->G || !a->H || !a->X || !a->info)
        return -7;
    hipStream_t s = (hipStream_t) stream;
    if (qrd_le_wave_route(a->m, a->n)) {
        if (a->n + 1 <= 8) le_launch_wave<8>(s, *a);
        else if (a->n + 1 <= 16) le_launch_wave<16>(s, *a);
        else le_launch_wave<32>(s, *a);
    } else {
        const int rc = le_allow_lds();
        if (rc) return rc;
        hipLaunchKernelGGL(le_wg_kernel, dim3((unsigned) a->batch), dim3(256), sizeof(double) * le_wg_doubles(a->m, a->n, a->mg), s, *a);
    }
    return (int) hipGetLastError();
}

}   // extern "C"
