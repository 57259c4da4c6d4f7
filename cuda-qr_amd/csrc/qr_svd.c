/* qr_svd.c -- singular values, SVD and minimum-norm least squares of rank-deficient systems (mi355x_qr.h section 7).
 *
 *   qr_jsvd_rounds / qr_jsvd_round_pairs   the round-robin tournament over column blocks (pure host code; the device runs exactly these pairs)
 *   qr_gesvj_dev     LAPACK dgesvj: one launch per round (qrd_jsvd_round), the sweep's convergence word read once per sweep, then column
 *                    norms, a stable descending sort on the host (n doubles in, n ints out), columns permuted in place, normalised
 *   qr_gesvd_dev     geqrf -> R^T -> the same iteration -> V = the normalised iterate, U = Q [Z ; 0] through qr_ormqr_dev('N')
 *   qr_cond_dev      sigma_max / sigma_min through the values-only path
 *   qr_gelss_dev     geqrf -> ormqr('T') -> iteration with accumulation -> X = Y S^+ (Z^T c) on qrd_gemm_tn / qrd_gemm_nn
 *   qr_svd, qr_lstsq_svd   the same on host pointers, through the plan cache of the host-pointer entry points (qr_host.c)
 *
 * Kept out of qr_host.c for the reason qr_solve.c is: the stub device layer of the sanitizer builds has none of the launch wrappers
 * called here. */
#define _POSIX_C_SOURCE 200809L
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355x_qr.h"
#include "qr_device.h"
#include "qr_plan_internal.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

#if QR_JSVD_BLOCK != QRD_JSVD_BLOCK
#error "the public block width and the kernels' disagree"
#endif

int qr_jsvd_rounds(int n, int* nblk, int* rounds)
{
    if (n < 1) return QR_E_ARG;
    const int nb = (n + QR_JSVD_BLOCK - 1) / QR_JSVD_BLOCK;
    if (nblk) *nblk = nb;
    if (rounds) *rounds = nb == 1 ? 1 : ((nb & 1) ? nb : nb - 1);
    return 0;
}

/* pairs per round: the same in every round of a sweep */
static int pairs_per_round(int nb) { return nb == 1 ? 1 : nb / 2; }

int qr_jsvd_round_pairs(int n, int round, int* pairs, int cap)
{
    int nb = 0, rounds = 0;
    if (qr_jsvd_rounds(n, &nb, &rounds) || !pairs || round < 0 || round >= rounds || cap < pairs_per_round(nb)) return QR_E_ARG;
    if (nb == 1) {
        pairs[0] = 0; pairs[1] = 0;
        return 1;
    }
    const int N = (nb & 1) ? nb : nb - 1;       /* the blocks on the circle; an even count leaves block nb - 1 in the middle */
    int c = 0;
    if (!(nb & 1)) { pairs[0] = round; pairs[1] = nb - 1; c = 1; }
    for (int k = 1; k <= (N - 1) / 2; ++k, ++c) {
        const int a = (round + k) % N, b = (round - k + N) % N;
        pairs[2 * c] = a < b ? a : b;
        pairs[2 * c + 1] = a < b ? b : a;
    }
    return c;
}

typedef struct jsvd_ws {
    double *W, *Z, *sig, *sval, *slots, *word;
    int *pairs, *perm;              /* device */
    int *hpairs, *hperm;            /* host */
} jsvd_ws;

static size_t max_pairs(int n)
{
    const size_t nb = ((size_t) n + QR_JSVD_BLOCK - 1) / QR_JSVD_BLOCK;
    return nb == 1 ? 1 : nb * (nb - 1) / 2;
}

/* the plan's workspace, allocated on the first call (sized for the plan's n) */
static int jsvd_workspace(qr_plan* p, jsvd_ws* w)
{
    const size_t n = (size_t) p->n, np = max_pairs(p->n);
    if (!p->sv_d) {
        CHECK(qr_plan_sync(p));
        CHECK(qrd_malloc((void**) &p->sv_d, sizeof(double) * (2 * n * n + 2 * n + np + 1)));
    }
    if (!p->sv_i) CHECK(qrd_malloc((void**) &p->sv_i, sizeof(int) * (2 * np + n)));
    if (!p->sv_h) {
        p->sv_h = (int*) malloc(sizeof(int) * (2 * np + n));
        if (!p->sv_h) return QR_E_ALLOC;
    }
    w->W = p->sv_d; w->Z = w->W + n * n; w->sig = w->Z + n * n; w->sval = w->sig + n; w->slots = w->sval + n; w->word = w->slots + np;
    w->pairs = p->sv_i; w->perm = w->pairs + 2 * np;
    w->hpairs = p->sv_h; w->hperm = w->hpairs + 2 * np;
    return 0;
}

typedef struct sv_key { double s; int i; } sv_key;
static int sv_desc(const void* a, const void* b)
{
    const sv_key *x = (const sv_key*) a, *y = (const sv_key*) b;
    if (x->s != y->s) return x->s > y->s ? -1 : 1;
    return x->i - y->i;                         /* ties keep column order */
}

/* The iteration on G (r x n, ldg) and what follows it.  Z (n x n, ldz; NULL: none) must hold the identity (or whatever the rotations are
 * to be applied to) on entry.  vecs != 0: the columns of G are permuted into descending order and normalised; else G is left as the
 * iteration left it (values only).  hS (n host doubles, may be NULL) receives the sorted values. */
static int jsvd_core(qr_plan* p, const jsvd_ws* w, double* G, int r, int n, int ldg, double* dS, double* Z, int ldz, int vecs, int* sweeps,
                     double* hS)
{
    void* s = p->stream;
    int nb = 0, rounds = 0;
    CHECK(qr_jsvd_rounds(n, &nb, &rounds));
    const int ppr = pairs_per_round(nb), total = ppr * rounds;
    for (int rd = 0; rd < rounds; ++rd)
        if (qr_jsvd_round_pairs(n, rd, w->hpairs + 2 * ppr * rd, ppr) != ppr) return QR_E_INTERNAL;
    CHECK(qrd_h2d(s, w->pairs, w->hpairs, sizeof(int) * 2 * (size_t) total));
    const double tol = sqrt((double) r) * DBL_EPSILON;
    int sw = 0, done = 0;
    while (!done && sw < QR_JSVD_MAX_SWEEPS) {
        ++sw;
        for (int rd = 0; rd < rounds; ++rd)
            CHECK(qrd_jsvd_round(s, G, ldg, r, n, Z, ldz, w->pairs + 2 * ppr * rd, ppr, tol, w->slots + ppr * rd));
        CHECK(qrd_jsvd_fold(s, w->slots, total, w->word));
        double worst = 0.0;
        CHECK(qrd_d2h(s, &worst, w->word, sizeof worst));
        CHECK(qrd_stream_sync(s));
        done = !(worst > tol);                  /* every pair was at or below the threshold before it was touched: nothing rotated */
    }
    if (sweeps) *sweeps = sw;
    if (!done) return QR_E_NOCONV;

    CHECK(qrd_jsvd_colnorms(s, G, ldg, r, n, w->sig));
    sv_key* key = (sv_key*) malloc(sizeof(sv_key) * (size_t) n);
    double* hs = (double*) malloc(sizeof(double) * (size_t) n);
    int rc = (key && hs) ? 0 : QR_E_ALLOC;
    if (!rc) rc = qrd_d2h(s, hs, w->sig, sizeof(double) * (size_t) n);
    if (!rc) rc = qrd_stream_sync(s);
    int moved = 0;
    if (!rc) {
        for (int i = 0; i < n; ++i) { key[i].s = hs[i]; key[i].i = i; }
        qsort(key, (size_t) n, sizeof(sv_key), sv_desc);
        for (int j = 0; j < n; ++j) {
            w->hperm[j] = key[j].i;
            if (key[j].i != j) moved = 1;
            if (hS) hS[j] = key[j].s;
        }
        /* the first column of every cycle carries the flag: the permute kernel starts a walk there and nowhere else */
        for (int j = 0; j < n; ++j) {
            int k = w->hperm[j], lead = 1;
            for (int guard = 0; guard < n && k != j; ++guard) {
                if (k < j) { lead = 0; break; }
                k = w->hperm[k] & (QRD_JSVD_LEAD - 1);
            }
            if (lead) w->hperm[j] |= QRD_JSVD_LEAD;
        }
        rc = qrd_h2d(s, w->perm, w->hperm, sizeof(int) * (size_t) n);
    }
    free(key);
    free(hs);
    CHECK(rc);
    CHECK(qrd_jsvd_gather(s, w->sig, w->perm, dS, n));
    if (vecs) {
        if (moved) CHECK(qrd_jsvd_permute(s, G, ldg, r, n, w->perm));
        CHECK(qrd_jsvd_normalise(s, G, ldg, r, n, dS));
    }
    if (Z && moved) CHECK(qrd_jsvd_permute(s, Z, ldz, n, n, w->perm));
    return 0;
}

static int job(char c, char yes)
{
    if (c == yes || c == yes + ('a' - 'A')) return 1;
    return (c == 'N' || c == 'n') ? 0 : -1;
}

int qr_gesvj_dev(qr_plan* p, char jobv, double* dG, int r, int n, int ldg, double* dS, double* dV, int ldv, int* sweeps)
{
    const int jv = job(jobv, 'V');
    if (!p || jv < 0 || !dG || !dS || n < 1 || r < n || r > p->m || n > p->n || ldg < r || (jv && (!dV || ldv < n))) return QR_E_ARG;
    jsvd_ws w;
    CHECK(jsvd_workspace(p, &w));
    if (jv) CHECK(qrd_set_identity(p->stream, dV, ldv, n, n, 0));
    return jsvd_core(p, &w, dG, r, n, ldg, dS, jv ? dV : NULL, ldv, 1, sweeps, NULL);
}

/* factor dA, R^T into the workspace, the iteration on it: W = Y (normalised, when vecs), Z = the rotations (when accumulate) */
static int rt_svd(qr_plan* p, const jsvd_ws* w, double* dA, int m, int n, int lda, double* dtau, double* dS, int accumulate, int vecs, int* sweeps,
                  double* hS)
{
    CHECK(qr_geqrf_dev(p, dA, m, n, lda, dtau));
    CHECK(qrd_jsvd_rt(p->stream, dA, lda, n, w->W, n));
    if (accumulate) CHECK(qrd_set_identity(p->stream, w->Z, n, n, n, 0));
    return jsvd_core(p, w, w->W, n, n, n, dS, accumulate ? w->Z : NULL, n, vecs, sweeps, hS);
}

int qr_gesvd_dev(qr_plan* p, char jobu, char jobv, double* dA, int m, int n, int lda, double* dtau, double* dS, double* dU, int ldu,
                 double* dV, int ldv, int* sweeps)
{
    const int ju = job(jobu, 'U'), jv = job(jobv, 'V');
    if (!p || ju < 0 || jv < 0 || !dA || !dtau || !dS || n < 1 || m < n || m > p->m || n > p->n || lda < m || (ju && (!dU || ldu < m)) ||
        (jv && (!dV || ldv < n)))
        return QR_E_ARG;
    jsvd_ws w;
    CHECK(jsvd_workspace(p, &w));
    CHECK(rt_svd(p, &w, dA, m, n, lda, dtau, dS, ju, jv, sweeps, NULL));
    if (jv) CHECK(qrd_copy_block(p->stream, w.W, n, dV, ldv, n, n));
    if (ju) {
        CHECK(qrd_copy_block(p->stream, w.Z, n, dU, ldu, n, n));
        CHECK(qrd_zero_block(p->stream, dU + n, ldu, m - n, n));
        CHECK(qr_ormqr_dev(p, 'N', dA, m, n, lda, dtau, NULL, 0, dU, n, ldu));
    }
    return 0;
}

int qr_cond_dev(qr_plan* p, double* dA, int m, int n, int lda, double* dtau, double* cond)
{
    if (!p || !dA || !dtau || !cond || n < 1 || m < n || m > p->m || n > p->n || lda < m) return QR_E_ARG;
    jsvd_ws w;
    CHECK(jsvd_workspace(p, &w));
    double* hs = (double*) malloc(sizeof(double) * 2 * (size_t) n);
    if (!hs) return QR_E_ALLOC;
    double* diag = hs + n;
    int rc = rt_svd(p, &w, dA, m, n, lda, dtau, w.sval, 0, 0, NULL, hs);
    if (!rc) rc = qrd_d2h_2d(p->stream, diag, sizeof(double), dA, sizeof(double) * ((size_t) lda + 1), sizeof(double), (size_t) n);
    const int rs = qr_plan_sync(p);
    if (!rc) rc = rs;
    /* a triangle with an exactly zero diagonal entry is exactly singular (qr_lstsq's test): the iteration would return rounding noise for
     * that zero, 1e-24 rather than 0 */
    int singular = 0;
    for (int i = 0; !rc && i < n; ++i)
        if (diag[i] == 0.0) singular = 1;
    if (!rc) *cond = (!singular && hs[n - 1] > 0.0) ? hs[0] / hs[n - 1] : INFINITY;
    free(hs);
    return rc;
}

/* Z^T c and its scaled copy: 2 n nrhs doubles, grown before anything of the call is queued */
static int gelss_workspace(qr_plan* p, int n, int nrhs)
{
    const size_t need = 2 * (size_t) n * nrhs;
    if (need <= p->sv_t_cap) return 0;
    CHECK(qr_plan_sync(p));
    qrd_free(p->sv_t);
    p->sv_t = NULL; p->sv_t_cap = 0;
    CHECK(qrd_malloc((void**) &p->sv_t, sizeof(double) * need));
    p->sv_t_cap = need;
    return 0;
}

/* hS: n host doubles (the sorted values); on return p->sv_t holds Z^T c (n x nrhs), unscaled */
static int gelss_core(qr_plan* p, double* dA, int m, int n, int lda, double* dtau, double* dB, int nrhs, int ldb, double rcond, double* dS,
                      int* rank, double* hS)
{
    jsvd_ws w;
    CHECK(jsvd_workspace(p, &w));
    CHECK(gelss_workspace(p, n, nrhs));
    CHECK(rt_svd(p, &w, dA, m, n, lda, dtau, dS, 1, 1, NULL, hS));
    CHECK(qr_ormqr_dev(p, 'T', dA, m, n, lda, dtau, NULL, 0, dB, nrhs, ldb));
    const double rc = rcond < 0.0 ? (double) (m > n ? m : n) * DBL_EPSILON : rcond;
    double *T1 = p->sv_t, *T2 = T1 + (size_t) n * nrhs;
    CHECK(qrd_gemm_tn(p->stream, n, nrhs, n, 1.0, w.Z, n, dB, ldb, 0.0, T1, n, p->slabs, p->slab_cap, NULL, 0));
    CHECK(qrd_jsvd_pinv_scale(p->stream, T1, T2, n, nrhs, dS, rc));
    CHECK(qrd_gemm_nn(p->stream, n, nrhs, n, 1.0, w.W, n, T2, n, 0.0, dB, ldb));
    int r = 0;
    for (int i = 0; i < n; ++i)
        if (hS[i] > rc * hS[0]) ++r;
    if (rank) *rank = r;
    return 0;
}

int qr_gelss_dev(qr_plan* p, double* dA, int m, int n, int lda, double* dtau, double* dB, int nrhs, int ldb, double rcond, double* dS, int* rank)
{
    if (!p || !dA || !dtau || !dB || !dS || n < 1 || m < n || m > p->m || n > p->n || lda < m || nrhs < 1 || ldb < m) return QR_E_ARG;
    double* hs = (double*) malloc(sizeof(double) * (size_t) n);
    if (!hs) return QR_E_ALLOC;
    const int rc = gelss_core(p, dA, m, n, lda, dtau, dB, nrhs, ldb, rcond, dS, rank, hs);
    free(hs);
    return rc;
}

int qr_svd(const double* A, int m, int n, double* S, double* U, double* V)
{
    if (!A || !S || n < 1 || m < n) return QR_E_ARG;
    host_slot priv, *sl = NULL;
    CHECK(qr_host_slot_acquire(m, n, &priv, &sl));
    qr_plan* p = sl->p;
    const int latch0 = p->guard_latch;
    p->guard_latch = 0;                    /* a blocking entry point: a refused tall panel goes to the leaf chain (as in qr_lstsq) */
    const size_t nn = (size_t) n * n;
    int rc = U ? qr_host_slot_need(&sl->dQ, &sl->q_cap, (size_t) m * n) : 0;
    if (!rc) rc = qr_host_slot_need(&sl->dR, &sl->r_cap, nn + (size_t) n);
    double *dV = sl->dR, *dS = rc ? NULL : sl->dR + nn;
    if (!rc) rc = qrd_h2d(p->stream, sl->dA, A, sizeof(double) * (size_t) m * n);
    if (!rc) rc = qr_gesvd_dev(p, U ? 'U' : 'N', V ? 'V' : 'N', sl->dA, m, n, m, sl->dtau, dS, U ? sl->dQ : NULL, m, V ? dV : NULL, n, NULL);
    if (!rc) rc = qrd_d2h(p->stream, S, dS, sizeof(double) * (size_t) n);
    if (!rc && U) rc = qrd_d2h(p->stream, U, sl->dQ, sizeof(double) * (size_t) m * n);
    if (!rc && V) rc = qrd_d2h(p->stream, V, dV, sizeof(double) * nn);
    const int rs = qr_plan_sync(p);
    if (!rc) rc = rs;
    p->guard_latch = latch0;
    qr_host_slot_release(sl);
    return rc;
}

int qr_lstsq_svd(const double* A, int m, int n, const double* B, int nrhs, double rcond, double* X, double* resid, int* rank, double* S)
{
    if (!A || !B || !X || n < 1 || m < n || nrhs < 1) return QR_E_ARG;
    host_slot priv, *sl = NULL;
    CHECK(qr_host_slot_acquire(m, n, &priv, &sl));
    qr_plan* p = sl->p;
    const int latch0 = p->guard_latch;
    p->guard_latch = 0;
    const size_t rows_b = (size_t) m, nz = (size_t) n * nrhs, nt = (size_t) (m - n) * nrhs;
    double* hs = (double*) malloc(sizeof(double) * (size_t) n);
    double* part = resid ? (double*) malloc(sizeof(double) * (nz + nt + 1)) : NULL;      /* Z^T c, then the last m - n rows of Q^T B */
    int rc = (!hs || (resid && !part)) ? QR_E_ALLOC : 0;
    int r = 0;
    if (!rc) rc = qr_host_slot_need(&sl->dQ, &sl->q_cap, rows_b * nrhs);
    if (!rc) rc = qr_host_slot_need(&sl->dR, &sl->r_cap, (size_t) n);
    if (!rc) rc = qrd_h2d(p->stream, sl->dA, A, sizeof(double) * (size_t) m * n);
    if (!rc) rc = qrd_h2d(p->stream, sl->dQ, B, sizeof(double) * rows_b * nrhs);
    if (!rc) rc = gelss_core(p, sl->dA, m, n, m, sl->dtau, sl->dQ, nrhs, m, rcond, sl->dR, &r, hs);
    if (!rc) rc = qrd_d2h_2d(p->stream, X, sizeof(double) * n, sl->dQ, sizeof(double) * rows_b, sizeof(double) * n, nrhs);
    if (!rc && resid) rc = qrd_d2h(p->stream, part, p->sv_t, sizeof(double) * nz);
    if (!rc && resid && m > n)
        rc = qrd_d2h_2d(p->stream, part + nz, sizeof(double) * (m - n), sl->dQ + n, sizeof(double) * rows_b, sizeof(double) * (m - n), nrhs);
    const int rs = qr_plan_sync(p);
    if (!rc) rc = rs;
    p->guard_latch = latch0;
    qr_host_slot_release(sl);
    if (!rc && resid)
        for (int j = 0; j < nrhs; ++j) {
            double scale = 0.0, ssq = 1.0;   /* scaled sum of squares (LAPACK dnrm2), as in qr_lstsq */
            for (size_t i = 0; i < (size_t) (n - r) + (size_t) (m - n); ++i) {
                const double v = fabs(i < (size_t) (n - r) ? part[(size_t) j * n + r + i] : part[nz + (size_t) j * (m - n) + (i - (size_t) (n - r))]);
                if (v == 0.0) continue;
                if (scale < v) { ssq = 1.0 + ssq * (scale / v) * (scale / v); scale = v; }
                else ssq += (v / scale) * (v / scale);
            }
            resid[j] = scale * sqrt(ssq);
        }
    if (!rc && rank) *rank = r;
    if (!rc && S) memcpy(S, hs, sizeof(double) * (size_t) n);
    free(hs);
    free(part);
    return rc;
}
