/* qr_pivot.c -- column-pivoted QR and rank-deficient least squares (mi355x_qr.h section 4).
 *
 *   qr_geqp3_dev      LAPACK dgeqp3 / dlaqps with every column free, panels of QR_PIVOT_PANEL columns: per column three launches
 *                     (qrd_pivot_column: pivot + swap + column update, the trailing matrix-vector product, F / pivot row / norm downdate),
 *                     per panel one block update A22 -= V F^T (qrd_gemm_nt where its predicate allows, else the general product on F^T)
 *                     and the exact recomputation of the norms the downdate flagged.  The factors are laid out as qr_geqrf_dev's.
 *   qr_rank_dev       numerical rank from R's diagonal
 *   qr_gelsp_dev      geqp3 -> rank -> ormqr('T') -> residual norms -> solve_r on the leading r x r block -> scatter by jpvt
 *   qr_lstsq_pivoted  the same on host pointers, through the plan cache of the host-pointer entry points
 *
 * The host reads one word per panel (how many of its columns were factored: a flagged norm ends a panel early, as in dlaqps); nothing
 * inside a panel waits for the device.
 * Kept out of qr_host.c for the reason qr_solve.c is: the stub device layer of the sanitizer builds has no qrd_pivot_* wrapper. */
#define _POSIX_C_SOURCE 200809L
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355x_qr.h"
#include "qr_device.h"
#include "qr_plan_internal.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

static int imin(int a, int b) { return a < b ? a : b; }

/* Panel width 32, from devtools/tools_geqp3_perf.py (profiles/r08_geqp3_perf.txt): 4096^2 takes 150.7 ms at 128, 129.7 at 64, 118.0 at 32;
 * 16384 x 512 24.7 / 21.1 / 19.7.  The in-panel work grows with the column's position in the panel (the column update reads j columns of V,
 * the F correction j columns of F) and costs more than the extra block updates of narrow panels.  Lab builds take MI355XQR_PIVOT_NB
 * (a multiple of 16 up to QRD_PIVOT_NBP) for that measurement. */
#define QR_PIVOT_PANEL 32
static int panel_width(const qr_plan* p)
{
    int w = imin(p->nb, QR_PIVOT_PANEL);
#ifdef QR_LAB
    const char* e = getenv("MI355XQR_PIVOT_NB");
    if (e && atoi(e) >= 16 && atoi(e) <= QRD_PIVOT_NBP && atoi(e) % 16 == 0) w = atoi(e);
#endif
    return w;
}

/* the plan's pivoting workspace, allocated on the first call (sized for the plan's n) */
static int pivot_ws(qr_plan* p, qrd_pivot_ws* w)
{
    if (!p->pv_d) {
        CHECK(qr_plan_sync(p));
        CHECK(qrd_malloc((void**) &p->pv_d, sizeof(double) * qrd_pivot_ws_doubles(p->n)));
    }
    if (!p->pv_i) CHECK(qrd_malloc((void**) &p->pv_i, sizeof(int) * qrd_pivot_ws_ints(p->n)));
    qrd_pivot_ws_bind(w, p->n, p->pv_d, p->pv_i);
    return 0;
}

int qr_geqp3_dev(qr_plan* p, double* dA, int m, int n, int lda, int* djpvt, double* dtau)
{
    if (!p || !dA || !djpvt || !dtau || n < 1 || m < n || m > p->m || n > p->n || lda < m) return QR_E_ARG;
    qrd_pivot_ws w;
    CHECK(pivot_ws(p, &w));
    void* s = p->stream;
    const int nbp = panel_width(p);
    CHECK(qrd_pivot_norms(s, &w, dA, lda, m, n, 0, 0, 1, djpvt));
    for (int k0 = 0; k0 < n;) {
        const int wd = imin(nbp, n - k0);
        for (int j = 0; j < wd; ++j) CHECK(qrd_pivot_column(s, &w, dA, lda, m, n, k0, j, djpvt, dtau));
        int pend = 0;
        CHECK(qrd_d2h(s, &pend, w.pend, sizeof pend));
        CHECK(qrd_stream_sync(s));
        const int jb = imin(wd, pend);
        if (jb < 1) return QR_E_INTERNAL;
        const int k1 = k0 + jb, M = m - k1, N = n - k1;
        if (N > 0) {
            if (M > 0) {      /* A(k1:, k1:) -= V F^T: rows k0 .. k1-1 of the trailing columns were brought up to date column by column */
                const double* V = dA + (size_t) k0 * lda + k1;
                const double* Bt = w.F + k1;
                double* C2 = dA + (size_t) k1 * lda + k1;
                if (qrd_gemm_nt_ok(M, N, jb, V, lda, Bt, w.ldf, C2, lda) || (M % 128 == 0 && qrd_gemm_nt4_ok(M, N, jb, V, lda, Bt, w.ldf, C2, lda)))
                    CHECK(qrd_gemm_nt(s, M, N, jb, -1, V, lda, Bt, w.ldf, C2, lda, -1, NULL));
                else {
                    CHECK(qrd_transpose(s, N, jb, Bt, w.ldf, w.FT, jb));
                    CHECK(qrd_gemm_nn(s, M, N, jb, -1.0, V, lda, w.FT, jb, 1.0, C2, lda));
                }
            }
            CHECK(qrd_pivot_norms(s, &w, dA, lda, m, n, k1, k1, 0, djpvt));
        }
        k0 = k1;
    }
    return 0;
}

/* the number of i with |d[i]| > rcond |d[0]| (rcond < 0: max(m, n) eps) */
static int rank_of_diag(const double* d, int m, int n, double rcond)
{
    const double rc = rcond < 0.0 ? (double) (m > n ? m : n) * DBL_EPSILON : rcond;
    const double thr = rc * fabs(d[0]);
    int r = 0;
    for (int i = 0; i < n; ++i)
        if (fabs(d[i]) > thr) ++r;
    return r;
}

int qr_rank_dev(qr_plan* p, const double* dA, int m, int n, int lda, double rcond, int* rank)
{
    if (!p || !dA || !rank || n < 1 || m < n || m > p->m || n > p->n || lda < m) return QR_E_ARG;
    double* d = (double*) malloc(sizeof(double) * (size_t) n);
    if (!d) return QR_E_ALLOC;
    int rc = qrd_d2h_2d(p->stream, d, sizeof(double), dA, sizeof(double) * ((size_t) lda + 1), sizeof(double), (size_t) n);
    const int rs = qr_plan_sync(p);
    if (!rc) rc = rs;
    if (!rc) *rank = rank_of_diag(d, m, n, rcond);
    free(d);
    return rc;
}

int qr_gelsp_dev(qr_plan* p, double* dA, int m, int n, int lda, int* djpvt, double* dtau, double* dB, int nrhs, int ldb, double rcond,
                 double* dresid, int* rank)
{
    if (!p || !dA || !djpvt || !dtau || !dB || n < 1 || m < n || m > p->m || n > p->n || lda < m || nrhs < 1 || ldb < m) return QR_E_ARG;
    CHECK(qr_geqp3_dev(p, dA, m, n, lda, djpvt, dtau));
    int r = 0;
    CHECK(qr_rank_dev(p, dA, m, n, lda, rcond, &r));
    const size_t need = (size_t) n * nrhs;
    if (need > p->pv_scatter_cap) {
        qrd_free(p->pv_scatter);             /* (the plan is idle: qr_rank_dev has just drained it) */
        p->pv_scatter = NULL; p->pv_scatter_cap = 0;
        CHECK(qrd_malloc((void**) &p->pv_scatter, sizeof(double) * need));
        p->pv_scatter_cap = need;
    }
    CHECK(qr_ormqr_dev(p, 'T', dA, m, n, lda, dtau, NULL, 0, dB, nrhs, ldb));
    if (dresid) CHECK(qrd_pivot_resid(p->stream, dB, ldb, r, m, nrhs, dresid));
    if (r > 0) CHECK(qr_solve_r_dev(p, dA, r, lda, dB, nrhs, ldb));
    CHECK(qrd_pivot_scatter(p->stream, dB, ldb, n, nrhs, r, djpvt, p->pv_scatter));
    CHECK(qrd_copy_block(p->stream, p->pv_scatter, n, dB, ldb, n, nrhs));
    if (rank) *rank = r;
    return 0;
}

int qr_lstsq_pivoted(const double* A, int m, int n, const double* B, int nrhs, double rcond, double* X, double* resid, int* rank, int* jpvt)
{
    if (!A || !B || !X || n < 1 || m < n || nrhs < 1) return QR_E_ARG;
    host_slot priv, *sl = NULL;
    CHECK(qr_host_slot_acquire(m, n, &priv, &sl));
    qr_plan* p = sl->p;
    const size_t rows_b = (size_t) m;
    /* dR of the slot as raw storage: nrhs residual norms, then n pivot indices */
    int rc = qr_host_slot_need(&sl->dQ, &sl->q_cap, rows_b * nrhs);
    if (!rc) rc = qr_host_slot_need(&sl->dR, &sl->r_cap, (size_t) nrhs + ((size_t) n + 1) / 2);
    double* dres = sl->dR;
    int* dj = rc ? NULL : (int*) (sl->dR + nrhs);
    int r = 0;
    if (!rc) rc = qrd_h2d(p->stream, sl->dA, A, sizeof(double) * (size_t) m * n);
    if (!rc) rc = qrd_h2d(p->stream, sl->dQ, B, sizeof(double) * rows_b * nrhs);
    if (!rc) rc = qr_gelsp_dev(p, sl->dA, m, n, m, dj, sl->dtau, sl->dQ, nrhs, m, rcond, dres, &r);
    if (!rc) rc = qrd_d2h_2d(p->stream, X, sizeof(double) * n, sl->dQ, sizeof(double) * rows_b, sizeof(double) * n, nrhs);
    if (!rc && resid) rc = qrd_d2h(p->stream, resid, dres, sizeof(double) * (size_t) nrhs);
    if (!rc && jpvt) rc = qrd_d2h(p->stream, jpvt, dj, sizeof(int) * (size_t) n);
    const int rs = qr_plan_sync(p);
    if (!rc) rc = rs;
    qr_host_slot_release(sl);
    if (!rc && rank) *rank = r;
    return rc;
}
