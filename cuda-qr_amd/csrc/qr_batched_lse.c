/* qr_batched_lse.c -- batched equality-constrained least squares, LAPACK dgglse's problem per member (mi355x_qr.h section 8h).
 *
 *   qr_gglse_batched_max_rows      the largest m taken for (n, p, nrhs); no device touched
 *   qr_gglse_batched_dev           min |A x - b| subject to C x = d for every member: one launch of qrd_bl_solve
 *   qr_lstsq_constrained_batched   the same on host pointers, packed batches
 *
 * The plan supplies the stream.  Nothing here waits on the host except the host-pointer twin.
 *
 * Kept out of qr_host.c for the reason qr_solve.c is: the sanitizer and stub builds compile qr_host.c against a stub device layer that
 * has none of the launch wrappers called here. */
#define _POSIX_C_SOURCE 200809L
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355x_qr.h"
#include "qr_device.h"
#include "qr_plan_internal.h"

/* a block of `cols` columns of `rows` rows: columns at least `rows` apart, members at least ld * cols apart */
static int bad_block(int rows, int cols, int ld, long long stride) { return ld < rows || stride < (long long) ld * cols; }

/* 1 <= p <= n, m >= 1, m + p >= n, nrhs >= 1, n + nrhs <= QR_BATCHED_MAX_N, and m rows are held */
static int bad_shape(int m, int n, int p, int nrhs)
{
    if (n < 1 || n > QR_BATCHED_MAX_N || p < 1 || p > n || m < 1 || m < n - p || nrhs < 1 || nrhs > QR_BATCHED_MAX_N - n) return 1;
    return m > qrd_bl_max_rows(n, p, nrhs);
}

int qr_gglse_batched_max_rows(int n, int p, int nrhs) { return qrd_bl_max_rows(n, p, nrhs); }

int qr_gglse_batched_dev(qr_plan* plan, const double* dA, int m, int n, int lda, long long strideA, const double* dC, int p, int ldc,
                         long long strideC, const double* dB, int ldb, long long strideB, const double* dD, int ldd, long long strideD, int nrhs,
                         double* dX, int ldx, long long strideX, double* dL, int ldl, long long strideL, double* dresid, long long strideres,
                         int* dinfo, int batch)
{
    if (!plan || !dA || !dC || !dB || !dD || !dX || !dinfo || batch < 0 || bad_shape(m, n, p, nrhs) || bad_block(m, n, lda, strideA) ||
        bad_block(p, n, ldc, strideC) || bad_block(m, nrhs, ldb, strideB) || bad_block(p, nrhs, ldd, strideD) || bad_block(n, nrhs, ldx, strideX) ||
        (dL && bad_block(p, nrhs, ldl, strideL)) || (dresid && strideres < nrhs))
        return QR_E_ARG;
    if (batch == 0) return 0;
    qrd_bl_args a;
    memset(&a, 0, sizeof a);
    a.A = dA; a.C = dC; a.B = dB; a.D = dD;
    a.X = dX; a.L = dL; a.resid = dresid; a.info = dinfo;
    a.sA = (size_t) strideA; a.sC = (size_t) strideC; a.sB = (size_t) strideB; a.sD = (size_t) strideD; a.sX = (size_t) strideX;
    a.sL = dL ? (size_t) strideL : 0; a.sres = dresid ? (size_t) strideres : 0;
    a.lda = lda; a.ldc = ldc; a.ldb = ldb; a.ldd = ldd; a.ldx = ldx; a.ldl = dL ? ldl : 0;
    a.m = m; a.n = n; a.p = p; a.nrhs = nrhs; a.batch = batch;
    return qrd_bl_solve(plan->stream, &a);
}

/* the host-pointer twin: a plan of its own, one device allocation, packed batches */
int qr_lstsq_constrained_batched(const double* A, int m, int n, const double* C, int p, const double* b, const double* d, int nrhs, int batch,
                                 double* X, double* L, double* resid, int* info)
{
    if (!A || !C || !b || !d || !X || !info || batch < 0 || bad_shape(m, n, p, nrhs)) return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t nb = (size_t) batch, mn = (size_t) m * n, pn = (size_t) p * n, mr = (size_t) m * nrhs, pr = (size_t) p * nrhs,
                 nr = (size_t) n * nrhs;
    qr_plan* plan = NULL;
    int rc = qr_plan_create(&plan, m > n ? m : n, n, 0, 0);
    if (rc) return rc;
    double* dv = NULL;
    int* dinfo = NULL;
    double *dA = NULL, *dC = NULL, *dB = NULL, *dD = NULL, *dX = NULL, *dL = NULL, *dres = NULL;
    rc = qrd_malloc((void**) &dv, sizeof(double) * nb * (mn + pn + mr + pr + nr + pr + (size_t) nrhs));
    if (!rc) { dA = dv; dC = dA + nb * mn; dB = dC + nb * pn; dD = dB + nb * mr; dX = dD + nb * pr; dL = dX + nb * nr; dres = dL + nb * pr; }
    if (!rc) rc = qrd_malloc((void**) &dinfo, sizeof(int) * nb);
    if (!rc) rc = qrd_h2d(plan->stream, dA, A, sizeof(double) * nb * mn);
    if (!rc) rc = qrd_h2d(plan->stream, dC, C, sizeof(double) * nb * pn);
    if (!rc) rc = qrd_h2d(plan->stream, dB, b, sizeof(double) * nb * mr);
    if (!rc) rc = qrd_h2d(plan->stream, dD, d, sizeof(double) * nb * pr);
    /* a member with an info word has nothing written: its X, L and resid read 0 */
    if (!rc) rc = qrd_memset(plan->stream, dX, 0, sizeof(double) * nb * (nr + pr + (size_t) nrhs));
    if (!rc)
        rc = qr_gglse_batched_dev(plan, dA, m, n, m, (long long) mn, dC, p, p, (long long) pn, dB, m, (long long) mr, dD, p, (long long) pr, nrhs,
                                  dX, n, (long long) nr, L ? dL : NULL, p, (long long) pr, resid ? dres : NULL, nrhs, dinfo, batch);
    if (!rc) rc = qrd_d2h(plan->stream, X, dX, sizeof(double) * nb * nr);
    if (!rc && L) rc = qrd_d2h(plan->stream, L, dL, sizeof(double) * nb * pr);
    if (!rc && resid) rc = qrd_d2h(plan->stream, resid, dres, sizeof(double) * nb * (size_t) nrhs);
    if (!rc) rc = qrd_d2h(plan->stream, info, dinfo, sizeof(int) * nb);
    const int rs = qrd_stream_sync(plan->stream);
    if (!rc) rc = rs;
    if (!rc)
        for (size_t q = 0; q < nb; ++q)
            if (info[q]) rc = QR_E_SINGULAR;
    if (dinfo) qrd_free(dinfo);
    if (dv) qrd_free(dv);
    qr_plan_destroy(plan);
    return rc;
}
