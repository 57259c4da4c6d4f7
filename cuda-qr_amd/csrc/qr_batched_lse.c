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
#include "qr_stage.h"

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

/* the host-pointer twin: packed batches, staged as qr_stage.h describes */
int qr_lstsq_constrained_batched(const double* A, int m, int n, const double* C, int p, const double* b, const double* d, int nrhs, int batch,
                                 double* X, double* L, double* resid, int* info)
{
    if (!A || !C || !b || !d || !X || !info || batch < 0 || bad_shape(m, n, p, nrhs)) return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t nb = (size_t) batch, mn = (size_t) m * n, pn = (size_t) p * n, mr = (size_t) m * nrhs, pr = (size_t) p * nrhs,
                 nr = (size_t) n * nrhs;
    double *dA, *dC, *dB, *dD, *dX, *dL, *dres;
    int* dinfo;
    /* a member with an info word has nothing written: its X, L and resid read 0 */
    qr_stage_buf t[] = { QR_STAGE_F64(dA, nb * mn, A, NULL, 0), QR_STAGE_F64(dC, nb * pn, C, NULL, 0), QR_STAGE_F64(dB, nb * mr, b, NULL, 0),
                         QR_STAGE_F64(dD, nb * pr, d, NULL, 0), QR_STAGE_F64(dX, nb * nr, NULL, X, 1), QR_STAGE_F64(dL, nb * pr, NULL, L, 1),
                         QR_STAGE_F64(dres, nb * (size_t) nrhs, NULL, resid, 1), QR_STAGE_I32(dinfo, nb, NULL, info, 0) };
    qr_stage st;
    int rc = qr_stage_open(&st, m > n ? m : n, n, t, QR_STAGE_COUNT(t));
    if (!rc)
        rc = qr_gglse_batched_dev(st.plan, dA, m, n, m, (long long) mn, dC, p, p, (long long) pn, dB, m, (long long) mr, dD, p, (long long) pr, nrhs,
                                  dX, n, (long long) nr, L ? dL : NULL, p, (long long) pr, resid ? dres : NULL, nrhs, dinfo, batch);
    rc = qr_stage_fetch(&st, rc);
    if (!rc && qr_stage_any(info, nb)) rc = QR_E_SINGULAR;
    qr_stage_close(&st);
    return rc;
}
