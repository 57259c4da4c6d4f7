/* qr_batched_irls.c -- batched robust and weighted least squares, IRLS per member (mi355x_qr.h section 8j).
 *
 *   qr_irls_batched_max_rows        the largest m taken for n unknowns; no device touched
 *   qr_irls_batched_dev             weighted least squares, Huber or bisquare fits of every member: one launch of qrd_ir_solve
 *   qr_gels_weighted_batched_dev    the QR_LOSS_LS case: min sum_i p_i (b - A x)_i^2
 *   qr_lstsq_robust_batched         the same on host pointers, packed batches
 *
 * The plan supplies the stream.  Nothing here waits on the host except the host-pointer twin.
 *
 * Kept out of qr_host.c for the reason qr_solve.c is: the sanitizer and stub builds compile qr_host.c against a stub device layer that
 * has none of the launch wrappers called here. */
#define _POSIX_C_SOURCE 200809L
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355x_qr.h"
#include "qr_device.h"
#include "qr_plan_internal.h"
#include "qr_stage.h"

/* 1 <= n <= 63, m >= n, and m rows are held */
static int bad_shape(int m, int n)
{
    if (n < 1 || n > QR_BATCHED_MAX_N - 1 || m < n) return 1;
    return m > qrd_ir_max_rows(n);
}

/* neither NaN nor inf */
static int finite_value(double v) { return v - v == 0.0; }

/* loss 0..2, tune finite, tol >= 0 (a NaN fails the comparison) */
static int bad_control(int loss, double tune, double tol)
{
    return loss < QR_LOSS_LS || loss > QR_LOSS_BISQUARE || !finite_value(tune) || !(tol >= 0.0);
}

/* tune <= 0: the constants of 95 % efficiency at the normal distribution */
static double tuning(int loss, double tune) { return tune > 0.0 ? tune : (loss == QR_LOSS_BISQUARE ? 4.685 : 1.345); }

/* maxit <= 0: 50; the kernels count passes in an int */
static int iteration_cap(int maxit) { return maxit <= 0 ? 50 : (maxit > INT_MAX / 4 ? INT_MAX / 4 : maxit); }

int qr_irls_batched_max_rows(int n) { return qrd_ir_max_rows(n); }

int qr_irls_batched_dev(qr_plan* plan, int loss, double tune, const double* dA, int m, int n, int lda, long long strideA, const double* dB,
                        long long strideB, const double* dprior, long long strideprior, const double* dscale_in, const double* dX0,
                        long long strideX0, double tol, int maxit, double* dX, long long strideX, double* dW, long long strideW, double* dscale,
                        double* dresid, int* diter, int* dstatus, int* dinfo, int batch)
{
    if (!plan || !dA || !dB || !dX || !dinfo || batch < 0 || bad_control(loss, tune, tol) || bad_shape(m, n) || lda < m ||
        strideA < (long long) lda * n || strideB < m || (strideprior != 0 && strideprior < m) || (dX0 && strideX0 < n) || strideX < n ||
        (dW && strideW < m))
        return QR_E_ARG;
    if (batch == 0) return 0;
    qrd_ir_args a;
    memset(&a, 0, sizeof a);
    a.A = dA; a.B = dB; a.prior = dprior; a.scale_in = dscale_in; a.X0 = dX0;
    a.X = dX; a.W = dW; a.scale = dscale; a.resid = dresid; a.iter = diter; a.status = dstatus; a.info = dinfo;
    a.sA = (size_t) strideA; a.sB = (size_t) strideB; a.sprior = (size_t) strideprior; a.sX0 = dX0 ? (size_t) strideX0 : 0;
    a.sX = (size_t) strideX; a.sW = dW ? (size_t) strideW : 0;
    a.tune = tuning(loss, tune); a.tol = tol;
    a.lda = lda; a.m = m; a.n = n; a.loss = loss; a.maxit = iteration_cap(maxit); a.batch = batch;
    return qrd_ir_solve(plan->stream, &a);
}

int qr_gels_weighted_batched_dev(qr_plan* plan, const double* dA, int m, int n, int lda, long long strideA, const double* dB, long long strideB,
                                 const double* dprior, long long strideprior, double* dX, long long strideX, double* dresid, int* dinfo,
                                 int batch)
{
    return qr_irls_batched_dev(plan, QR_LOSS_LS, 0.0, dA, m, n, lda, strideA, dB, strideB, dprior, strideprior, NULL, NULL, 0, 0.0, 1, dX,
                               strideX, NULL, 0, NULL, dresid, NULL, NULL, dinfo, batch);
}

/* the host-pointer twin: packed batches, staged as qr_stage.h describes */
int qr_lstsq_robust_batched(const double* A, int m, int n, const double* b, int loss, double tune, const double* prior, const double* scale_in,
                            const double* x0, double tol, int maxit, int batch, double* X, double* W, double* scale, double* resid, int* iter,
                            int* status, int* info)
{
    if (!A || !b || !X || !info || batch < 0 || bad_control(loss, tune, tol) || bad_shape(m, n)) return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t nb = (size_t) batch, mn = (size_t) m * n, nn = (size_t) n, mm = (size_t) m;
    double *dA, *dB, *dP, *dS, *dX0, *dX, *dW, *dsc, *dres;
    int *diter, *dstat, *dinfo;
    /* a member with an info word has nothing else written: its X, W, scale, resid, iter and status read 0 */
    qr_stage_buf t[] = { QR_STAGE_F64(dA, nb * mn, A, NULL, 0), QR_STAGE_F64(dB, nb * mm, b, NULL, 0), QR_STAGE_F64(dP, nb * mm, prior, NULL, 0),
                         QR_STAGE_F64(dS, nb, scale_in, NULL, 0), QR_STAGE_F64(dX0, nb * nn, x0, NULL, 0), QR_STAGE_F64(dX, nb * nn, NULL, X, 1),
                         QR_STAGE_F64(dW, nb * mm, NULL, W, 1), QR_STAGE_F64(dsc, nb, NULL, scale, 1), QR_STAGE_F64(dres, nb, NULL, resid, 1),
                         QR_STAGE_I32(diter, nb, NULL, iter, 1), QR_STAGE_I32(dstat, nb, NULL, status, 1), QR_STAGE_I32(dinfo, nb, NULL, info, 0) };
    qr_stage st;
    int rc = qr_stage_open(&st, m, n, t, QR_STAGE_COUNT(t));
    if (!rc)
        rc = qr_irls_batched_dev(st.plan, loss, tune, dA, m, n, m, (long long) mn, dB, m, prior ? dP : NULL, m, scale_in ? dS : NULL,
                                 x0 ? dX0 : NULL, n, tol, maxit, dX, n, W ? dW : NULL, m, scale ? dsc : NULL, resid ? dres : NULL,
                                 iter ? diter : NULL, status ? dstat : NULL, dinfo, batch);
    rc = qr_stage_fetch(&st, rc);
    if (!rc && qr_stage_any(info, nb)) rc = QR_E_SINGULAR;
    qr_stage_close(&st);
    return rc;
}
