/* qr_batched_bvls.c -- batched bound-constrained least squares, BVLS and NNLS per member (mi355x_qr.h section 8i).
 *
 *   qr_bvls_batched_max_rows    the largest m taken for n unknowns; no device touched
 *   qr_bvls_batched_dev         min |A x - b| subject to lo <= x <= hi for every member: one launch of qrd_bv_solve
 *   qr_lstsq_bounded_batched    the same on host pointers, packed batches
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
    return m > qrd_bv_max_rows(n);
}

/* maxit <= 0: 3 n; the kernels count actions in an int */
static int iteration_cap(int maxit, int n) { return maxit <= 0 ? 3 * n : (maxit > INT_MAX / 4 ? INT_MAX / 4 : maxit); }

int qr_bvls_batched_max_rows(int n) { return qrd_bv_max_rows(n); }

int qr_bvls_batched_dev(qr_plan* plan, const double* dA, int m, int n, int lda, long long strideA, const double* dB, long long strideB,
                        const double* dlo, const double* dhi, long long stridebnd, int maxit, double* dX, long long strideX, double* dW,
                        long long strideW, int* dstate, long long stridestate, double* dresid, int* diter, int* dinfo, int batch)
{
    if (!plan || !dA || !dB || !dX || !dinfo || batch < 0 || bad_shape(m, n) || lda < m || strideA < (long long) lda * n || strideB < m ||
        (stridebnd != 0 && stridebnd < n) || strideX < n || (dW && strideW < n) || (dstate && stridestate < n))
        return QR_E_ARG;
    if (batch == 0) return 0;
    qrd_bv_args a;
    memset(&a, 0, sizeof a);
    a.A = dA; a.B = dB; a.lo = dlo; a.hi = dhi;
    a.X = dX; a.W = dW; a.resid = dresid; a.state = dstate; a.iter = diter; a.info = dinfo;
    a.sA = (size_t) strideA; a.sB = (size_t) strideB; a.sbnd = (size_t) stridebnd; a.sX = (size_t) strideX;
    a.sW = dW ? (size_t) strideW : 0; a.sstate = dstate ? (size_t) stridestate : 0;
    a.lda = lda; a.m = m; a.n = n; a.maxit = iteration_cap(maxit, n); a.batch = batch;
    return qrd_bv_solve(plan->stream, &a);
}

/* the host-pointer twin: packed batches, staged as qr_stage.h describes */
int qr_lstsq_bounded_batched(const double* A, int m, int n, const double* b, const double* lo, const double* hi, int maxit, int batch, double* X,
                             double* W, int* state, double* resid, int* iter, int* info)
{
    if (!A || !b || !X || !info || batch < 0 || bad_shape(m, n)) return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t nb = (size_t) batch, mn = (size_t) m * n, nn = (size_t) n;
    double *dA, *dB, *dlo, *dhi, *dX, *dW, *dres;
    int *dstate, *diter, *dinfo;
    /* a member with info -1 or j + 1 has nothing written: its X, W, resid, state and iter read 0 */
    qr_stage_buf t[] = { QR_STAGE_F64(dA, nb * mn, A, NULL, 0), QR_STAGE_F64(dB, nb * (size_t) m, b, NULL, 0), QR_STAGE_F64(dlo, nb * nn, lo, NULL, 0),
                         QR_STAGE_F64(dhi, nb * nn, hi, NULL, 0), QR_STAGE_F64(dX, nb * nn, NULL, X, 1), QR_STAGE_F64(dW, nb * nn, NULL, W, 1),
                         QR_STAGE_F64(dres, nb, NULL, resid, 1), QR_STAGE_I32(dstate, nb * nn, NULL, state, 1), QR_STAGE_I32(diter, nb, NULL, iter, 1),
                         QR_STAGE_I32(dinfo, nb, NULL, info, 0) };
    qr_stage st;
    int rc = qr_stage_open(&st, m, n, t, QR_STAGE_COUNT(t));
    if (!rc)
        rc = qr_bvls_batched_dev(st.plan, dA, m, n, m, (long long) mn, dB, m, lo ? dlo : NULL, hi ? dhi : NULL, n, maxit, dX, n, W ? dW : NULL, n,
                                 state ? dstate : NULL, n, resid ? dres : NULL, iter ? diter : NULL, dinfo, batch);
    rc = qr_stage_fetch(&st, rc);
    if (!rc && qr_stage_any(info, nb)) rc = QR_E_SINGULAR;
    qr_stage_close(&st);
    return rc;
}
