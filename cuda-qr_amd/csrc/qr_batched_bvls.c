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

/* the host-pointer twin: a plan of its own, one device allocation of doubles and one of ints, packed batches */
int qr_lstsq_bounded_batched(const double* A, int m, int n, const double* b, const double* lo, const double* hi, int maxit, int batch, double* X,
                             double* W, int* state, double* resid, int* iter, int* info)
{
    if (!A || !b || !X || !info || batch < 0 || bad_shape(m, n)) return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t nb = (size_t) batch, mn = (size_t) m * n, nn = (size_t) n;
    qr_plan* plan = NULL;
    int rc = qr_plan_create(&plan, m, n, 0, 0);
    if (rc) return rc;
    double* dv = NULL;
    int* di = NULL;
    double *dA = NULL, *dB = NULL, *dlo = NULL, *dhi = NULL, *dX = NULL, *dW = NULL, *dres = NULL;
    int *dstate = NULL, *diter = NULL, *dinfo = NULL;
    rc = qrd_malloc((void**) &dv, sizeof(double) * nb * (mn + (size_t) m + 4 * nn + 1));
    if (!rc) { dA = dv; dB = dA + nb * mn; dlo = dB + nb * m; dhi = dlo + nb * nn; dX = dhi + nb * nn; dW = dX + nb * nn; dres = dW + nb * nn; }
    if (!rc) rc = qrd_malloc((void**) &di, sizeof(int) * nb * (nn + 2));
    if (!rc) { dstate = di; diter = dstate + nb * nn; dinfo = diter + nb; }
    if (!rc) rc = qrd_h2d(plan->stream, dA, A, sizeof(double) * nb * mn);
    if (!rc) rc = qrd_h2d(plan->stream, dB, b, sizeof(double) * nb * m);
    if (!rc && lo) rc = qrd_h2d(plan->stream, dlo, lo, sizeof(double) * nb * nn);
    if (!rc && hi) rc = qrd_h2d(plan->stream, dhi, hi, sizeof(double) * nb * nn);
    /* a member with info -1 or j + 1 has nothing written: its X, W, resid, state and iter read 0 */
    if (!rc) rc = qrd_memset(plan->stream, dX, 0, sizeof(double) * nb * (2 * nn + 1));
    if (!rc) rc = qrd_memset(plan->stream, di, 0, sizeof(int) * nb * (nn + 1));
    if (!rc)
        rc = qr_bvls_batched_dev(plan, dA, m, n, m, (long long) mn, dB, m, lo ? dlo : NULL, hi ? dhi : NULL, n, maxit, dX, n, W ? dW : NULL, n,
                                 state ? dstate : NULL, n, resid ? dres : NULL, iter ? diter : NULL, dinfo, batch);
    if (!rc) rc = qrd_d2h(plan->stream, X, dX, sizeof(double) * nb * nn);
    if (!rc && W) rc = qrd_d2h(plan->stream, W, dW, sizeof(double) * nb * nn);
    if (!rc && resid) rc = qrd_d2h(plan->stream, resid, dres, sizeof(double) * nb);
    if (!rc && state) rc = qrd_d2h(plan->stream, state, dstate, sizeof(int) * nb * nn);
    if (!rc && iter) rc = qrd_d2h(plan->stream, iter, diter, sizeof(int) * nb);
    if (!rc) rc = qrd_d2h(plan->stream, info, dinfo, sizeof(int) * nb);
    const int rs = qrd_stream_sync(plan->stream);
    if (!rc) rc = rs;
    if (!rc)
        for (size_t q = 0; q < nb; ++q)
            if (info[q]) rc = QR_E_SINGULAR;
    if (di) qrd_free(di);
    if (dv) qrd_free(dv);
    qr_plan_destroy(plan);
    return rc;
}
