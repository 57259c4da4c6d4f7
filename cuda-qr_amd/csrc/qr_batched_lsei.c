/* qr_batched_lsei.c -- batched inequality-constrained least squares, Lawson & Hanson's LSEI per member (mi355x_qr.h section 8l).
 *
 *   qr_lsei_batched_max_rows      the largest m taken for n unknowns and mg constraint rows; no device touched
 *   qr_lsei_batched_dev           min |A x - b| subject to G(0:neq) x = h(0:neq), G(neq:mg) x >= h(neq:mg) for every member: one launch
 *                                 of qrd_le_solve
 *   qr_lstsq_inequality_batched   the same on host pointers, packed batches
 *
 * The plan supplies the stream.  Nothing here waits on the host except the host-pointer twin.
 *
 * Kept out of qr_host.c for the reason qr_solve.c is: the sanitizer and stub builds compile qr_host.c against a stub device layer that
 * has none of the launch wrappers called here. */
#define _POSIX_C_SOURCE 200809L
#include <float.h>
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355x_qr.h"
#include "qr_device.h"
#include "qr_plan_internal.h"
#include "qr_stage.h"

/* 1 <= n <= 63, 1 <= mg <= 64, 0 <= neq <= min(n, mg), m >= 1, m + neq >= n, and m rows are held */
static int bad_shape(int m, int n, int mg, int neq)
{
    if (n < 1 || n > QR_BATCHED_MAX_N - 1 || mg < 1 || mg > 64 || neq < 0 || neq > n || neq > mg || m < 1 || m < n - neq) return 1;
    return m > qrd_le_max_rows(n, mg);
}

/* maxit <= 0: 3 mg + 1; the kernels count candidates in an int */
static int iteration_cap(int maxit, int mg) { return maxit <= 0 ? 3 * mg + 1 : (maxit > INT_MAX / 4 ? INT_MAX / 4 : maxit); }

/* rcond <= 0 (or a NaN): n eps */
static double dependence_bound(double rcond, int n) { return rcond > 0.0 ? rcond : n * DBL_EPSILON; }

int qr_lsei_batched_max_rows(int n, int mg) { return qrd_le_max_rows(n, mg); }

int qr_lsei_batched_dev(qr_plan* plan, const double* dA, int m, int n, int lda, long long strideA, const double* dB, long long strideB,
                        const double* dG, int mg, int neq, int ldg, long long strideG, const double* dH, long long strideH, int maxit,
                        double rcond, double* dX, long long strideX, double* dMU, long long strideMU, double* dS, long long strideS, int* dstate,
                        long long stridestate, double* dresid, int* diter, int* dinfo, int batch)
{
    if (!plan || !dA || !dB || !dG || !dH || !dX || !dinfo || batch < 0 || bad_shape(m, n, mg, neq) || lda < m ||
        strideA < (long long) lda * n || strideB < m || ldg < mg || (strideG != 0 && strideG < (long long) ldg * n) ||
        (strideH != 0 && strideH < mg) || strideX < n || (dMU && strideMU < mg) || (dS && strideS < mg) || (dstate && stridestate < mg))
        return QR_E_ARG;
    if (batch == 0) return 0;
    qrd_le_args a;
    memset(&a, 0, sizeof a);
    a.A = dA; a.B = dB; a.G = dG; a.H = dH;
    a.X = dX; a.MU = dMU; a.S = dS; a.resid = dresid; a.state = dstate; a.iter = diter; a.info = dinfo;
    a.sA = (size_t) strideA; a.sB = (size_t) strideB; a.sG = (size_t) strideG; a.sH = (size_t) strideH; a.sX = (size_t) strideX;
    a.sMU = dMU ? (size_t) strideMU : 0; a.sS = dS ? (size_t) strideS : 0; a.sstate = dstate ? (size_t) stridestate : 0;
    a.rcond = dependence_bound(rcond, n);
    a.lda = lda; a.ldg = ldg; a.m = m; a.n = n; a.mg = mg; a.neq = neq; a.maxit = iteration_cap(maxit, mg); a.batch = batch;
    return qrd_le_solve(plan->stream, &a);
}

/* the host-pointer twin: packed batches, staged as qr_stage.h describes */
int qr_lstsq_inequality_batched(const double* A, int m, int n, const double* b, const double* G, int mg, int neq, const double* h, int maxit,
                                double rcond, int batch, double* X, double* MU, double* S, int* state, double* resid, int* iter, int* info)
{
    if (!A || !b || !G || !h || !X || !info || batch < 0 || bad_shape(m, n, mg, neq)) return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t nb = (size_t) batch, mn = (size_t) m * n, gn = (size_t) mg * n, nn = (size_t) n, gg = (size_t) mg;
    double *dA, *dB, *dG, *dH, *dX, *dMU, *dS, *dres;
    int *dstate, *diter, *dinfo;
    /* a member with info -2, -3 or i + 1 has nothing written: its X, MU, S, resid, state and iter read 0 */
    qr_stage_buf t[] = { QR_STAGE_F64(dA, nb * mn, A, NULL, 0), QR_STAGE_F64(dB, nb * (size_t) m, b, NULL, 0), QR_STAGE_F64(dG, nb * gn, G, NULL, 0),
                         QR_STAGE_F64(dH, nb * gg, h, NULL, 0), QR_STAGE_F64(dX, nb * nn, NULL, X, 1), QR_STAGE_F64(dMU, nb * gg, NULL, MU, 1),
                         QR_STAGE_F64(dS, nb * gg, NULL, S, 1), QR_STAGE_F64(dres, nb, NULL, resid, 1), QR_STAGE_I32(dstate, nb * gg, NULL, state, 1),
                         QR_STAGE_I32(diter, nb, NULL, iter, 1), QR_STAGE_I32(dinfo, nb, NULL, info, 0) };
    qr_stage st;
    int rc = qr_stage_open(&st, m > n ? m : n, n, t, QR_STAGE_COUNT(t));
    if (!rc)
        rc = qr_lsei_batched_dev(st.plan, dA, m, n, m, (long long) mn, dB, m, dG, mg, neq, mg, (long long) gn, dH, mg, maxit, rcond, dX, n,
                                 MU ? dMU : NULL, mg, S ? dS : NULL, mg, state ? dstate : NULL, mg, resid ? dres : NULL, iter ? diter : NULL,
                                 dinfo, batch);
    rc = qr_stage_fetch(&st, rc);
    if (!rc && qr_stage_any(info, nb)) rc = QR_E_SINGULAR;
    qr_stage_close(&st);
    return rc;
}
