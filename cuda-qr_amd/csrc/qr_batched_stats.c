/* qr_batched_stats.c -- batched covariance, standard errors and leverages (mi355x_qr.h section 8k).
 *
 *   qr_stats_batched_max_rows       the largest m the fused fit takes for n unknowns; no device touched
 *   qr_covar_batched_dev            C = mult P [(R11^T R11)^-1 0; 0 0] P^T and its standard errors from a triangle: one launch of qrd_bs_covar
 *   qr_leverage_batched_dev         p_i |R11^-T (P^T a_i)(0 : r)|^2 for arbitrary rows: one launch of qrd_bs_leverage
 *   qr_gels_stats_batched_dev       the weighted fit with residuals, leverages, sigma2, covariance and standard errors: one launch of qrd_bs_fit
 *   qr_lsacc_batched_covar_dev      qr_covar_batched_dev on a batched accumulator's R, the multiplier formed on the device
 *   qr_lstsq_stats_batched          the fused fit on host pointers, packed batches
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

/* the fused fit: 1 <= n <= 63, m >= n, and m rows are held */
static int bad_shape(int m, int n)
{
    if (n < 1 || n > QR_BATCHED_MAX_N - 1 || m < n) return 1;
    return m > qrd_bs_max_rows(n);
}

/* a triangle: 1 <= n <= 64 at ldr >= n, members strideR >= ldr * n apart; jpvt, where given, n per member */
static int bad_triangle(const double* dR, int n, int ldr, long long strideR, const int* djpvt, long long stridejpvt)
{
    return !dR || n < 1 || n > QR_BATCHED_MAX_N || ldr < n || strideR < (long long) ldr * n || (djpvt && stridejpvt < n);
}

/* C (n x n at ldc >= n) and se (n per member): either may be missing, not both */
static int bad_cov_out(int n, const double* dC, int ldc, long long strideC, const double* dse, long long stridese)
{
    return (!dC && !dse) || (dC && (ldc < n || strideC < (long long) ldc * n)) || (dse && stridese < n);
}

int qr_stats_batched_max_rows(int n) { return qrd_bs_max_rows(n); }

int qr_covar_batched_dev(qr_plan* plan, const double* dR, int n, int ldr, long long strideR, const int* djpvt, long long stridejpvt,
                         const int* drank, const double* dmult, double* dC, int ldc, long long strideC, double* dse, long long stridese,
                         int* dinfo, int batch)
{
    if (!plan || !dinfo || batch < 0 || bad_triangle(dR, n, ldr, strideR, djpvt, stridejpvt) || bad_cov_out(n, dC, ldc, strideC, dse, stridese))
        return QR_E_ARG;
    if (batch == 0) return 0;
    qrd_bs_args a;
    memset(&a, 0, sizeof a);
    a.R = dR; a.mult = dmult; a.jpvt = djpvt; a.rank = drank; a.C = dC; a.se = dse; a.info = dinfo;
    a.sR = (size_t) strideR; a.sj = djpvt ? (size_t) stridejpvt : 0; a.sC = dC ? (size_t) strideC : 0; a.sse = dse ? (size_t) stridese : 0;
    a.ldr = ldr; a.ldc = dC ? ldc : n; a.n = n; a.batch = batch;
    return qrd_bs_covar(plan->stream, &a);
}

int qr_leverage_batched_dev(qr_plan* plan, const double* dR, int n, int ldr, long long strideR, const int* djpvt, long long stridejpvt,
                            const int* drank, const double* dA, int mrows, int lda, long long strideA, const double* dprior,
                            long long strideprior, double* dH, long long strideH, int* dinfo, int batch)
{
    if (!plan || !dA || !dH || !dinfo || batch < 0 || bad_triangle(dR, n, ldr, strideR, djpvt, stridejpvt) || mrows < 1 || lda < mrows ||
        strideA < (long long) lda * n || (strideprior != 0 && strideprior < mrows) || strideH < mrows ||
        (long long) batch * qrd_bs_lev_chunks(mrows) > INT_MAX)
        return QR_E_ARG;
    if (batch == 0) return 0;
    qrd_bs_lev_args a;
    memset(&a, 0, sizeof a);
    a.R = dR; a.A = dA; a.prior = dprior; a.jpvt = djpvt; a.rank = drank; a.H = dH; a.info = dinfo;
    a.sR = (size_t) strideR; a.sj = djpvt ? (size_t) stridejpvt : 0; a.sA = (size_t) strideA; a.sprior = (size_t) strideprior;
    a.sH = (size_t) strideH;
    a.ldr = ldr; a.lda = lda; a.n = n; a.mrows = mrows; a.nchunk = qrd_bs_lev_chunks(mrows); a.batch = batch;
    return qrd_bs_leverage(plan->stream, &a);
}

int qr_gels_stats_batched_dev(qr_plan* plan, int scaled, const double* dA, int m, int n, int lda, long long strideA, const double* dB,
                              long long strideB, const double* dprior, long long strideprior, double* dX, long long strideX, double* dE,
                              long long strideE, double* dH, long long strideH, double* dsigma2, int* ddof, double* dC, int ldc,
                              long long strideC, double* dse, long long stridese, int* dinfo, int batch)
{
    if (!plan || !dA || !dB || !dX || !dinfo || batch < 0 || (scaled != QR_COV_UNSCALED && scaled != QR_COV_SCALED) || bad_shape(m, n) ||
        lda < m || strideA < (long long) lda * n || strideB < m || (strideprior != 0 && strideprior < m) || strideX < n ||
        (dE && strideE < m) || (dH && strideH < m) || (dC && (ldc < n || strideC < (long long) ldc * n)) || (dse && stridese < n))
        return QR_E_ARG;
    if (batch == 0) return 0;
    qrd_bs_fit_args a;
    memset(&a, 0, sizeof a);
    a.A = dA; a.B = dB; a.prior = dprior; a.X = dX; a.E = dE; a.H = dH; a.sigma2 = dsigma2; a.C = dC; a.se = dse; a.dof = ddof; a.info = dinfo;
    a.sA = (size_t) strideA; a.sB = (size_t) strideB; a.sprior = (size_t) strideprior; a.sX = (size_t) strideX;
    a.sE = dE ? (size_t) strideE : 0; a.sH = dH ? (size_t) strideH : 0; a.sC = dC ? (size_t) strideC : 0; a.sse = dse ? (size_t) stridese : 0;
    a.lda = lda; a.ldc = dC ? ldc : n; a.m = m; a.n = n; a.scaled = scaled; a.batch = batch;
    return qrd_bs_fit(plan->stream, &a);
}

int qr_lsacc_batched_covar_dev(qr_lsacc_batched* acc, int scaled, int rhs, double* dC, int ldc, long long strideC, double* dse,
                               long long stridese, double* dsigma2, int* dinfo)
{
    if (!acc || !dinfo || (scaled != QR_COV_UNSCALED && scaled != QR_COV_SCALED) || rhs < 0 || rhs >= acc->nrhs ||
        bad_cov_out(acc->n, dC, ldc, strideC, dse, stridese))
        return QR_E_ARG;
    qrd_bs_args a;
    memset(&a, 0, sizeof a);
    a.R = acc->R; a.rss = acc->rss; a.rows = acc->rows; a.C = dC; a.se = dse; a.sigma2 = dsigma2; a.info = dinfo;
    a.sR = (size_t) acc->n * acc->n; a.sC = dC ? (size_t) strideC : 0; a.sse = dse ? (size_t) stridese : 0;
    a.ldr = acc->n; a.ldc = dC ? ldc : acc->n; a.n = acc->n; a.batch = acc->batch; a.acc = 1; a.scaled = scaled; a.nrhs = acc->nrhs; a.rhs = rhs;
    return qrd_bs_covar(acc->p->stream, &a);
}

/* the host-pointer twin: packed batches, staged as qr_stage.h describes */
int qr_lstsq_stats_batched(const double* A, int m, int n, const double* b, const double* prior, int scaled, int batch, double* X, double* E,
                           double* H, double* sigma2, int* dof, double* Cov, double* se, int* info)
{
    if (!A || !b || !X || !info || batch < 0 || (scaled != QR_COV_UNSCALED && scaled != QR_COV_SCALED) || bad_shape(m, n)) return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t nb = (size_t) batch, mn = (size_t) m * n, nn = (size_t) n, mm = (size_t) m;
    double *dA, *dB, *dP, *dX, *dE, *dH, *dsig, *dC, *dse;
    int *ddof, *dinfo;
    /* a member with an info word has nothing else written: its outputs read 0 */
    qr_stage_buf t[] = { QR_STAGE_F64(dA, nb * mn, A, NULL, 0), QR_STAGE_F64(dB, nb * mm, b, NULL, 0), QR_STAGE_F64(dP, nb * mm, prior, NULL, 0),
                         QR_STAGE_F64(dX, nb * nn, NULL, X, 1), QR_STAGE_F64(dE, nb * mm, NULL, E, 1), QR_STAGE_F64(dH, nb * mm, NULL, H, 1),
                         QR_STAGE_F64(dsig, nb, NULL, sigma2, 1), QR_STAGE_F64(dC, nb * nn * nn, NULL, Cov, 1), QR_STAGE_F64(dse, nb * nn, NULL, se, 1),
                         QR_STAGE_I32(ddof, nb, NULL, dof, 1), QR_STAGE_I32(dinfo, nb, NULL, info, 0) };
    qr_stage st;
    int rc = qr_stage_open(&st, m, n, t, QR_STAGE_COUNT(t));
    if (!rc)
        rc = qr_gels_stats_batched_dev(st.plan, scaled, dA, m, n, m, (long long) mn, dB, m, prior ? dP : NULL, m, dX, n, E ? dE : NULL, m,
                                       H ? dH : NULL, m, sigma2 ? dsig : NULL, dof ? ddof : NULL, Cov ? dC : NULL, n, (long long) (nn * nn),
                                       se ? dse : NULL, n, dinfo, batch);
    rc = qr_stage_fetch(&st, rc);
    if (!rc && qr_stage_any(info, nb)) rc = QR_E_SINGULAR;
    qr_stage_close(&st);
    return rc;
}
