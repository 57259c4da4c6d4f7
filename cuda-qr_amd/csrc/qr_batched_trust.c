/* qr_batched_trust.c -- batched trust-region step: per member the lambda >= 0 for which the minimiser x of |A x - b|^2 + lambda^2 |D x|^2
 * has |D x| within rtol of a radius Delta, or lambda = 0 where the Gauss-Newton step is already inside it (mi355x_qr.h section 8g; MINPACK
 * lmpar, the search run on the device).
 *
 *   qr_trust_batched_dev              from factors that exist (R, the top of Q^T b, optional tail sum, jpvt, flip): one launch of
 *                                     qrd_bt_solve (a wave or a workgroup per member; the route follows from n alone)
 *   qr_gels_trust_batched_dev         m >= n: one fused launch of qrd_bt_fused for m <= 64 and n + 1 <= 32; else qrd_b_geqrf, qrd_b_ormqr 'T'
 *                                     and qrd_bt_solve on the triangle and the rows of Q^T b
 *   qr_gels_trust_wide_batched_dev    m < n, D = I: qrd_bm_transpose, qrd_b_geqrf, qrd_bt_solve with flip writing [y ; 0], qrd_b_ormqr 'N'
 *   qr_lsacc_batched_solve_trust_dev  qrd_bt_solve on the accumulator's R, Z and sums
 *   qr_lstsq_trust_batched            the tall or the wide call on host pointers, packed batches
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

#define CHECK(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

/* a block of `cols` columns of `rows` rows: columns at least `rows` apart, members at least ld * cols apart */
static int bad_block(int rows, long long cols, int ld, long long stride) { return cols < 1 || ld < rows || stride < (long long) ld * cols; }

/* `len` values per member that every member may share: a stride of 0, or at least len */
static int bad_shared(long long stride, int len) { return stride != 0 && stride < len; }

/* what every call takes beside its matrices: the radius, the starting guess, the tolerances, the outputs */
typedef struct trust_io {
    const double *ddelta, *dlam0;
    long long stridedelta, stridelam0;
    double rtol;
    int maxit;
    double *dX, *dlam, *dxnorm, *dresid;
    int ldx;
    long long strideX;
    int *diter, *dstatus, *dinfo;
} trust_io;

/* n: the order of the triangle, xrows: the rows of X */
static int bad_io(const trust_io* t, int n, int xrows, int batch)
{
    return n < 1 || n > QR_BATCHED_MAX_N - 1 || batch < 0 || !t->ddelta || bad_shared(t->stridedelta, 1) ||
           (t->dlam0 && bad_shared(t->stridelam0, 1)) || !(t->rtol > 0.0 && t->rtol < 1.0) || t->maxit < 1 || !t->dX || !t->dlam || !t->dinfo ||
           bad_block(xrows, 1, t->ldx, t->strideX);
}

static void fill(qrd_bt_args* a, const trust_io* t, int n, int xrows, int batch)
{
    memset(a, 0, sizeof *a);
    a->delta = t->ddelta; a->sdelta = (size_t) t->stridedelta;
    a->lam0 = t->dlam0; a->slam0 = (size_t) t->stridelam0;
    a->rtol = t->rtol; a->maxit = t->maxit;
    a->lam = t->dlam; a->iter = t->diter; a->status = t->dstatus;
    a->d.X = t->dX; a->d.ldx = t->ldx; a->d.sX = (size_t) t->strideX;
    a->d.xnorm = t->dxnorm; a->d.resid = t->dresid; a->d.info = t->dinfo;
    a->d.n = n; a->d.nrhs = 1; a->d.nlam = 1; a->d.zrows = n; a->d.xrows = xrows; a->d.batch = batch;
}

int qr_trust_batched_dev(qr_plan* p, const double* dR, int n, int ldr, long long strideR, const double* dZ, int ldz, long long strideZ,
                         const double* drss, const int* djpvt, long long stridejpvt, const double* dD, long long strideD, const double* ddelta,
                         long long stridedelta, const double* dlam0, long long stridelam0, double rtol, int maxit, int flip, double* dX, int ldx,
                         long long strideX, double* dlam, double* dxnorm, double* dresid, int* diter, int* dstatus, int* dinfo, int batch)
{
    const trust_io t = {ddelta, dlam0, stridedelta, stridelam0, rtol, maxit, dX, dlam, dxnorm, dresid, ldx, strideX, diter, dstatus, dinfo};
    if (!p || !dR || !dZ || bad_io(&t, n, n, batch) || bad_block(n, n, ldr, strideR) || bad_block(n, 1, ldz, strideZ) ||
        (djpvt && stridejpvt < n) || (dD && bad_shared(strideD, n)) || (flip && (dD || djpvt)))
        return QR_E_ARG;
    if (batch == 0) return 0;
    qrd_bt_args a;
    fill(&a, &t, n, n, batch);
    a.d.R = dR; a.d.ldr = ldr; a.d.sR = (size_t) strideR;
    a.d.Z = dZ; a.d.ldz = ldz; a.d.sZ = (size_t) strideZ;
    a.d.rss = drss;
    a.d.jpvt = djpvt; a.d.sj = (size_t) stridejpvt;
    a.d.D = dD; a.d.sD = (size_t) strideD;
    a.d.flip = flip != 0;
    return qrd_bt_solve(p->stream, &a);
}

int qr_gels_trust_batched_dev(qr_plan* p, double* dA, int m, int n, int lda, long long strideA, double* dtau, long long stridetau, double* dB,
                              int ldb, long long strideB, const double* dD, long long strideD, const double* ddelta, long long stridedelta,
                              const double* dlam0, long long stridelam0, double rtol, int maxit, double* dX, int ldx, long long strideX,
                              double* dlam, double* dxnorm, double* dresid, int* diter, int* dstatus, int* dinfo, int batch)
{
    const trust_io t = {ddelta, dlam0, stridedelta, stridelam0, rtol, maxit, dX, dlam, dxnorm, dresid, ldx, strideX, diter, dstatus, dinfo};
    if (!p || !dA || !dtau || !dB || bad_io(&t, n, n, batch) || m < n || !qrd_b_fits(m, n) || lda < m || strideA < (long long) lda * n ||
        stridetau < n || bad_block(m, 1, ldb, strideB) || (dD && bad_shared(strideD, n)))
        return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t sa = (size_t) strideA, st = (size_t) stridetau, sb = (size_t) strideB;
    qrd_bt_args a;
    fill(&a, &t, n, n, batch);
    a.d.ldz = ldb; a.d.sZ = sb;
    a.d.D = dD; a.d.sD = (size_t) strideD;
    if (m <= 64 && qrd_bd_wave_route(n + 1))             /* fused: factor [A | b] and search in one kernel */
        return qrd_bt_fused(p->stream, dA, m, lda, sa, dtau, st, dB, &a);
    CHECK(qrd_b_geqrf(p->stream, dA, m, n, lda, sa, dtau, st, NULL, 0, 0, 0, NULL, batch));
    CHECK(qrd_b_ormqr(p->stream, 1, dA, m, n, lda, sa, dtau, st, dB, 1, ldb, sb, batch));
    a.d.R = dA; a.d.ldr = lda; a.d.sR = sa;
    a.d.Z = dB; a.d.zrows = m;                            /* rss: the squares of rows n .. m-1 of Q^T b */
    return qrd_bt_solve(p->stream, &a);
}

/* the shape m x n of a wide member whose transpose is factored: qr_gels_wide_batched_dev's rule, m < n; one column rides along */
static int bad_wide_shape(int m, int n)
{
    if (m < 1 || m > QR_BATCHED_MAX_N - 1 || n <= m) return 1;
    if (n <= qrd_b_max_rows(m)) return 0;
    return !qrd_b_fits(n, m);
}

int qr_gels_trust_wide_batched_dev(qr_plan* p, const double* dA, int m, int n, int lda, long long strideA, double* dF, int ldf,
                                   long long strideF, double* dtau, long long stridetau, const double* dB, int ldb, long long strideB,
                                   const double* ddelta, long long stridedelta, const double* dlam0, long long stridelam0, double rtol,
                                   int maxit, double* dX, int ldx, long long strideX, double* dlam, double* dxnorm, double* dresid, int* diter,
                                   int* dstatus, int* dinfo, int batch)
{
    const trust_io t = {ddelta, dlam0, stridedelta, stridelam0, rtol, maxit, dX, dlam, dxnorm, dresid, ldx, strideX, diter, dstatus, dinfo};
    if (!p || !dA || !dF || !dtau || !dB || bad_wide_shape(m, n) || bad_io(&t, m, n, batch) || bad_block(m, n, lda, strideA) ||
        bad_block(n, m, ldf, strideF) || stridetau < m || bad_block(m, 1, ldb, strideB))
        return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t sa = (size_t) strideA, sf = (size_t) strideF, st = (size_t) stridetau;
    CHECK(qrd_bm_transpose(p->stream, dA, m, n, lda, sa, dF, ldf, sf, batch));
    CHECK(qrd_b_geqrf(p->stream, dF, n, m, ldf, sf, dtau, st, NULL, 0, 0, 0, NULL, batch));
    qrd_bt_args a;
    fill(&a, &t, m, n, batch);
    a.d.R = dF; a.d.ldr = ldf; a.d.sR = sf;
    a.d.Z = dB; a.d.ldz = ldb; a.d.sZ = (size_t) strideB;
    a.d.flip = 1;
    CHECK(qrd_bt_solve(p->stream, &a));                   /* [y ; 0]; |x| = |y|, so the radius applies to y */
    return qrd_b_ormqr(p->stream, 0, dF, n, m, ldf, sf, dtau, st, dX, 1, ldx, (size_t) strideX, batch);
}

int qr_lsacc_batched_solve_trust_dev(qr_lsacc_batched* acc, const double* dD, long long strideD, const double* ddelta, long long stridedelta,
                                     const double* dlam0, long long stridelam0, double rtol, int maxit, double* dX, int ldx, long long strideX,
                                     double* dlam, double* dxnorm, double* dresid, int* diter, int* dstatus, int* dinfo)
{
    const trust_io t = {ddelta, dlam0, stridedelta, stridelam0, rtol, maxit, dX, dlam, dxnorm, dresid, ldx, strideX, diter, dstatus, dinfo};
    if (!acc || acc->nrhs != 1 || bad_io(&t, acc->n, acc->n, acc->batch) || (dD && bad_shared(strideD, acc->n))) return QR_E_ARG;
    if (acc->batch == 0) return 0;
    const size_t n = (size_t) acc->n;
    qrd_bt_args a;
    fill(&a, &t, acc->n, acc->n, acc->batch);
    a.d.R = acc->R; a.d.ldr = acc->n; a.d.sR = n * n;
    a.d.Z = acc->Z; a.d.ldz = acc->n; a.d.sZ = n;
    a.d.rss = acc->rss;
    a.d.D = dD; a.d.sD = (size_t) strideD;
    return qrd_bt_solve(acc->p->stream, &a);
}

/* the host-pointer twin: packed batches, staged as qr_stage.h describes */
int qr_lstsq_trust_batched(const double* A, int m, int n, const double* b, int batch, const double* D, const double* delta, const double* lam0,
                           double rtol, int maxit, double* X, double* lam, double* xnorm, double* resid, int* iter, int* status, int* info)
{
    if (!A || !b || !delta || !X || !lam || !info || m < 1 || n < 1 || batch < 0 || !(rtol > 0.0 && rtol < 1.0) || maxit < 1) return QR_E_ARG;
    const int wide = m < n, k = wide ? m : n;             /* k: the order of the triangle */
    if (wide ? (D != NULL || bad_wide_shape(m, n)) : (n > QR_BATCHED_MAX_N - 1 || !qrd_b_fits(m, n))) return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t nb = (size_t) batch, mn = (size_t) m * n;
    double *dA, *dF, *dB, *dtau, *dD, *dX, *ddel, *dl0, *dlam, *dxn, *dres;
    int *diter, *dstat, *dinfo;
    /* iter and status of a member with an info word read 0 */
    qr_stage_buf t[] = { QR_STAGE_F64(dA, nb * mn, A, NULL, 0), QR_STAGE_F64(dF, nb * mn, NULL, NULL, 0), QR_STAGE_F64(dB, nb * (size_t) m, b, NULL, 0),
                         QR_STAGE_F64(dtau, nb * (size_t) k, NULL, NULL, 0), QR_STAGE_F64(dD, nb * (size_t) n, D, NULL, 0),
                         QR_STAGE_F64(dX, nb * (size_t) n, NULL, X, 0), QR_STAGE_F64(ddel, nb, delta, NULL, 0), QR_STAGE_F64(dl0, nb, lam0, NULL, 0),
                         QR_STAGE_F64(dlam, nb, NULL, lam, 0), QR_STAGE_F64(dxn, nb, NULL, xnorm, 0), QR_STAGE_F64(dres, nb, NULL, resid, 0),
                         QR_STAGE_I32(diter, nb, NULL, iter, 1), QR_STAGE_I32(dstat, nb, NULL, status, 1), QR_STAGE_I32(dinfo, nb, NULL, info, 1) };
    qr_stage st;
    int rc = qr_stage_open(&st, wide ? n : m, k, t, QR_STAGE_COUNT(t));
    if (!rc) {
        if (wide)
            rc = qr_gels_trust_wide_batched_dev(st.plan, dA, m, n, m, (long long) mn, dF, n, (long long) mn, dtau, m, dB, m, m, ddel, 1,
                                                lam0 ? dl0 : NULL, 1, rtol, maxit, dX, n, n, dlam, dxn, dres, diter, dstat, dinfo, batch);
        else
            rc = qr_gels_trust_batched_dev(st.plan, dA, m, n, m, (long long) mn, dtau, n, dB, m, m, D ? dD : NULL, n, ddel, 1, lam0 ? dl0 : NULL, 1,
                                           rtol, maxit, dX, n, n, dlam, dxn, dres, diter, dstat, dinfo, batch);
    }
    rc = qr_stage_fetch(&st, rc);
    if (!rc && qr_stage_any(info, nb)) rc = QR_E_SINGULAR;
    qr_stage_close(&st);
    return rc;
}
