/* qr_batched_damped.c -- batched damped least squares: ridge and the Levenberg-Marquardt step, min |A x - b|^2 + lambda^2 |D x|^2 for a
 * list of lambda per member (mi355x_qr.h section 8f).
 *
 *   qr_damped_batched_dev              from factors that exist (R, the top of Q^T B, optional tail sums, jpvt, flip): one launch of
 *                                      qrd_bd_solve (a wave or a workgroup per member; the route follows from n + nrhs alone)
 *   qr_gels_damped_batched_dev         m >= n: one fused launch of qrd_bd_fused for m <= 64 and n + nrhs <= 32; else qrd_b_geqrf,
 *                                      qrd_b_ormqr 'T' and qrd_bd_solve on the triangle and the rows of Q^T B
 *   qr_gels_damped_wide_batched_dev    m < n, D = I: qrd_bm_transpose, qrd_b_geqrf, qrd_bd_solve with flip writing [y ; 0], qrd_b_ormqr 'N'
 *   qr_lsacc_batched_solve_damped_dev  qrd_bd_solve on the accumulator's R, Z and sums
 *   qr_lstsq_damped_batched            the tall or the wide call on host pointers, packed batches
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

/* n, nrhs and the lambda list */
static int bad_counts(int n, int nrhs, int nlam, long long stridelam, int batch)
{
    return n < 1 || nrhs < 1 || nrhs > QR_BATCHED_MAX_N - n || nlam < 1 || bad_shared(stridelam, nlam) || batch < 0;
}

/* the outputs every call has: X (xrows x (nlam * nrhs)), info */
static int bad_out(const double* dX, int xrows, int nrhs, int nlam, int ldx, long long strideX, const int* dinfo)
{
    return !dX || !dinfo || bad_block(xrows, (long long) nlam * nrhs, ldx, strideX);
}

int qr_damped_batched_dev(qr_plan* p, const double* dR, int n, int ldr, long long strideR, const double* dZ, int nrhs, int ldz,
                          long long strideZ, const double* drss, const int* djpvt, long long stridejpvt, const double* dD, long long strideD,
                          const double* dlam, int nlam, long long stridelam, int flip, double* dX, int ldx, long long strideX, double* dxnorm,
                          double* dresid, int* dinfo, int batch)
{
    if (!p || !dR || !dZ || !dlam || bad_counts(n, nrhs, nlam, stridelam, batch) || bad_block(n, n, ldr, strideR) ||
        bad_block(n, nrhs, ldz, strideZ) || (djpvt && stridejpvt < n) || (dD && bad_shared(strideD, n)) || (flip && (dD || djpvt)) ||
        bad_out(dX, n, nrhs, nlam, ldx, strideX, dinfo))
        return QR_E_ARG;
    if (batch == 0) return 0;
    qrd_bd_args a;
    memset(&a, 0, sizeof a);
    a.R = dR; a.ldr = ldr; a.sR = (size_t) strideR;
    a.Z = dZ; a.ldz = ldz; a.sZ = (size_t) strideZ;
    a.rss = drss;
    a.jpvt = djpvt; a.sj = (size_t) stridejpvt;
    a.D = dD; a.sD = (size_t) strideD;
    a.lam = dlam; a.slam = (size_t) stridelam;
    a.X = dX; a.ldx = ldx; a.sX = (size_t) strideX;
    a.xnorm = dxnorm; a.resid = dresid; a.info = dinfo;
    a.n = n; a.nrhs = nrhs; a.nlam = nlam; a.zrows = n; a.xrows = n; a.flip = flip != 0; a.batch = batch;
    return qrd_bd_solve(p->stream, &a);
}

int qr_gels_damped_batched_dev(qr_plan* p, double* dA, int m, int n, int lda, long long strideA, double* dtau, long long stridetau, double* dB,
                               int nrhs, int ldb, long long strideB, const double* dD, long long strideD, const double* dlam, int nlam,
                               long long stridelam, double* dX, int ldx, long long strideX, double* dxnorm, double* dresid, int* dinfo,
                               int batch)
{
    if (!p || !dA || !dtau || !dB || !dlam || bad_counts(n, nrhs, nlam, stridelam, batch) || m < n || !qrd_b_fits(m, n) || lda < m ||
        strideA < (long long) lda * n || stridetau < n || bad_block(m, nrhs, ldb, strideB) || (dD && bad_shared(strideD, n)) ||
        bad_out(dX, n, nrhs, nlam, ldx, strideX, dinfo))
        return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t sa = (size_t) strideA, st = (size_t) stridetau, sb = (size_t) strideB;
    qrd_bd_args a;
    memset(&a, 0, sizeof a);
    a.ldz = ldb; a.sZ = sb;
    a.D = dD; a.sD = (size_t) strideD;
    a.lam = dlam; a.slam = (size_t) stridelam;
    a.X = dX; a.ldx = ldx; a.sX = (size_t) strideX;
    a.xnorm = dxnorm; a.resid = dresid; a.info = dinfo;
    a.n = n; a.nrhs = nrhs; a.nlam = nlam; a.zrows = n; a.xrows = n; a.batch = batch;
    if (m <= 64 && qrd_bd_wave_route(n + nrhs))          /* fused: factor [A | B] and damp in one kernel */
        return qrd_bd_fused(p->stream, dA, m, lda, sa, dtau, st, dB, &a);
    CHECK(qrd_b_geqrf(p->stream, dA, m, n, lda, sa, dtau, st, NULL, 0, 0, 0, NULL, batch));
    CHECK(qrd_b_ormqr(p->stream, 1, dA, m, n, lda, sa, dtau, st, dB, nrhs, ldb, sb, batch));
    a.R = dA; a.ldr = lda; a.sR = sa;
    a.Z = dB; a.zrows = m;                                /* rss: the squares of rows n .. m-1 of Q^T B */
    return qrd_bd_solve(p->stream, &a);
}

/* the shape m x n of a wide member whose transpose is factored: qr_gels_wide_batched_dev's rule, m < n */
static int bad_wide_shape(int m, int n)
{
    if (m < 1 || m > QR_BATCHED_MAX_N || n <= m) return 1;
    if (n <= qrd_b_max_rows(m)) return 0;
    return m == QR_BATCHED_MAX_N || !qrd_b_fits(n, m);
}

int qr_gels_damped_wide_batched_dev(qr_plan* p, const double* dA, int m, int n, int lda, long long strideA, double* dF, int ldf,
                                    long long strideF, double* dtau, long long stridetau, const double* dB, int nrhs, int ldb,
                                    long long strideB, const double* dlam, int nlam, long long stridelam, double* dX, int ldx,
                                    long long strideX, double* dxnorm, double* dresid, int* dinfo, int batch)
{
    if (!p || !dA || !dF || !dtau || !dB || !dlam || bad_wide_shape(m, n) || bad_counts(m, nrhs, nlam, stridelam, batch) ||
        bad_block(m, n, lda, strideA) || bad_block(n, m, ldf, strideF) || stridetau < m || bad_block(m, nrhs, ldb, strideB) ||
        bad_out(dX, n, nrhs, nlam, ldx, strideX, dinfo))
        return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t sa = (size_t) strideA, sf = (size_t) strideF, st = (size_t) stridetau;
    CHECK(qrd_bm_transpose(p->stream, dA, m, n, lda, sa, dF, ldf, sf, batch));
    CHECK(qrd_b_geqrf(p->stream, dF, n, m, ldf, sf, dtau, st, NULL, 0, 0, 0, NULL, batch));
    qrd_bd_args a;
    memset(&a, 0, sizeof a);
    a.R = dF; a.ldr = ldf; a.sR = sf;
    a.Z = dB; a.ldz = ldb; a.sZ = (size_t) strideB;
    a.lam = dlam; a.slam = (size_t) stridelam;
    a.X = dX; a.ldx = ldx; a.sX = (size_t) strideX;
    a.xnorm = dxnorm; a.resid = dresid; a.info = dinfo;
    a.n = m; a.nrhs = nrhs; a.nlam = nlam; a.zrows = m; a.xrows = n; a.flip = 1; a.batch = batch;
    CHECK(qrd_bd_solve(p->stream, &a));                   /* [y ; 0] in every column */
    return qrd_b_ormqr(p->stream, 0, dF, n, m, ldf, sf, dtau, st, dX, nlam * nrhs, ldx, (size_t) strideX, batch);
}

int qr_lsacc_batched_solve_damped_dev(qr_lsacc_batched* acc, const double* dD, long long strideD, const double* dlam, int nlam,
                                      long long stridelam, double* dX, int ldx, long long strideX, double* dxnorm, double* dresid, int* dinfo)
{
    if (!acc || !dlam || nlam < 1 || bad_shared(stridelam, nlam) || (dD && bad_shared(strideD, acc->n)) ||
        bad_out(dX, acc->n, acc->nrhs, nlam, ldx, strideX, dinfo))
        return QR_E_ARG;
    if (acc->batch == 0) return 0;
    const size_t n = (size_t) acc->n;
    qrd_bd_args a;
    memset(&a, 0, sizeof a);
    a.R = acc->R; a.ldr = acc->n; a.sR = n * n;
    a.Z = acc->Z; a.ldz = acc->n; a.sZ = n * (size_t) acc->nrhs;
    a.rss = acc->rss;
    a.D = dD; a.sD = (size_t) strideD;
    a.lam = dlam; a.slam = (size_t) stridelam;
    a.X = dX; a.ldx = ldx; a.sX = (size_t) strideX;
    a.xnorm = dxnorm; a.resid = dresid; a.info = dinfo;
    a.n = acc->n; a.nrhs = acc->nrhs; a.nlam = nlam; a.zrows = acc->n; a.xrows = acc->n; a.batch = acc->batch;
    return qrd_bd_solve(acc->p->stream, &a);
}

/* the host-pointer twin: packed batches, staged as qr_stage.h describes */
int qr_lstsq_damped_batched(const double* A, int m, int n, const double* B, int nrhs, int batch, const double* D, const double* lam, int nlam,
                            double* X, double* xnorm, double* resid, int* info)
{
    if (!A || !B || !lam || !X || !info || m < 1 || n < 1 || nrhs < 1 || nlam < 1 || batch < 0) return QR_E_ARG;
    const int wide = m < n, k = wide ? m : n;             /* k: the order of the triangle */
    if (nrhs > QR_BATCHED_MAX_N - k || (wide ? (D != NULL || bad_wide_shape(m, n)) : (n > QR_BATCHED_MAX_N || !qrd_b_fits(m, n))))
        return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t nb = (size_t) batch, mn = (size_t) m * n, mr = (size_t) m * nrhs, cols = (size_t) nlam * nrhs, nx = (size_t) n * cols;
    double *dA, *dF, *dB, *dtau, *dD, *dlam, *dX, *dxn, *dres;
    int* dinfo;
    qr_stage_buf t[] = { QR_STAGE_F64(dA, nb * mn, A, NULL, 0), QR_STAGE_F64(dF, nb * mn, NULL, NULL, 0), QR_STAGE_F64(dB, nb * mr, B, NULL, 0),
                         QR_STAGE_F64(dtau, nb * (size_t) k, NULL, NULL, 0), QR_STAGE_F64(dD, nb * (size_t) n, D, NULL, 0),
                         QR_STAGE_F64(dlam, nb * (size_t) nlam, lam, NULL, 0), QR_STAGE_F64(dX, nb * nx, NULL, X, 0),
                         QR_STAGE_F64(dxn, nb * cols, NULL, xnorm, 0), QR_STAGE_F64(dres, nb * cols, NULL, resid, 0),
                         QR_STAGE_I32(dinfo, nb * (size_t) nlam, NULL, info, 0) };
    qr_stage st;
    int rc = qr_stage_open(&st, wide ? n : m, k, t, QR_STAGE_COUNT(t));
    if (!rc) {
        if (wide)
            rc = qr_gels_damped_wide_batched_dev(st.plan, dA, m, n, m, (long long) mn, dF, n, (long long) mn, dtau, m, dB, nrhs, m, (long long) mr,
                                                 dlam, nlam, nlam, dX, n, (long long) nx, dxn, dres, dinfo, batch);
        else
            rc = qr_gels_damped_batched_dev(st.plan, dA, m, n, m, (long long) mn, dtau, n, dB, nrhs, m, (long long) mr, D ? dD : NULL, n, dlam,
                                            nlam, nlam, dX, n, (long long) nx, dxn, dres, dinfo, batch);
    }
    rc = qr_stage_fetch(&st, rc);
    if (!rc && qr_stage_any(info, nb * (size_t) nlam)) rc = QR_E_SINGULAR;
    qr_stage_close(&st);
    return rc;
}
