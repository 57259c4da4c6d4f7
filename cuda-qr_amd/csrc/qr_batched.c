/* qr_batched.c -- factorisation and least squares of many small matrices at once (mi355x_qr.h section 8).
 *
 *   qr_geqrf_batched_dev   one launch: a wave or a workgroup per matrix (qrd_b_geqrf; the route follows from (m, n) alone)
 *   qr_ormqr_batched_dev   one launch (qrd_b_ormqr);  qr_orgqr_batched_dev: the identity written on the device, then ormqr 'N'
 *   qr_gels_batched_dev    one fused launch while n + nrhs columns fit the kernel (the right-hand sides ride along as columns that are
 *                          updated but never factored, the back substitution runs in the same kernel); else geqrf, ormqr 'T', qrd_b_trsm
 *   qr_thin_batched, qr_lstsq_batched   the same on host pointers, packed batches
 *   section 8b, column pivoting: qr_geqp3_batched_dev and qr_rank_batched_dev are one launch each (qrd_b_geqp3, qrd_b_rank);
 *                          qr_gelsp_batched_dev / qr_gelsy_batched_dev route as qr_gels_batched_dev does: fused, else geqp3, ormqr 'T',
 *                          qrd_b_solve_piv; qr_thin_pivoted_batched, qr_lstsq_pivoted_batched on host pointers
 *   section 8c, singular values: qr_gesvd_batched_dev is geqp3, qrd_b_jsvd (qr_batched_svd.hip: rank cut, Jacobi on R^T in LDS, V) and,
 *                          when U is wanted, ormqr 'N' on [W; 0]: three launches, or two; qr_svd_batched on host pointers
 *
 * The plan supplies the stream; its shape does not bound m and n.  Nothing here waits on the host except the host-pointer twins.
 *
 * Kept out of qr_host.c for the reason qr_solve.c is: the sanitizer and stub builds compile qr_host.c against a stub device layer that
 * has none of the launch wrappers called here. */
#define _POSIX_C_SOURCE 200809L
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355x_qr.h"
#include "qr_device.h"
#include "qr_plan_internal.h"
#include "qr_stage.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

int qr_batched_max_rows(int ncols) { return qrd_b_max_rows(ncols); }

/* the shape of one matrix of the batch and its place in it */
static int bad_shape(int m, int n, int lda, long long strideA, long long stridetau, int batch)
{
    return n < 1 || n > QR_BATCHED_MAX_N || m < n || !qrd_b_fits(m, n) || lda < m || strideA < (long long) lda * n || stridetau < n ||
           batch < 0;
}

/* a block of `cols` columns beside it: at least m rows apart, matrices at least ld * cols apart */
static int bad_block(int m, int cols, int ld, long long stride) { return cols < 1 || ld < m || stride < (long long) ld * cols; }

int qr_geqrf_batched_dev(qr_plan* p, double* dA, int m, int n, int lda, long long strideA, double* dtau, long long stridetau, int batch)
{
    if (!p || !dA || !dtau || bad_shape(m, n, lda, strideA, stridetau, batch)) return QR_E_ARG;
    if (batch == 0) return 0;
    return qrd_b_geqrf(p->stream, dA, m, n, lda, (size_t) strideA, dtau, (size_t) stridetau, NULL, 0, 0, 0, NULL, batch);
}

int qr_ormqr_batched_dev(qr_plan* p, char trans, const double* dA, int m, int n, int lda, long long strideA, const double* dtau,
                         long long stridetau, double* dC, int nrhs, int ldc, long long strideC, int batch)
{
    if (!p || !dA || !dtau || !dC || (trans != 'T' && trans != 'N') || bad_shape(m, n, lda, strideA, stridetau, batch) ||
        bad_block(m, nrhs, ldc, strideC))
        return QR_E_ARG;
    if (batch == 0) return 0;
    return qrd_b_ormqr(p->stream, trans == 'T', dA, m, n, lda, (size_t) strideA, dtau, (size_t) stridetau, dC, nrhs, ldc, (size_t) strideC, batch);
}

int qr_orgqr_batched_dev(qr_plan* p, const double* dA, int m, int n, int lda, long long strideA, const double* dtau, long long stridetau,
                         double* dQ, int ldq, long long strideQ, int batch)
{
    if (!p || !dA || !dtau || !dQ || bad_shape(m, n, lda, strideA, stridetau, batch) || bad_block(m, n, ldq, strideQ)) return QR_E_ARG;
    if (batch == 0) return 0;
    CHECK(qrd_b_eye(p->stream, dQ, m, n, ldq, (size_t) strideQ, batch));
    return qrd_b_ormqr(p->stream, 0, dA, m, n, lda, (size_t) strideA, dtau, (size_t) stridetau, dQ, n, ldq, (size_t) strideQ, batch);
}

int qr_gels_batched_dev(qr_plan* p, double* dA, int m, int n, int lda, long long strideA, double* dtau, long long stridetau, double* dB,
                        int nrhs, int ldb, long long strideB, int* dinfo, int batch)
{
    if (!p || !dA || !dtau || !dB || !dinfo || bad_shape(m, n, lda, strideA, stridetau, batch) || bad_block(m, nrhs, ldb, strideB))
        return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t sa = (size_t) strideA, st = (size_t) stridetau, sb = (size_t) strideB;
    if (nrhs <= QR_BATCHED_MAX_N - n && m <= qrd_b_max_rows(n + nrhs))      /* fused: [A | B] in one kernel */
        return qrd_b_geqrf(p->stream, dA, m, n, lda, sa, dtau, st, dB, nrhs, ldb, sb, dinfo, batch);
    CHECK(qrd_b_geqrf(p->stream, dA, m, n, lda, sa, dtau, st, NULL, 0, 0, 0, NULL, batch));
    CHECK(qrd_b_ormqr(p->stream, 1, dA, m, n, lda, sa, dtau, st, dB, nrhs, ldb, sb, batch));
    return qrd_b_trsm(p->stream, dA, n, lda, sa, dB, nrhs, ldb, sb, dinfo, batch);
}

/* R (n x n, packed) of every member from the factored images F (m x n, packed) */
static void upper_triangles(const double* F, int m, int n, size_t nb, double* R)
{
    for (size_t q = 0; q < nb; ++q)
        for (int c = 0; c < n; ++c)
            for (int r = 0; r < n; ++r) R[q * n * n + (size_t) c * n + r] = r <= c ? F[q * (size_t) m * n + (size_t) c * m + r] : 0.0;
}

/* the host-pointer twins, here and in sections 8b and 8c: packed batches, staged as qr_stage.h describes */
int qr_thin_batched(const double* A, int m, int n, int batch, double* Q, double* R)
{
    if (!A || !Q || !R || n < 1 || n > QR_BATCHED_MAX_N || m < n || !qrd_b_fits(m, n) || batch < 0) return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t mn = (size_t) m * n, nb = (size_t) batch;
    double* F = (double*) malloc(sizeof(double) * nb * mn);
    if (!F) return QR_E_ALLOC;
    double *dA, *dQ, *dtau;
    qr_stage_buf t[] = { QR_STAGE_F64(dA, nb * mn, A, F, 0), QR_STAGE_F64(dQ, nb * mn, NULL, Q, 0), QR_STAGE_F64(dtau, nb * (size_t) n, NULL, NULL, 0) };
    qr_stage st;
    int rc = qr_stage_open(&st, m, n, t, QR_STAGE_COUNT(t));
    if (!rc) rc = qr_geqrf_batched_dev(st.plan, dA, m, n, m, (long long) mn, dtau, n, batch);
    if (!rc) rc = qr_orgqr_batched_dev(st.plan, dA, m, n, m, (long long) mn, dtau, n, dQ, m, (long long) mn, batch);
    rc = qr_stage_fetch(&st, rc);
    if (!rc) upper_triangles(F, m, n, nb, R);
    qr_stage_close(&st);
    free(F);
    return rc;
}

int qr_lstsq_batched(const double* A, int m, int n, const double* B, int nrhs, int batch, double* X, double* resid, int* info)
{
    if (!A || !B || !X || !info || n < 1 || n > QR_BATCHED_MAX_N || m < n || !qrd_b_fits(m, n) || nrhs < 1 || batch < 0) return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t mn = (size_t) m * n, mr = (size_t) m * nrhs, nb = (size_t) batch;
    double* C = (double*) malloc(sizeof(double) * nb * mr);
    if (!C) return QR_E_ALLOC;
    double *dA, *dB, *dtau;
    int* dinfo;
    qr_stage_buf t[] = { QR_STAGE_F64(dA, nb * mn, A, NULL, 0), QR_STAGE_F64(dB, nb * mr, B, C, 0), QR_STAGE_F64(dtau, nb * (size_t) n, NULL, NULL, 0),
                         QR_STAGE_I32(dinfo, nb, NULL, info, 0) };
    qr_stage st;
    int rc = qr_stage_open(&st, m, n, t, QR_STAGE_COUNT(t));
    if (!rc) rc = qr_gels_batched_dev(st.plan, dA, m, n, m, (long long) mn, dtau, n, dB, nrhs, m, (long long) mr, dinfo, batch);
    rc = qr_stage_fetch(&st, rc);
    if (!rc)
        for (size_t q = 0; q < nb; ++q) {
            for (int j = 0; j < nrhs; ++j) {
                const double* c = C + q * mr + (size_t) j * m;
                memcpy(X + (q * nrhs + j) * n, c, sizeof(double) * (size_t) n);
                if (resid) {
                    double s = 0.0;
                    for (int i = n; i < m; ++i) s += c[i] * c[i];
                    resid[q * nrhs + j] = sqrt(s);
                }
            }
            if (info[q]) rc = QR_E_SINGULAR;
        }
    qr_stage_close(&st);
    free(C);
    return rc;
}

/* ---- section 8b: column pivoting ---- */

static double eff_rcond(double rcond, int m, int n) { return rcond < 0.0 ? (double) (m > n ? m : n) * DBL_EPSILON : rcond; }

int qr_geqp3_batched_dev(qr_plan* p, double* dA, int m, int n, int lda, long long strideA, int* djpvt, long long stridejpvt, double* dtau,
                         long long stridetau, int batch)
{
    if (!p || !dA || !djpvt || !dtau || bad_shape(m, n, lda, strideA, stridetau, batch) || stridejpvt < n) return QR_E_ARG;
    if (batch == 0) return 0;
    return qrd_b_geqp3(p->stream, dA, m, n, lda, (size_t) strideA, djpvt, (size_t) stridejpvt, dtau, (size_t) stridetau, NULL, 0, 0, 0, 0.0, 0,
                       NULL, NULL, batch);
}

int qr_rank_batched_dev(qr_plan* p, const double* dA, int m, int n, int lda, long long strideA, double rcond, int* drank, int batch)
{
    if (!p || !dA || !drank || rcond != rcond || bad_shape(m, n, lda, strideA, n, batch)) return QR_E_ARG;
    if (batch == 0) return 0;
    return qrd_b_rank(p->stream, dA, n, lda, (size_t) strideA, eff_rcond(rcond, m, n), drank, batch);
}

static int gelsx_batched(qr_plan* p, double* dA, int m, int n, int lda, long long strideA, int* djpvt, long long stridejpvt, double* dtau,
                         long long stridetau, double* dB, int nrhs, int ldb, long long strideB, double rcond, double* dresid, int* drank,
                         int batch, int minnorm)
{
    if (!p || !dA || !djpvt || !dtau || !dB || rcond != rcond || bad_shape(m, n, lda, strideA, stridetau, batch) || stridejpvt < n ||
        bad_block(m, nrhs, ldb, strideB))
        return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t sa = (size_t) strideA, sj = (size_t) stridejpvt, st = (size_t) stridetau, sb = (size_t) strideB;
    const double rc = eff_rcond(rcond, m, n);
    if (nrhs <= QR_BATCHED_MAX_N - n && m <= qrd_b_max_rows(n + nrhs))      /* fused: [A | B] in one kernel */
        return qrd_b_geqp3(p->stream, dA, m, n, lda, sa, djpvt, sj, dtau, st, dB, nrhs, ldb, sb, rc, minnorm, dresid, drank, batch);
    CHECK(qrd_b_geqp3(p->stream, dA, m, n, lda, sa, djpvt, sj, dtau, st, NULL, 0, 0, 0, 0.0, 0, NULL, NULL, batch));
    CHECK(qrd_b_ormqr(p->stream, 1, dA, m, n, lda, sa, dtau, st, dB, nrhs, ldb, sb, batch));
    return qrd_b_solve_piv(p->stream, dA, m, n, lda, sa, djpvt, sj, dB, nrhs, ldb, sb, rc, minnorm, dresid, drank, batch);
}

int qr_gelsp_batched_dev(qr_plan* p, double* dA, int m, int n, int lda, long long strideA, int* djpvt, long long stridejpvt, double* dtau,
                         long long stridetau, double* dB, int nrhs, int ldb, long long strideB, double rcond, double* dresid, int* drank,
                         int batch)
{
    return gelsx_batched(p, dA, m, n, lda, strideA, djpvt, stridejpvt, dtau, stridetau, dB, nrhs, ldb, strideB, rcond, dresid, drank, batch, 0);
}

int qr_gelsy_batched_dev(qr_plan* p, double* dA, int m, int n, int lda, long long strideA, int* djpvt, long long stridejpvt, double* dtau,
                         long long stridetau, double* dB, int nrhs, int ldb, long long strideB, double rcond, double* dresid, int* drank,
                         int batch)
{
    return gelsx_batched(p, dA, m, n, lda, strideA, djpvt, stridejpvt, dtau, stridetau, dB, nrhs, ldb, strideB, rcond, dresid, drank, batch, 1);
}

int qr_thin_pivoted_batched(const double* A, int m, int n, int batch, double* Q, double* R, int* jpvt)
{
    if (!A || !Q || !R || !jpvt || n < 1 || n > QR_BATCHED_MAX_N || m < n || !qrd_b_fits(m, n) || batch < 0) return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t mn = (size_t) m * n, nb = (size_t) batch;
    double* F = (double*) malloc(sizeof(double) * nb * mn);
    if (!F) return QR_E_ALLOC;
    double *dA, *dQ, *dtau;
    int* dj;
    qr_stage_buf t[] = { QR_STAGE_F64(dA, nb * mn, A, F, 0), QR_STAGE_F64(dQ, nb * mn, NULL, Q, 0), QR_STAGE_F64(dtau, nb * (size_t) n, NULL, NULL, 0),
                         QR_STAGE_I32(dj, nb * (size_t) n, NULL, jpvt, 0) };
    qr_stage st;
    int rc = qr_stage_open(&st, m, n, t, QR_STAGE_COUNT(t));
    if (!rc) rc = qr_geqp3_batched_dev(st.plan, dA, m, n, m, (long long) mn, dj, n, dtau, n, batch);
    if (!rc) rc = qr_orgqr_batched_dev(st.plan, dA, m, n, m, (long long) mn, dtau, n, dQ, m, (long long) mn, batch);
    rc = qr_stage_fetch(&st, rc);
    if (!rc) upper_triangles(F, m, n, nb, R);
    qr_stage_close(&st);
    free(F);
    return rc;
}

int qr_lstsq_pivoted_batched(const double* A, int m, int n, const double* B, int nrhs, int batch, double rcond, int minnorm, double* X,
                             double* resid, int* rank, int* jpvt)
{
    if (!A || !B || !X || rcond != rcond || n < 1 || n > QR_BATCHED_MAX_N || m < n || !qrd_b_fits(m, n) || nrhs < 1 || batch < 0)
        return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t mn = (size_t) m * n, mr = (size_t) m * nrhs, nb = (size_t) batch;
    double* C = (double*) malloc(sizeof(double) * nb * mr);
    if (!C) return QR_E_ALLOC;
    double *dA, *dB, *dtau, *dres;
    int *dj, *drank;
    qr_stage_buf t[] = { QR_STAGE_F64(dA, nb * mn, A, NULL, 0), QR_STAGE_F64(dB, nb * mr, B, C, 0), QR_STAGE_F64(dtau, nb * (size_t) n, NULL, NULL, 0),
                         QR_STAGE_F64(dres, nb * (size_t) nrhs, NULL, resid, 0), QR_STAGE_I32(dj, nb * (size_t) n, NULL, jpvt, 0),
                         QR_STAGE_I32(drank, nb, NULL, rank, 0) };
    qr_stage st;
    int rc = qr_stage_open(&st, m, n, t, QR_STAGE_COUNT(t));
    if (!rc)
        rc = gelsx_batched(st.plan, dA, m, n, m, (long long) mn, dj, n, dtau, n, dB, nrhs, m, (long long) mr, rcond, dres, drank, batch, minnorm != 0);
    rc = qr_stage_fetch(&st, rc);
    if (!rc)
        for (size_t q = 0; q < nb; ++q)
            for (int j = 0; j < nrhs; ++j) memcpy(X + (q * nrhs + j) * n, C + q * mr + (size_t) j * m, sizeof(double) * (size_t) n);
    qr_stage_close(&st);
    free(C);
    return rc;
}

/* ---- section 8c: singular value decomposition ---- */

static int bad_job(char job, char yes) { return job != yes && job != 'N'; }

int qr_gesvd_batched_dev(qr_plan* p, char jobu, char jobv, double* dA, int m, int n, int lda, long long strideA, int* djpvt,
                         long long stridejpvt, double* dtau, long long stridetau, double* dS, long long strideS, double* dU, int ldu,
                         long long strideU, double* dV, int ldv, long long strideV, int* drank, int* dsweeps, int* dinfo, int batch)
{
    if (!p || !dA || !djpvt || !dtau || !dS || !dinfo || bad_job(jobu, 'U') || bad_job(jobv, 'V') ||
        bad_shape(m, n, lda, strideA, stridetau, batch) || stridejpvt < n || strideS < n)
        return QR_E_ARG;
    if (jobu == 'U' && (!dU || bad_block(m, n, ldu, strideU))) return QR_E_ARG;
    if (jobv == 'V' && (!dV || bad_block(n, n, ldv, strideV))) return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t sa = (size_t) strideA, sj = (size_t) stridejpvt, st = (size_t) stridetau;
    double* U = jobu == 'U' ? dU : NULL;
    double* V = jobv == 'V' ? dV : NULL;
    CHECK(qrd_b_geqp3(p->stream, dA, m, n, lda, sa, djpvt, sj, dtau, st, NULL, 0, 0, 0, 0.0, 0, NULL, NULL, batch));
    CHECK(qrd_b_jsvd(p->stream, dA, m, n, lda, sa, djpvt, sj, dS, (size_t) strideS, U, ldu, (size_t) strideU, V, ldv, (size_t) strideV, drank,
                     dsweeps, dinfo, QR_JSVD_MAX_SWEEPS, batch));
    if (!U) return 0;
    return qrd_b_ormqr(p->stream, 0, dA, m, n, lda, sa, dtau, st, U, n, ldu, (size_t) strideU, batch);
}

int qr_svd_batched(const double* A, int m, int n, int batch, double* S, double* U, double* V, int* rank)
{
    if (!A || !S || n < 1 || n > QR_BATCHED_MAX_N || m < n || !qrd_b_fits(m, n) || batch < 0) return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t mn = (size_t) m * n, nn = (size_t) n * n, nb = (size_t) batch;
    int* info = (int*) malloc(sizeof(int) * nb);
    if (!info) return QR_E_ALLOC;
    double *dA, *dtau, *dS, *dU, *dV;
    int *dj, *drank, *dinfo;
    /* U and V take no room where they are not wanted */
    qr_stage_buf t[] = { QR_STAGE_F64(dA, nb * mn, A, NULL, 0), QR_STAGE_F64(dtau, nb * (size_t) n, NULL, NULL, 0),
                         QR_STAGE_F64(dS, nb * (size_t) n, NULL, S, 0), QR_STAGE_F64(dU, U ? nb * mn : 0, NULL, U, 0),
                         QR_STAGE_F64(dV, V ? nb * nn : 0, NULL, V, 0), QR_STAGE_I32(dj, nb * (size_t) n, NULL, NULL, 0),
                         QR_STAGE_I32(drank, nb, NULL, rank, 0), QR_STAGE_I32(dinfo, nb, NULL, info, 0) };
    qr_stage st;
    int rc = qr_stage_open(&st, m, n, t, QR_STAGE_COUNT(t));
    if (!rc)
        rc = qr_gesvd_batched_dev(st.plan, U ? 'U' : 'N', V ? 'V' : 'N', dA, m, n, m, (long long) mn, dj, n, dtau, n, dS, n, U ? dU : NULL, m,
                                  (long long) mn, V ? dV : NULL, n, (long long) nn, drank, NULL, dinfo, batch);
    rc = qr_stage_fetch(&st, rc);
    if (!rc && qr_stage_any(info, nb)) rc = QR_E_NOCONV;
    qr_stage_close(&st);
    free(info);
    return rc;
}
