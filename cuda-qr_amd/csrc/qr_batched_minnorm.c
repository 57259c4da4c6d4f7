/* qr_batched_minnorm.c -- batched minimum-norm solutions: transposed and wide systems of small matrices (mi355x_qr.h section 8e).
 *
 *   qr_minnorm_batched_dev     X = Q [R^-T B ; 0] from factors that exist: one launch of qrd_bm_apply, any nrhs
 *   qr_gels_t_batched_dev      dgels 'T', m >= n: one fused launch of qrd_bm_fused while n + nrhs columns fit the kernel; else
 *                              qrd_b_geqrf and qrd_bm_apply
 *   qr_transpose_batched_dev   one launch of qrd_bm_transpose
 *   qr_gels_wide_batched_dev   dgels 'N', m <= n: one fused launch of qrd_bm_fused reading A through the transposed index map while
 *                              m + nrhs columns fit; else qrd_bm_transpose into dF, qrd_b_geqrf on it, qrd_bm_apply
 *   qr_lstsq_minnorm_batched   the wide call on host pointers, packed batches
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

/* the tall matrix that is factored and its place in the batch: section 8's rule */
static int bad_shape(int m, int n, int lda, long long strideA, long long stridetau, int batch)
{
    return n < 1 || n > QR_BATCHED_MAX_N || m < n || !qrd_b_fits(m, n) || lda < m || strideA < (long long) lda * n || stridetau < n ||
           batch < 0;
}

/* a block of `cols` columns of `rows` rows: columns at least `rows` apart, members at least ld * cols apart */
static int bad_block(int rows, int cols, int ld, long long stride) { return cols < 1 || ld < rows || stride < (long long) ld * cols; }

/* n + nrhs columns of m rows are held by one kernel */
static int fused_fits(int m, int n, int nrhs)
{
    return nrhs <= QR_BATCHED_MAX_N - n && (m <= qrd_b_max_rows(n + nrhs) || qrd_b_fits(m, n + nrhs));
}

/* the shape m x n of a wide member, its transpose being what is factored: the n rows are within qr_batched_max_rows(m), the value
 * of the widest matrix of m's class, or m is narrower than that matrix and section 8's narrower-fit rule takes n x m (for the widest
 * itself, m == QR_BATCHED_MAX_N, the documented 256 rows are the limit: 64 x 257 is not taken; at m == 32 the class limit is already
 * QRD_B_MAX_ROWS) */
static int bad_wide_shape(int m, int n)
{
    if (m < 1 || m > QR_BATCHED_MAX_N || n < m) return 1;
    if (n <= qrd_b_max_rows(m)) return 0;
    return m == QR_BATCHED_MAX_N || !qrd_b_fits(n, m);
}

int qr_minnorm_batched_dev(qr_plan* p, const double* dA, int m, int n, int lda, long long strideA, const double* dtau, long long stridetau,
                           double* dB, int nrhs, int ldb, long long strideB, int* dinfo, int batch)
{
    if (!p || !dA || !dtau || !dB || !dinfo || bad_shape(m, n, lda, strideA, stridetau, batch) || bad_block(m, nrhs, ldb, strideB))
        return QR_E_ARG;
    if (batch == 0) return 0;
    return qrd_bm_apply(p->stream, dA, m, n, lda, (size_t) strideA, dtau, (size_t) stridetau, dB, nrhs, ldb, (size_t) strideB, dinfo, batch);
}

int qr_gels_t_batched_dev(qr_plan* p, double* dA, int m, int n, int lda, long long strideA, double* dtau, long long stridetau, double* dB,
                          int nrhs, int ldb, long long strideB, int* dinfo, int batch)
{
    if (!p || !dA || !dtau || !dB || !dinfo || bad_shape(m, n, lda, strideA, stridetau, batch) || bad_block(m, nrhs, ldb, strideB))
        return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t sa = (size_t) strideA, st = (size_t) stridetau, sb = (size_t) strideB;
    if (fused_fits(m, n, nrhs))               /* fused: [A | X] in one kernel */
        return qrd_bm_fused(p->stream, 0, dA, m, n, lda, sa, dA, lda, sa, dtau, st, dB, nrhs, ldb, sb, dinfo, batch);
    CHECK(qrd_b_geqrf(p->stream, dA, m, n, lda, sa, dtau, st, NULL, 0, 0, 0, NULL, batch));
    return qrd_bm_apply(p->stream, dA, m, n, lda, sa, dtau, st, dB, nrhs, ldb, sb, dinfo, batch);
}

int qr_transpose_batched_dev(qr_plan* p, const double* dS, int rows, int cols, int lds, long long strideS, double* dD, int ldd,
                             long long strideD, int batch)
{
    if (!p || !dS || !dD || rows < 1 || cols < 1 || rows > QRD_B_MAX_ROWS || cols > QRD_B_MAX_ROWS || bad_block(rows, cols, lds, strideS) ||
        bad_block(cols, rows, ldd, strideD) || batch < 0)
        return QR_E_ARG;
    if (batch == 0) return 0;
    return qrd_bm_transpose(p->stream, dS, rows, cols, lds, (size_t) strideS, dD, ldd, (size_t) strideD, batch);
}

int qr_gels_wide_batched_dev(qr_plan* p, const double* dA, int m, int n, int lda, long long strideA, double* dF, int ldf, long long strideF,
                             double* dtau, long long stridetau, double* dB, int nrhs, int ldb, long long strideB, int* dinfo, int batch)
{
    if (!p || !dA || !dF || !dtau || !dB || !dinfo || bad_wide_shape(m, n) || bad_block(m, n, lda, strideA) || bad_block(n, m, ldf, strideF) ||
        stridetau < m || bad_block(n, nrhs, ldb, strideB) || batch < 0)
        return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t sa = (size_t) strideA, sf = (size_t) strideF, st = (size_t) stridetau, sb = (size_t) strideB;
    if (fused_fits(n, m, nrhs))               /* fused: A read through the transposed index map, [A^T | X] in one kernel */
        return qrd_bm_fused(p->stream, 1, dA, n, m, lda, sa, dF, ldf, sf, dtau, st, dB, nrhs, ldb, sb, dinfo, batch);
    CHECK(qrd_bm_transpose(p->stream, dA, m, n, lda, sa, dF, ldf, sf, batch));
    CHECK(qrd_b_geqrf(p->stream, dF, n, m, ldf, sf, dtau, st, NULL, 0, 0, 0, NULL, batch));
    return qrd_bm_apply(p->stream, dF, n, m, ldf, sf, dtau, st, dB, nrhs, ldb, sb, dinfo, batch);
}

/* the host-pointer twin: packed batches, staged as qr_stage.h describes */
int qr_lstsq_minnorm_batched(const double* A, int m, int n, const double* B, int nrhs, int batch, double* X, int* info)
{
    if (!A || !B || !X || !info || bad_wide_shape(m, n) || nrhs < 1 || batch < 0) return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t mn = (size_t) m * n, nr = (size_t) n * nrhs, nb = (size_t) batch;
    /* X doubles as the staging image of dB: B on top of n - m rows of zeros per column */
    for (size_t q = 0; q < nb; ++q)
        for (int j = 0; j < nrhs; ++j) {
            double* c = X + (q * nrhs + j) * n;
            memcpy(c, B + (q * nrhs + j) * m, sizeof(double) * (size_t) m);
            memset(c + m, 0, sizeof(double) * (size_t) (n - m));
        }
    double *dA, *dF, *dB, *dtau;
    int* dinfo;
    qr_stage_buf t[] = { QR_STAGE_F64(dA, nb * mn, A, NULL, 0), QR_STAGE_F64(dF, nb * mn, NULL, NULL, 0), QR_STAGE_F64(dB, nb * nr, X, X, 0),
                         QR_STAGE_F64(dtau, nb * (size_t) m, NULL, NULL, 0), QR_STAGE_I32(dinfo, nb, NULL, info, 0) };
    qr_stage st;
    int rc = qr_stage_open(&st, n, m, t, QR_STAGE_COUNT(t));
    if (!rc)
        rc = qr_gels_wide_batched_dev(st.plan, dA, m, n, m, (long long) mn, dF, n, (long long) mn, dtau, m, dB, nrhs, n, (long long) nr, dinfo, batch);
    rc = qr_stage_fetch(&st, rc);
    if (!rc && qr_stage_any(info, nb)) rc = QR_E_SINGULAR;
    qr_stage_close(&st);
    return rc;
}
