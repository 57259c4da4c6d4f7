/* qr_minnorm.c -- minimum-norm solutions with the factors of qr_geqrf_dev (mi355x_qr.h section 5).
 *
 *   qr_solve_rt_dev    R^T X = B: blocked forward substitution on 64-row diagonal blocks, one launch per block (qrd_trsm_t_step); above
 *                      QR_TRSM_T_SKINNY right-hand sides halves are split recursively and the off-diagonal blocks applied with qrd_gemm_tn
 *   qr_minnorm_dev     X = Q [R^-T B ; 0]: solve_rt, zero the tail rows, ormqr('N')
 *   qr_gels_t_dev      geqrf -> minnorm
 *   qr_transpose_dev   D = S^T on 64 x 64 tiles (qrd_transpose_tiled)
 *   qr_gels_wide_dev   transpose the wide matrix into the factor array -> gels_t
 *   qr_lstsq_minnorm   the same on host pointers, through the plan cache of the host-pointer entry points keyed on the transposed shape
 *
 * Kept out of qr_host.c for the reason qr_solve.c is: the sanitizer and stub builds compile qr_host.c against a stub device layer that
 * has none of the launch wrappers called here. */
#define _POSIX_C_SOURCE 200809L
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355x_qr.h"
#include "qr_device.h"
#include "qr_plan_internal.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

/* the one-launch-per-block substitution up to 64 right-hand sides, recursive halving above: the rule of qr_solve_r_dev (QR_TRSM_SKINNY),
 * whose launch count and bytes this mirrors; devtools/tools_minnorm_perf.py measures both routes of both solves side by side */
#define QR_TRSM_T_SKINNY 64

/* lab build: MI355XQR_SOLVE_ROUTE = skinny | gemm forces one route, as in qr_solve.c */
static int trsm_t_skinny(int nrhs)
{
#ifdef QR_LAB
    const char* e = getenv("MI355XQR_SOLVE_ROUTE");
    if (e && strcmp(e, "skinny") == 0) return 1;
    if (e && strcmp(e, "gemm") == 0) return 0;
#endif
    return nrhs <= QR_TRSM_T_SKINNY;
}

static int imin(int a, int b) { return a < b ? a : b; }

/* rows [r0, r1) of the recursive forward substitution (wide B): top part, one TN product for the bottom part's right-hand sides
 * (B[mid:r1] -= R[r0:mid, mid:r1]^T B[r0:mid]), bottom part */
static int solve_rt_rec(qr_plan* p, const double* R, int lda, double* B, int ldb, int nrhs, int r0, int r1)
{
    if (r1 - r0 <= 64) return qrd_trsm_t_step(p->stream, R, lda, B, ldb, nrhs, r1, r0, r1, r0, r0);
    const int mid = r0 + ((r1 - r0) / 2 + 63) / 64 * 64;
    CHECK(solve_rt_rec(p, R, lda, B, ldb, nrhs, r0, mid));
    CHECK(qrd_gemm_tn(p->stream, r1 - mid, nrhs, mid - r0, -1.0, R + (size_t) mid * lda + r0, lda, B + r0, ldb, 1.0, B + mid, ldb,
                      p->slabs, p->slab_cap, NULL, 0));
    return solve_rt_rec(p, R, lda, B, ldb, nrhs, mid, r1);
}

int qr_solve_rt_dev(qr_plan* p, const double* dA, int n, int lda, double* dB, int nrhs, int ldb)
{
    if (!p || !dA || !dB || n < 1 || n > p->n || lda < n || nrhs < 1 || ldb < n) return QR_E_ARG;
    if (!trsm_t_skinny(nrhs)) return solve_rt_rec(p, dA, lda, dB, ldb, nrhs, 0, n);
    /* 64-row blocks q = [64 q, 64 q + 64) from the top: launch q updates every row below block q - 1 with that block's solution and
     * solves block q -- one launch per block */
    const int nl = (n + 63) / 64;
    for (int q = 0; q < nl; ++q) {
        const int l0 = 64 * q, l1 = imin(n, l0 + 64);
        const int x0 = q == 0 ? 0 : l0 - 64, x1 = q == 0 ? 0 : l0;
        CHECK(qrd_trsm_t_step(p->stream, dA, lda, dB, ldb, nrhs, n, l0, l1, x0, x1));
    }
    return 0;
}

static int minnorm_args_ok(const qr_plan* p, const void* dA, int m, int n, int lda, const void* dtau, const void* dB, int nrhs, int ldb)
{
    return p && dA && dtau && dB && n >= 1 && m >= n && m <= p->m && n <= p->n && lda >= m && nrhs >= 1 && ldb >= m;
}

int qr_minnorm_dev(qr_plan* p, const double* dA, int m, int n, int lda, const double* dtau, const double* dT, int ldt, double* dB, int nrhs,
                   int ldb)
{
    if (!minnorm_args_ok(p, dA, m, n, lda, dtau, dB, nrhs, ldb) || (dT && ldt < p->nb)) return QR_E_ARG;
    CHECK(qr_solve_rt_dev(p, dA, n, lda, dB, nrhs, ldb));
    CHECK(qrd_zero_block(p->stream, dB + n, ldb, m - n, nrhs));
    return qr_ormqr_dev(p, 'N', dA, m, n, lda, dtau, dT, ldt, dB, nrhs, ldb);
}

int qr_gels_t_dev(qr_plan* p, double* dA, int m, int n, int lda, double* dtau, double* dB, int nrhs, int ldb)
{
    if (!minnorm_args_ok(p, dA, m, n, lda, dtau, dB, nrhs, ldb)) return QR_E_ARG;
    CHECK(qr_geqrf_dev(p, dA, m, n, lda, dtau));
    return qr_minnorm_dev(p, dA, m, n, lda, dtau, NULL, 0, dB, nrhs, ldb);
}

int qr_transpose_dev(qr_plan* p, const double* dS, int rows, int cols, int lds, double* dD, int ldd)
{
    if (!p || !dS || !dD || rows < 1 || cols < 1 || lds < rows || ldd < cols) return QR_E_ARG;
    return qrd_transpose_tiled(p->stream, rows, cols, dS, lds, dD, ldd);
}

int qr_gels_wide_dev(qr_plan* p, const double* dA, int m, int n, int lda, double* dF, int ldf, double* dtau, double* dB, int nrhs, int ldb)
{
    /* the plan factors A^T: n x m */
    if (!p || !dA || !dF || !dtau || !dB || m < 1 || m > n || n > p->m || m > p->n || lda < m || ldf < n || nrhs < 1 || ldb < n)
        return QR_E_ARG;
    CHECK(qr_transpose_dev(p, dA, m, n, lda, dF, ldf));
    return qr_gels_t_dev(p, dF, n, m, ldf, dtau, dB, nrhs, ldb);
}

int qr_lstsq_minnorm(const double* A, int m, int n, const double* B, int nrhs, double* X)
{
    if (!A || !B || !X || m < 1 || m > n || nrhs < 1) return QR_E_ARG;
    host_slot priv, *sl = NULL;
    CHECK(qr_host_slot_acquire(n, m, &priv, &sl));       /* the transposed shape: sl->dA is n x m, sl->dtau m doubles */
    qr_plan* p = sl->p;
    const int latch0 = p->guard_latch;
    p->guard_latch = 0;                    /* a blocking entry point: a refused tall panel goes to the leaf chain (as in qr_lstsq) */
    double* diag = (double*) malloc(sizeof(double) * (size_t) m);
    int rc = diag ? 0 : QR_E_ALLOC;
    if (!rc) rc = qr_host_slot_need(&sl->dR, &sl->r_cap, (size_t) m * n);        /* A as the caller holds it: transposed on the device */
    if (!rc) rc = qr_host_slot_need(&sl->dQ, &sl->q_cap, (size_t) n * nrhs);
    if (!rc) rc = qrd_h2d(p->stream, sl->dR, A, sizeof(double) * (size_t) m * n);
    if (!rc) rc = qrd_h2d_2d(p->stream, sl->dQ, sizeof(double) * (size_t) n, B, sizeof(double) * (size_t) m, sizeof(double) * (size_t) m, nrhs);
    if (!rc) rc = qr_gels_wide_dev(p, sl->dR, m, n, m, sl->dA, n, sl->dtau, sl->dQ, nrhs, n);
    if (!rc) rc = qrd_d2h_2d(p->stream, diag, sizeof(double), sl->dA, sizeof(double) * ((size_t) n + 1), sizeof(double), m);
    if (!rc) rc = qrd_d2h(p->stream, X, sl->dQ, sizeof(double) * (size_t) n * nrhs);
    const int rs = qr_plan_sync(p);
    if (!rc) rc = rs;
    p->guard_latch = latch0;
    qr_host_slot_release(sl);
    for (int i = 0; !rc && i < m; ++i)
        if (diag[i] == 0.0) rc = QR_E_SINGULAR;
    free(diag);
    return rc;
}
