/* qr_batched_update.c -- batched row append / removal and sliding-window least squares (mi355x_qr.h section 8d).
 *
 *   qr_tphqrt_batched_dev / qr_tpqrt_batched_dev   [R ; B] -> [R' ; 0] per member with signed rows, right-hand sides riding along: one
 *                          launch of qrd_bu_update (a wave or a workgroup per member; the route follows from (n + nrhs, p) alone)
 *   qr_tpmqrt_batched_dev  the stored reflectors applied to later right-hand sides: one launch of qrd_bu_apply
 *   qr_lsacc_batched_*     per member R, Z, the residual sums and a row count on the device; push / pop / slide are qrd_bu_update in its
 *                          accumulator mode (inputs read only, no V, no tau), solve is qrd_bu_solve_prep and qrd_b_trsm
 *   qr_lstsq_rolling_batched   the moving-window fit of a packed batch of series on host pointers
 *
 * The plan supplies the stream.  Nothing here waits on the host except the host-pointer twin and destroy.
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

int qr_tpqrt_batched_max_rows(int ncols) { return qrd_bu_max_rows(ncols); }

/* a block of rows x cols beside the others: at least `rows` apart, members at least ld * cols apart (cols == 0: not referenced) */
static int bad_block(const void* ptr, int rows, int cols, int ld, long long stride)
{
    return cols > 0 && (!ptr || ld < rows || stride < (long long) ld * cols);
}

/* n, nrhs and the signed row counts of the fused calls */
static int bad_counts(int n, int nrhs, int p_add, int p_del)
{
    if (n < 1 || nrhs < 0 || nrhs > QR_BATCHED_MAX_N - n || p_add < 0 || p_del < 0) return 1;
    const int cap = qrd_bu_max_rows(n + nrhs);
    return p_add > cap || p_del > cap || p_add + p_del < 1 || p_add + p_del > cap;
}

static int tphqrt_batched(qr_plan* pl, double* dR, int n, int ldr, long long strideR, double* dB, int p_add, int p_del, int ldb,
                          long long strideB, double* dtau, long long stridetau, double* dC1, int ldc1, long long strideC1, double* dC2,
                          int ldc2, long long strideC2, int nrhs, int* dinfo, int batch)
{
    if (!pl || !dtau || batch < 0 || bad_counts(n, nrhs, p_add, p_del) || (p_del > 0 && !dinfo) || stridetau < n) return QR_E_ARG;
    const int p = p_add + p_del;
    if (bad_block(dR, n, n, ldr, strideR) || bad_block(dB, p, n, ldb, strideB) || bad_block(dC1, n, nrhs, ldc1, strideC1) ||
        bad_block(dC2, p, nrhs, ldc2, strideC2))
        return QR_E_ARG;
    if (batch == 0) return 0;
    qrd_bu_args a;
    memset(&a, 0, sizeof a);
    a.R = dR; a.ldr = ldr; a.sR = (size_t) strideR;
    a.tau = dtau; a.stau = (size_t) stridetau;
    a.info = dinfo;
    a.A0 = dB; a.A1 = dB + p_add; a.lda0 = a.lda1 = ldb; a.sA0 = a.sA1 = (size_t) strideB;
    if (nrhs) {
        a.Z = dC1; a.ldz = ldc1; a.sZ = (size_t) strideC1;
        a.C0 = dC2; a.C1 = dC2 + p_add; a.ldc0 = a.ldc1 = ldc2; a.sC0 = a.sC1 = (size_t) strideC2;
    }
    a.n = n; a.nrhs = nrhs; a.p = p; a.p_add = p_add; a.batch = batch; a.acc = 0;
    return qrd_bu_update(pl->stream, &a);
}

int qr_tphqrt_batched_dev(qr_plan* pl, double* dR, int n, int ldr, long long strideR, double* dB, int p_add, int p_del, int ldb,
                          long long strideB, double* dtau, long long stridetau, double* dC1, int ldc1, long long strideC1, double* dC2,
                          int ldc2, long long strideC2, int nrhs, int* dinfo, int batch)
{
    if (!dinfo) return QR_E_ARG;
    return tphqrt_batched(pl, dR, n, ldr, strideR, dB, p_add, p_del, ldb, strideB, dtau, stridetau, dC1, ldc1, strideC1, dC2, ldc2, strideC2,
                          nrhs, dinfo, batch);
}

int qr_tpqrt_batched_dev(qr_plan* pl, double* dR, int n, int ldr, long long strideR, double* dB, int p, int ldb, long long strideB,
                         double* dtau, long long stridetau, double* dC1, int ldc1, long long strideC1, double* dC2, int ldc2,
                         long long strideC2, int nrhs, int batch)
{
    return tphqrt_batched(pl, dR, n, ldr, strideR, dB, p, 0, ldb, strideB, dtau, stridetau, dC1, ldc1, strideC1, dC2, ldc2, strideC2, nrhs,
                          NULL, batch);
}

int qr_tpmqrt_batched_dev(qr_plan* pl, char trans, const double* dV, int p_add, int p_del, int n, int ldv, long long strideV,
                          const double* dtau, long long stridetau, double* dC1, int ldc1, long long strideC1, double* dC2, int ldc2,
                          long long strideC2, int nrhs, int batch)
{
    if (!pl || !dtau || (trans != 'T' && trans != 'N') || batch < 0 || nrhs < 1 || bad_counts(n, 0, p_add, p_del) || stridetau < n ||
        (trans == 'N' && p_del > 0))
        return QR_E_ARG;
    const int p = p_add + p_del;
    if (bad_block(dV, p, n, ldv, strideV) || bad_block(dC1, n, nrhs, ldc1, strideC1) || bad_block(dC2, p, nrhs, ldc2, strideC2))
        return QR_E_ARG;
    if (batch == 0) return 0;
    return qrd_bu_apply(pl->stream, trans == 'T', dV, p, p_add, n, ldv, (size_t) strideV, dtau, (size_t) stridetau, dC1, ldc1,
                        (size_t) strideC1, dC2, ldc2, (size_t) strideC2, nrhs, batch);
}

/* ---- the accumulator: per member R (n x n, ld n), Z (n x nrhs, ld n), rss (nrhs), one row count, all on the device (struct
 * qr_lsacc_batched: qr_plan_internal.h) ---- */

static size_t acc_doubles(const qr_lsacc_batched* a)
{
    return (size_t) a->batch * ((size_t) a->n * a->n + (size_t) a->n * a->nrhs + (size_t) a->nrhs);
}

int qr_lsacc_batched_reset(qr_lsacc_batched* a)
{
    if (!a) return QR_E_ARG;
    if (a->batch == 0) return 0;
    CHECK(qrd_memset(a->p->stream, a->R, 0, sizeof(double) * acc_doubles(a)));
    return qrd_memset(a->p->stream, a->rows, 0, sizeof(int) * (size_t) a->batch);
}

int qr_lsacc_batched_create(qr_lsacc_batched** out, qr_plan* p, int n, int nrhs, int batch)
{
    if (!out || !p || n < 1 || nrhs < 1 || nrhs > QR_BATCHED_MAX_N - n || batch < 0) return QR_E_ARG;
    qr_lsacc_batched* a = (qr_lsacc_batched*) calloc(1, sizeof *a);
    if (!a) return QR_E_ALLOC;
    a->p = p; a->n = n; a->nrhs = nrhs; a->batch = batch;
    int rc = 0;
    if (batch > 0) {
        rc = qrd_malloc((void**) &a->R, sizeof(double) * acc_doubles(a));
        if (!rc) rc = qrd_malloc((void**) &a->rows, sizeof(int) * (size_t) batch);
        if (!rc) {
            a->Z = a->R + (size_t) batch * n * n;
            a->rss = a->Z + (size_t) batch * n * nrhs;
            rc = qr_lsacc_batched_reset(a);
        }
    }
    if (rc) {
        if (a->rows) qrd_free(a->rows);
        if (a->R) qrd_free(a->R);
        free(a);
        return rc;
    }
    *out = a;
    return 0;
}

int qr_lsacc_batched_destroy(qr_lsacc_batched* a)
{
    if (!a) return QR_E_ARG;
    int rc = 0;
    if (a->batch > 0) {
        rc = qrd_stream_sync(a->p->stream);
        qrd_free(a->rows);
        qrd_free(a->R);
    }
    free(a);
    return rc;
}

/* one launch: rows [0, pa) from (An, Bn), rows [pa, pa + pd) from (Ao, Bo); the inputs are read only (the device layer's argument
 * block has one pointer type for both modes) */
static int acc_update(qr_lsacc_batched* a, const double* An, int pa, int ldan, long long san, const double* Bn, int ldbn, long long sbn,
                      const double* Ao, int pd, int ldao, long long sao, const double* Bo, int ldbo, long long sbo, int* dinfo)
{
    qrd_bu_args u;
    memset(&u, 0, sizeof u);
    const size_t n = (size_t) a->n, nrhs = (size_t) a->nrhs;
    u.R = a->R; u.ldr = a->n; u.sR = n * n;
    u.Z = a->Z; u.ldz = a->n; u.sZ = n * nrhs;
    u.rss = a->rss; u.rows = a->rows; u.info = dinfo;
    u.A0 = (double*) An; u.lda0 = ldan; u.sA0 = (size_t) san; u.C0 = (double*) Bn; u.ldc0 = ldbn; u.sC0 = (size_t) sbn;
    u.A1 = (double*) Ao; u.lda1 = ldao; u.sA1 = (size_t) sao; u.C1 = (double*) Bo; u.ldc1 = ldbo; u.sC1 = (size_t) sbo;
    u.n = a->n; u.nrhs = a->nrhs; u.p = pa + pd; u.p_add = pa; u.batch = a->batch; u.acc = 1;
    return qrd_bu_update(a->p->stream, &u);
}

int qr_lsacc_batched_push_dev(qr_lsacc_batched* a, const double* dA, int p, int lda, long long strideA, const double* dB, int ldb,
                              long long strideB)
{
    if (!a || p < 1 || bad_block(dA, p, a->n, lda, strideA) || bad_block(dB, p, a->nrhs, ldb, strideB)) return QR_E_ARG;
    if (a->batch == 0) return 0;
    const int cap = qrd_bu_max_rows(a->n + a->nrhs);
    for (int i = 0; i < p; i += cap) {       /* a push cannot fail: its row blocks are committed one by one */
        const int pb = p - i < cap ? p - i : cap;
        CHECK(acc_update(a, dA + i, pb, lda, strideA, dB + i, ldb, strideB, NULL, 0, 0, 0, NULL, 0, 0, NULL));
    }
    return 0;
}

int qr_lsacc_batched_pop_dev(qr_lsacc_batched* a, const double* dA, int p, int lda, long long strideA, const double* dB, int ldb,
                             long long strideB, int* dinfo)
{
    if (!a || !dinfo || p < 1 || p > qrd_bu_max_rows(a->n + a->nrhs) || bad_block(dA, p, a->n, lda, strideA) ||
        bad_block(dB, p, a->nrhs, ldb, strideB))
        return QR_E_ARG;
    if (a->batch == 0) return 0;
    return acc_update(a, NULL, 0, 0, 0, NULL, 0, 0, dA, p, lda, strideA, dB, ldb, strideB, dinfo);
}

int qr_lsacc_batched_slide_dev(qr_lsacc_batched* a, const double* dAnew, int pnew, int ldan, long long strideAn, const double* dBnew,
                               int ldbn, long long strideBn, const double* dAold, int pold, int ldao, long long strideAo,
                               const double* dBold, int ldbo, long long strideBo, int* dinfo)
{
    if (!a || !dinfo || pnew < 1 || pold < 1) return QR_E_ARG;
    const int cap = qrd_bu_max_rows(a->n + a->nrhs);
    if (pnew > cap || pold > cap || pnew + pold > cap || bad_block(dAnew, pnew, a->n, ldan, strideAn) ||
        bad_block(dBnew, pnew, a->nrhs, ldbn, strideBn) || bad_block(dAold, pold, a->n, ldao, strideAo) ||
        bad_block(dBold, pold, a->nrhs, ldbo, strideBo))
        return QR_E_ARG;
    if (a->batch == 0) return 0;
    return acc_update(a, dAnew, pnew, ldan, strideAn, dBnew, ldbn, strideBn, dAold, pold, ldao, strideAo, dBold, ldbo, strideBo, dinfo);
}

int qr_lsacc_batched_factor_dev(qr_lsacc_batched* a, const double** dR, int* ldr, long long* strideR, const double** dZ, int* ldz,
                                long long* strideZ, const double** drss, const int** drows)
{
    if (!a) return QR_E_ARG;
    if (dR) *dR = a->R;
    if (ldr) *ldr = a->n;
    if (strideR) *strideR = (long long) a->n * a->n;
    if (dZ) *dZ = a->Z;
    if (ldz) *ldz = a->n;
    if (strideZ) *strideZ = (long long) a->n * a->nrhs;
    if (drss) *drss = a->rss;
    if (drows) *drows = a->rows;
    return 0;
}

int qr_lsacc_batched_solve_dev(qr_lsacc_batched* a, double* dX, int ldx, long long strideX, double* dresid, long long strideresid, int* dinfo)
{
    if (!a || !dinfo || bad_block(dX, a->n, a->nrhs, ldx, strideX) || (dresid && strideresid < a->nrhs)) return QR_E_ARG;
    if (a->batch == 0) return 0;
    void* s = a->p->stream;
    CHECK(qrd_bu_solve_prep(s, a->Z, a->n, a->nrhs, dX, ldx, (size_t) strideX, a->rss, dresid, (size_t) strideresid, a->batch));
    return qrd_b_trsm(s, a->R, a->n, a->n, (size_t) a->n * a->n, dX, a->nrhs, ldx, (size_t) strideX, dinfo, a->batch);
}

/* ---- the host-pointer twin: staged as qr_stage.h describes; the accumulator borrows the stage's plan ---- */
int qr_lstsq_rolling_batched(const double* A, int m, int n, const double* B, int nrhs, int batch, int window, int step, double* X,
                             double* resid, int* info)
{
    if (!A || !B || !X || !info || n < 1 || m < 1 || nrhs < 1 || nrhs > QR_BATCHED_MAX_N - n || batch < 0 || window < n || step < 1 ||
        step > window || window > m || 2 * (long long) step > qrd_bu_max_rows(n + nrhs))
        return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t nwin = (size_t) ((m - window) / step + 1), nb = (size_t) batch, nx = (size_t) n * nrhs;
    const size_t mn = (size_t) m * n, mr = (size_t) m * nrhs;
    int* hi = (int*) malloc(sizeof(int) * 2 * nwin * nb);
    if (!hi) return QR_E_ALLOC;
    qr_lsacc_batched* a = NULL;
    double *dA, *dB, *dX, *dres;
    int* di;
    qr_stage_buf t[] = { QR_STAGE_F64(dA, nb * mn, A, NULL, 0), QR_STAGE_F64(dB, nb * mr, B, NULL, 0), QR_STAGE_F64(dX, nb * nwin * nx, NULL, X, 0),
                         QR_STAGE_F64(dres, nb * nwin * (size_t) nrhs, NULL, resid, 0), QR_STAGE_I32(di, 2 * nwin * nb, NULL, hi, 1) };
    qr_stage st;
    int rc = qr_stage_open(&st, window, n, t, QR_STAGE_COUNT(t));
    if (!rc) rc = qr_lsacc_batched_create(&a, st.plan, n, nrhs, batch);
    /* di: window k's update words at [k * batch, ..), its solve words nwin * batch further on */
    for (size_t k = 0; !rc && k < nwin; ++k) {
        if (k == 0) rc = qr_lsacc_batched_push_dev(a, dA, window, m, (long long) mn, dB, m, (long long) mr);
        else {
            const size_t o = (k - 1) * (size_t) step, e = o + (size_t) window;     /* rows [o, o + step) leave, rows [e, e + step) enter */
            rc = qr_lsacc_batched_slide_dev(a, dA + e, step, m, (long long) mn, dB + e, m, (long long) mr, dA + o, step, m, (long long) mn,
                                            dB + o, m, (long long) mr, di + k * nb);
        }
        if (!rc)
            rc = qr_lsacc_batched_solve_dev(a, dX + k * nx, n, (long long) (nwin * nx), dres + k * (size_t) nrhs,
                                            (long long) (nwin * (size_t) nrhs), di + (nwin + k) * nb);
    }
    rc = qr_stage_fetch(&st, rc);
    if (!rc) {
        int notpd = 0, sing = 0;
        for (size_t q = 0; q < nb; ++q)
            for (size_t k = 0; k < nwin; ++k) {
                const int up = hi[k * nb + q], so = hi[(nwin + k) * nb + q];
                info[q * nwin + k] = up ? up : so;
                if (up) notpd = 1;
                else if (so) sing = 1;
            }
        rc = notpd ? QR_E_NOTPD : (sing ? QR_E_SINGULAR : 0);
    }
    if (a) qr_lsacc_batched_destroy(a);
    qr_stage_close(&st);
    free(hi);
    return rc;
}
