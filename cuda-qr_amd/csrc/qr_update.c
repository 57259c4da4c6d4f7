/* qr_update.c -- row-append updating and streaming least squares (mi355x_qr.h section 6).
 *
 *   qr_tpqrt_dev       LAPACK dtpqrt (L = 0): [R ; B] = Q' [R' ; 0] panel by panel of 32 columns: one workgroup factors the panel
 *                      (qrd_tp_panel), one launch of the apply kernel updates everything to its right (qrd_tp_apply)
 *   qr_tpmqrt_dev      LAPACK dtpmqrt (side 'L'): the apply kernel once per panel, forward with T^T for Q'^T, backward with T for Q'
 *   qr_lsacc_*         R, Z = (Q^T b)(0:n) and one sum of squares per right-hand side, updated chunk by chunk
 *   qr_lstsq_chunked   the same on host pointers: one chunk of rows on the device at a time, through the plan cache of qr_host.c
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

static int imin(int a, int b) { return a < b ? a : b; }

int qr_tpqrt_max_rows(void) { return QRD_TP_MAXROWS; }

/* the primitive without the argument checks: n is not bounded by a plan (the accumulator calls it on trailing blocks of its R) */
static int tpqrt_core(void* s, double* R, int n, int ldr, double* B, int p, int ldb, double* T, int ldt)
{
    for (int k = 0; k < n; k += QRD_TP_W) {
        const int w = imin(QRD_TP_W, n - k);
        double* Bk = B + (size_t) k * ldb;
        double* Tk = T + (size_t) k * ldt;
        CHECK(qrd_tp_panel(s, R + (size_t) k * ldr + k, ldr, Bk, ldb, p, w, Tk, ldt));
        CHECK(qrd_tp_apply(s, 1, Bk, ldb, p, w, Tk, ldt, R + (size_t) (k + w) * ldr + k, ldr, Bk + (size_t) w * ldb, ldb, n - k - w));
    }
    return 0;
}

static int tpmqrt_core(void* s, int tr, const double* V, int p, int n, int ldv, const double* T, int ldt, double* C1, int ldc1, double* C2,
                       int ldc2, int nrhs)
{
    const int npan = (n + QRD_TP_W - 1) / QRD_TP_W;
    for (int i = 0; i < npan; ++i) {
        const int k = (tr ? i : npan - 1 - i) * QRD_TP_W;      /* Q'^T = H_{n-1} .. H_0: panel 0 first; Q' from the last panel */
        CHECK(qrd_tp_apply(s, tr, V + (size_t) k * ldv, ldv, p, imin(QRD_TP_W, n - k), T + (size_t) k * ldt, ldt, C1 + k, ldc1, C2, ldc2, nrhs));
    }
    return 0;
}

int qr_tpqrt_dev(qr_plan* p, double* dR, int n, int ldr, double* dB, int rows, int ldb, double* dT, int ldt)
{
    if (!p || !dR || !dB || !dT || n < 1 || n > p->n || rows < 1 || rows > QRD_TP_MAXROWS || ldr < n || ldb < rows || ldt < QRD_TP_W)
        return QR_E_ARG;
    return tpqrt_core(p->stream, dR, n, ldr, dB, rows, ldb, dT, ldt);
}

int qr_tpmqrt_dev(qr_plan* p, char trans, const double* dV, int rows, int n, int ldv, const double* dT, int ldt, double* dC1, int ldc1,
                  double* dC2, int ldc2, int nrhs)
{
    const int tr = (trans == 'T' || trans == 't') ? 1 : ((trans == 'N' || trans == 'n') ? 0 : -1);
    if (!p || tr < 0 || !dV || !dT || !dC1 || !dC2 || n < 1 || n > p->n || rows < 1 || rows > QRD_TP_MAXROWS || ldv < rows ||
        ldt < QRD_TP_W || ldc1 < n || ldc2 < rows || nrhs < 1)
        return QR_E_ARG;
    return tpmqrt_core(p->stream, tr, dV, rows, n, ldv, dT, ldt, dC1, ldc1, dC2, ldc2, nrhs);
}

/* struct qr_lsacc: qr_plan_internal.h (qr_downdate.c works on it as well) */

int qr_lsacc_reset(qr_lsacc* a)
{
    if (!a) return QR_E_ARG;
    const size_t n = (size_t) a->n;
    CHECK(qrd_memset(a->p->stream, a->R, 0, sizeof(double) * n * n));
    CHECK(qrd_memset(a->p->stream, a->Z, 0, sizeof(double) * n * a->nrhs));
    CHECK(qrd_memset(a->p->stream, a->ssq, 0, sizeof(double) * (size_t) a->nrhs));
    a->rows = 0;
    return 0;
}

int qr_lsacc_create(qr_lsacc** out, qr_plan* p, int n, int nrhs)
{
    if (!out || !p || n < 1 || n > p->n || nrhs < 1) return QR_E_ARG;
    qr_lsacc* a = (qr_lsacc*) calloc(1, sizeof(*a));
    if (!a) return QR_E_ALLOC;
    a->p = p; a->n = n; a->nrhs = nrhs;
    const size_t nn = (size_t) n * n, nz = (size_t) n * nrhs, nt = (size_t) QRD_TP_W * n;
    int rc = qrd_malloc((void**) &a->buf, sizeof(double) * (2 * nn + nz + nt + (size_t) n + (size_t) nrhs));
    if (!rc) {
        a->R = a->buf; a->Rc = a->R + nn; a->Z = a->Rc + nn; a->T = a->Z + nz; a->tau = a->T + nt; a->ssq = a->tau + n;
        rc = qr_lsacc_reset(a);
    }
    if (rc) { qrd_free(a->buf); free(a); return rc; }
    *out = a;
    return 0;
}

int qr_lsacc_destroy(qr_lsacc* a)
{
    if (!a) return QR_E_ARG;
    int rc = qrd_stream_sync(a->p->stream);      /* launches that read the buffers may still be queued */
    const int rf = qrd_free(a->buf), rd = qrd_free(a->dd_buf);
    if (!rc) rc = rf;
    if (!rc) rc = rd;
    free(a);
    return rc;
}

int qr_lsacc_rows(qr_lsacc* a, long long* rows)
{
    if (!a || !rows) return QR_E_ARG;
    *rows = a->rows;
    return 0;
}

/* h rows V-to-be (B: h x nn, ldb) against the trailing nn x nn block of R at row / column r0, their right-hand sides (C2: h x nrhs)
 * against rows r0.. of Z; what is left in C2 is orthogonal to everything kept: it goes into the sums of squares */
static int fold_block(qr_lsacc* a, int r0, double* B, int h, int ldb, double* C2, int ldc2)
{
    void* s = a->p->stream;
    const int n = a->n, nn = n - r0;
    double* T = a->T + (size_t) r0 * QRD_TP_W;
    CHECK(tpqrt_core(s, a->R + (size_t) r0 * n + r0, nn, n, B, h, ldb, T, QRD_TP_W));
    CHECK(tpmqrt_core(s, 1, B, h, nn, ldb, T, QRD_TP_W, a->Z + r0, n, C2, ldc2, a->nrhs));
    return qrd_tp_colssq_add(s, C2, ldc2, h, a->nrhs, a->ssq);
}

int qr_lsacc_push_dev(qr_lsacc* a, double* dA, int rows, int lda, double* dB, int ldb)
{
    if (!a || !dA || !dB || rows < 1 || lda < rows || ldb < rows) return QR_E_ARG;
    qr_plan* p = a->p;
    const int n = a->n, nrhs = a->nrhs, P = QRD_TP_MAXROWS;
    if (rows >= n) {
        /* the chunk's own QR, then its triangle in row blocks: block i of an upper-triangular matrix is zero left of column i P, so it
         * meets only the trailing block of R from there on */
        if (rows > p->m) return QR_E_ARG;
        CHECK(qr_geqrf_dev(p, dA, rows, n, lda, a->tau));
        CHECK(qr_ormqr_dev(p, 'T', dA, rows, n, lda, a->tau, NULL, 0, dB, nrhs, ldb));
        CHECK(qrd_tp_colssq_add(p->stream, dB + n, ldb, rows - n, nrhs, a->ssq));
        CHECK(qrd_extract_r(p->stream, dA, lda, rows, n, a->Rc, n, n));
        for (int r0 = 0; r0 < n; r0 += P)
            CHECK(fold_block(a, r0, a->Rc + (size_t) r0 * n + r0, imin(P, n - r0), n, dB + r0, ldb));
    } else {
        for (int r0 = 0; r0 < rows; r0 += P) CHECK(fold_block(a, 0, dA + r0, imin(P, rows - r0), lda, dB + r0, ldb));
    }
    a->rows += rows;
    return 0;
}

int qr_lsacc_factor_dev(qr_lsacc* a, const double** dR, int* ldr, const double** dZ, int* ldz)
{
    if (!a) return QR_E_ARG;
    if (dR) *dR = a->R;
    if (ldr) *ldr = a->n;
    if (dZ) *dZ = a->Z;
    if (ldz) *ldz = a->n;
    return 0;
}

int qr_lsacc_solve_dev(qr_lsacc* a, double* dX, int ldx, double* dresid)
{
    if (!a || !dX || ldx < a->n) return QR_E_ARG;
    qr_plan* p = a->p;
    CHECK(qrd_copy_block(p->stream, a->Z, a->n, dX, ldx, a->n, a->nrhs));
    CHECK(qr_solve_r_dev(p, a->R, a->n, a->n, dX, a->nrhs, ldx));
    if (dresid) CHECK(qrd_tp_sqrt(p->stream, a->ssq, dresid, a->nrhs));
    return 0;
}

int qr_lstsq_chunked(const double* A, long long m, int n, int lda, const double* B, int nrhs, int ldb, int chunk_rows, double* X, double* resid)
{
    if (!A || !B || !X || n < 1 || m < 1 || nrhs < 1 || chunk_rows < 1 || lda < m || ldb < m) return QR_E_ARG;
    if (m < n) return QR_E_SINGULAR;       /* fewer rows than unknowns: R cannot have a full diagonal */
    const int cr = (int) ((long long) chunk_rows < m ? chunk_rows : m);
    host_slot priv, *sl = NULL;
    CHECK(qr_host_slot_acquire(cr > n ? cr : n, n, &priv, &sl));
    qr_plan* p = sl->p;
    const int latch0 = p->guard_latch;
    p->guard_latch = 0;                    /* a blocking entry point: a refused tall panel goes to the leaf chain (as in qr_lstsq) */
    qr_lsacc* a = NULL;
    double* diag = (double*) malloc(sizeof(double) * (size_t) n);
    int rc = diag ? 0 : QR_E_ALLOC;
    if (!rc) rc = qr_host_slot_need(&sl->dQ, &sl->q_cap, (size_t) cr * nrhs);
    if (!rc) rc = qr_host_slot_need(&sl->dR, &sl->r_cap, (size_t) n * nrhs + (size_t) nrhs);
    if (!rc) rc = qr_lsacc_create(&a, p, n, nrhs);
    for (long long r = 0; !rc && r < m; r += cr) {
        const int h = (int) (m - r < cr ? m - r : cr);
        rc = qrd_h2d_2d(p->stream, sl->dA, sizeof(double) * (size_t) h, A + r, sizeof(double) * (size_t) lda, sizeof(double) * (size_t) h, n);
        if (!rc) rc = qrd_h2d_2d(p->stream, sl->dQ, sizeof(double) * (size_t) h, B + r, sizeof(double) * (size_t) ldb, sizeof(double) * (size_t) h, nrhs);
        if (!rc) rc = qr_lsacc_push_dev(a, sl->dA, h, h, sl->dQ, h);
    }
    double* dres = sl->dR + (size_t) n * nrhs;
    if (!rc) rc = qr_lsacc_solve_dev(a, sl->dR, n, dres);
    if (!rc) rc = qrd_d2h_2d(p->stream, diag, sizeof(double), a->R, sizeof(double) * ((size_t) n + 1), sizeof(double), n);
    if (!rc) rc = qrd_d2h(p->stream, X, sl->dR, sizeof(double) * (size_t) n * nrhs);
    if (!rc && resid) rc = qrd_d2h(p->stream, resid, dres, sizeof(double) * (size_t) nrhs);
    const int rs = qr_plan_sync(p);
    if (!rc) rc = rs;
    if (a) qr_lsacc_destroy(a);
    p->guard_latch = latch0;
    qr_host_slot_release(sl);
    for (int i = 0; !rc && i < n; ++i)
        if (diag[i] == 0.0) rc = QR_E_SINGULAR;
    free(diag);
    return rc;
}
