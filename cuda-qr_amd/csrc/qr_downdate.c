/* qr_downdate.c -- row removal: the signed-row update of R and sliding-window least squares (mi355x_qr.h section 6b).
 *
 *   qr_tphqrt_dev       [R ; B] -> [R' ; 0] with the first p_add rows of B added and its last p_del rows removed, panel by panel of 32
 *                       columns: one workgroup factors the panel (qrd_th_panel), one launch updates everything to its right (qrd_th_apply)
 *   qr_tphmqrt_dev      the same transformation applied to [C1 ; C2]: the apply kernel once per panel, forward
 *   qr_lsacc_pop_dev    rows leave the accumulator of qr_update.c;  qr_lsacc_slide_dev: rows enter and leave in one pass
 *   qr_lstsq_rolling    least squares over a moving window on host pointers, through the plan cache of qr_host.c
 *
 * The failure protocol: a removal that leaves no positive-definite triangle sets the plan's device status word in the panel kernel
 * that meets it; every later launch of the call returns at once; the host reads the word once, after the last launch.
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

/* the plan's status word, zeroed on the plan's stream: the start of every call of this section */
static int status_begin(qr_plan* p)
{
    if (!p->hd_status) CHECK(qrd_malloc((void**) &p->hd_status, sizeof(int)));
    return qrd_memset(p->stream, p->hd_status, 0, sizeof(int));
}

/* the one host wait of a call: 0, or QR_E_NOTPD with the failing column + 1 */
static int status_end(qr_plan* p, int* info)
{
    int word = 0;
    CHECK(qrd_d2h(p->stream, &word, p->hd_status, sizeof(int)));
    CHECK(qrd_stream_sync(p->stream));
    if (info) *info = word;
    return word ? QR_E_NOTPD : 0;
}

/* the primitives without the argument checks and without the wait: n is not bounded by a plan */
static int tphqrt_core(qr_plan* pl, double* R, int n, int ldr, double* B, int p_add, int p_del, int ldb, double* T, int ldt)
{
    void* s = pl->stream;
    const int p = p_add + p_del;
    for (int k = 0; k < n; k += QRD_TP_W) {
        const int w = imin(QRD_TP_W, n - k);
        double* Bk = B + (size_t) k * ldb;
        double* Tk = T + (size_t) k * ldt;
        CHECK(qrd_th_panel(s, R + (size_t) k * ldr + k, ldr, Bk, ldb, p, p_add, w, Tk, ldt, k, pl->hd_status));
        CHECK(qrd_th_apply(s, Bk, ldb, p, p_add, w, Tk, ldt, R + (size_t) (k + w) * ldr + k, ldr, Bk + (size_t) w * ldb, ldb, n - k - w,
                           pl->hd_status));
    }
    return 0;
}

static int tphmqrt_core(qr_plan* pl, const double* V, int p_add, int p_del, int n, int ldv, const double* T, int ldt, double* C1, int ldc1,
                        double* C2, int ldc2, int nrhs)
{
    for (int k = 0; k < n; k += QRD_TP_W)
        CHECK(qrd_th_apply(pl->stream, V + (size_t) k * ldv, ldv, p_add + p_del, p_add, imin(QRD_TP_W, n - k), T + (size_t) k * ldt, ldt,
                           C1 + k, ldc1, C2, ldc2, nrhs, pl->hd_status));
    return 0;
}

int qr_tphqrt_dev(qr_plan* p, double* dR, int n, int ldr, double* dB, int p_add, int p_del, int ldb, double* dT, int ldt, int* info)
{
    if (!p || !dR || !dB || !dT || n < 1 || n > p->n || p_add < 0 || p_del < 0 || p_add > QRD_TP_MAXROWS || p_del > QRD_TP_MAXROWS ||
        p_add + p_del < 1 || p_add + p_del > QRD_TP_MAXROWS || ldr < n || ldb < p_add + p_del || ldt < QRD_TP_W)
        return QR_E_ARG;
    CHECK(status_begin(p));
    if (p_del == 0) CHECK(qr_tpqrt_dev(p, dR, n, ldr, dB, p_add, ldb, dT, ldt));      /* S = +I: the row-append update as it stands */
    else CHECK(tphqrt_core(p, dR, n, ldr, dB, p_add, p_del, ldb, dT, ldt));
    return status_end(p, info);
}

int qr_tphmqrt_dev(qr_plan* p, const double* dV, int p_add, int p_del, int n, int ldv, const double* dT, int ldt, double* dC1, int ldc1,
                   double* dC2, int ldc2, int nrhs)
{
    if (!p || !dV || !dT || !dC1 || !dC2 || n < 1 || n > p->n || p_add < 0 || p_del < 0 || p_add > QRD_TP_MAXROWS || p_del > QRD_TP_MAXROWS ||
        p_add + p_del < 1 || p_add + p_del > QRD_TP_MAXROWS || ldv < p_add + p_del || ldt < QRD_TP_W || ldc1 < n || ldc2 < p_add + p_del ||
        nrhs < 1)
        return QR_E_ARG;
    CHECK(status_begin(p));
    return tphmqrt_core(p, dV, p_add, p_del, n, ldv, dT, ldt, dC1, ldc1, dC2, ldc2, nrhs);
}

/* the workspace of pop / slide: Rw (n x n), Zw (n x nrhs), sw (nrhs), Bw (P x n, ld P), Cw (P x nrhs, ld P) */
typedef struct { double *Rw, *Zw, *sw, *Bw, *Cw; } dd_ws;

static int dd_bind(qr_lsacc* a, dd_ws* w)
{
    const size_t n = (size_t) a->n, nrhs = (size_t) a->nrhs, P = QRD_TP_MAXROWS;
    if (!a->dd_buf) CHECK(qrd_malloc((void**) &a->dd_buf, sizeof(double) * (n * n + n * nrhs + nrhs + P * n + P * nrhs)));
    w->Rw = a->dd_buf; w->Zw = w->Rw + n * n; w->sw = w->Zw + n * nrhs; w->Bw = w->sw + nrhs; w->Cw = w->Bw + P * n;
    return 0;
}

/* pnew rows in, pold rows out (either may be 0), on copies; committed only when every block went through */
static int slide_core(qr_lsacc* a, const double* An, int pnew, int ldan, const double* Bn, int ldbn, const double* Ao, int pold, int ldao,
                      const double* Bo, int ldbo)
{
    qr_plan* p = a->p;
    void* s = p->stream;
    const int n = a->n, nrhs = a->nrhs, P = QRD_TP_MAXROWS;
    if (a->rows + pnew - pold < n) return QR_E_NOTPD;      /* no triangle of full rank can remain */
    dd_ws w;
    CHECK(dd_bind(a, &w));
    CHECK(status_begin(p));
    CHECK(qrd_d2d(s, w.Rw, a->R, sizeof(double) * (size_t) n * n));
    CHECK(qrd_d2d(s, w.Zw, a->Z, sizeof(double) * (size_t) n * nrhs));
    CHECK(qrd_d2d(s, w.sw, a->ssq, sizeof(double) * (size_t) nrhs));
    for (int in = 0, io = 0; in < pnew || io < pold;) {
        /* a block takes both kinds, half and half while both last: adding beside removing keeps d away from zero */
        int na = imin(pnew - in, P / 2);
        const int nd = imin(pold - io, P - na);
        na = imin(pnew - in, P - nd);
        if (na) {
            CHECK(qrd_copy_block(s, An + in, ldan, w.Bw, P, na, n));
            CHECK(qrd_copy_block(s, Bn + in, ldbn, w.Cw, P, na, nrhs));
        }
        if (nd) {
            CHECK(qrd_copy_block(s, Ao + io, ldao, w.Bw + na, P, nd, n));
            CHECK(qrd_copy_block(s, Bo + io, ldbo, w.Cw + na, P, nd, nrhs));
        }
        CHECK(tphqrt_core(p, w.Rw, n, n, w.Bw, na, nd, P, a->T, QRD_TP_W));
        CHECK(tphmqrt_core(p, w.Bw, na, nd, n, P, a->T, QRD_TP_W, w.Zw, n, w.Cw, P, nrhs));
        CHECK(qrd_th_colssq(s, w.Cw, P, na + nd, na, nrhs, w.sw, p->hd_status));
        in += na; io += nd;
    }
    CHECK(status_end(p, NULL));
    CHECK(qrd_d2d(s, a->R, w.Rw, sizeof(double) * (size_t) n * n));
    CHECK(qrd_d2d(s, a->Z, w.Zw, sizeof(double) * (size_t) n * nrhs));
    CHECK(qrd_d2d(s, a->ssq, w.sw, sizeof(double) * (size_t) nrhs));
    a->rows += pnew - pold;
    return 0;
}

int qr_lsacc_pop_dev(qr_lsacc* a, const double* dA, int rows, int lda, const double* dB, int ldb)
{
    if (!a || !dA || !dB || rows < 1 || lda < rows || ldb < rows || rows > a->rows) return QR_E_ARG;
    return slide_core(a, NULL, 0, 0, NULL, 0, dA, rows, lda, dB, ldb);
}

int qr_lsacc_slide_dev(qr_lsacc* a, const double* dAnew, int pnew, int ldan, const double* dBnew, int ldbn, const double* dAold, int pold,
                       int ldao, const double* dBold, int ldbo)
{
    if (!a || !dAnew || !dBnew || !dAold || !dBold || pnew < 1 || pold < 1 || ldan < pnew || ldbn < pnew || ldao < pold || ldbo < pold ||
        pold > a->rows)
        return QR_E_ARG;
    return slide_core(a, dAnew, pnew, ldan, dBnew, ldbn, dAold, pold, ldao, dBold, ldbo);
}

int qr_lstsq_rolling(const double* A, long long m, int n, int lda, const double* B, int nrhs, int ldb, int window, int step, double* X,
                     double* resid)
{
    if (!A || !B || !X || n < 1 || m < 1 || nrhs < 1 || window < n || step < 1 || step > window || window > m || lda < m || ldb < m)
        return QR_E_ARG;
    const long long nwin = (m - window) / step + 1;
    host_slot priv, *sl = NULL;
    CHECK(qr_host_slot_acquire(window, n, &priv, &sl));
    qr_plan* p = sl->p;
    const int latch0 = p->guard_latch;
    p->guard_latch = 0;                    /* a blocking entry point: a refused tall panel goes to the leaf chain (as in qr_lstsq) */
    qr_lsacc* a = NULL;
    double* diag = (double*) malloc(sizeof(double) * (size_t) n);
    int rc = diag ? 0 : QR_E_ALLOC;
    const size_t bytes_w = sizeof(double) * (size_t) window, bytes_s = sizeof(double) * (size_t) step;
    const size_t nx = (size_t) n * nrhs;
    /* dQ: the first window's right-hand sides, later [new | old] rows of A and of B at a leading dimension of step;  dR: X and resid */
    size_t need = (size_t) window * nrhs;
    if (need < 2 * (size_t) step * ((size_t) n + nrhs)) need = 2 * (size_t) step * ((size_t) n + nrhs);
    if (!rc) rc = qr_host_slot_need(&sl->dQ, &sl->q_cap, need);
    if (!rc) rc = qr_host_slot_need(&sl->dR, &sl->r_cap, nx + (size_t) nrhs);
    if (!rc) rc = qr_lsacc_create(&a, p, n, nrhs);
    double* dres = sl->dR + nx;
    double *dAn = sl->dQ, *dAo = dAn + (size_t) step * n, *dBn = dAo + (size_t) step * n, *dBo = dBn + (size_t) step * nrhs;
    for (long long k = 0; !rc && k < nwin; ++k) {
        if (k == 0) {
            rc = qrd_h2d_2d(p->stream, sl->dA, bytes_w, A, sizeof(double) * (size_t) lda, bytes_w, n);
            if (!rc) rc = qrd_h2d_2d(p->stream, sl->dQ, bytes_w, B, sizeof(double) * (size_t) ldb, bytes_w, nrhs);
            if (!rc) rc = qr_lsacc_push_dev(a, sl->dA, window, window, sl->dQ, window);
            if (!rc) rc = qrd_d2h_2d(p->stream, diag, sizeof(double), a->R, sizeof(double) * ((size_t) n + 1), sizeof(double), n);
            if (!rc) rc = qr_plan_sync(p);
            for (int i = 0; !rc && i < n; ++i)
                if (diag[i] == 0.0) rc = QR_E_SINGULAR;
        } else {
            const long long o = (k - 1) * step, e = o + window;        /* rows [o, o + step) leave, rows [e, e + step) enter */
            rc = qrd_h2d_2d(p->stream, dAn, bytes_s, A + e, sizeof(double) * (size_t) lda, bytes_s, n);
            if (!rc) rc = qrd_h2d_2d(p->stream, dAo, bytes_s, A + o, sizeof(double) * (size_t) lda, bytes_s, n);
            if (!rc) rc = qrd_h2d_2d(p->stream, dBn, bytes_s, B + e, sizeof(double) * (size_t) ldb, bytes_s, nrhs);
            if (!rc) rc = qrd_h2d_2d(p->stream, dBo, bytes_s, B + o, sizeof(double) * (size_t) ldb, bytes_s, nrhs);
            if (!rc) rc = qr_lsacc_slide_dev(a, dAn, step, step, dBn, step, dAo, step, step, dBo, step);
        }
        if (!rc) rc = qr_lsacc_solve_dev(a, sl->dR, n, dres);
        if (!rc) rc = qrd_d2h(p->stream, X + (size_t) k * nx, sl->dR, sizeof(double) * nx);
        if (!rc && resid) rc = qrd_d2h(p->stream, resid + (size_t) k * nrhs, dres, sizeof(double) * (size_t) nrhs);
    }
    const int rs = qr_plan_sync(p);
    if (!rc) rc = rs;
    if (a) qr_lsacc_destroy(a);
    p->guard_latch = latch0;
    qr_host_slot_release(sl);
    free(diag);
    return rc;
}
