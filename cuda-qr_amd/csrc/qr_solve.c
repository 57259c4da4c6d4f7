/* qr_solve.c -- least-squares solve with the factors of qr_geqrf_dev (mi355x_qr.h section 3).
 *
 *   qr_build_t_dev   T of every outer block (extract V, Gram matrix, larft: the per-panel steps of qr_applyq_dev)
 *   qr_ormqr_dev     Q^T C / Q C panel by panel: for a few right-hand sides on tall panels three VALU launches per panel that read V
 *                    in place from the factored matrix (qrd_ormqr_skinny); else the MFMA products of qr_applyq_dev on the explicit V
 *   qr_solve_r_dev   R X = B: blocked back substitution on 64-row diagonal blocks, one launch per block (qrd_trsm_step); above
 *                    QR_TRSM_SKINNY right-hand sides halves are split recursively and the off-diagonal blocks applied with qrd_gemm_nn
 *   qr_gels_dev      geqrf -> ormqr('T') -> solve_r, all on the plan's stream
 *   qr_lstsq         the same on host pointers, through the plan cache of the host-pointer entry points (qr_host.c)
 *
 * Kept out of qr_host.c on purpose: the sanitizer and order builds of the host schedule link qr_host.c alone against the stub device
 * layer; the units_* builds link every unit against it (tests/c/qrd_stub_units.c holds the launch wrappers called here). */
#define _POSIX_C_SOURCE 200809L
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355x_qr.h"
#include "qr_device.h"
#include "qr_plan_internal.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

/* Routes, from devtools/tools_lstsq_perf.py (profiles/r07_lstsq_perf.txt).  qr_ormqr_dev: the VALU route pays only on tall panels and
 * very few right-hand sides (262144 x 512: 1.71 against 1.93 ms at nrhs 1, 1.81 / 1.94 at 4, 2.43 / 1.97 at 16); on square shapes the
 * MFMA route is faster at every nrhs (16384^2, nrhs 1: 5.5 against 4.6 ms).  qr_solve_r_dev: the one-launch-per-block substitution is
 * faster up to 64 right-hand sides (16384, nrhs 1: 5.2 against 8.7 ms; 64: 8.2 / 9.2; 256: 12.7 / 9.7). */
#define QR_ORMQR_SKINNY 4
#define QR_TRSM_SKINNY 64

/* lab build: MI355XQR_SOLVE_ROUTE = skinny | gemm forces one route (devtools/tools_lstsq_perf.py) */
static int route_forced(void)
{
#ifdef QR_LAB
    const char* e = getenv("MI355XQR_SOLVE_ROUTE");
    if (e && strcmp(e, "skinny") == 0) return 1;
    if (e && strcmp(e, "gemm") == 0) return 0;
#endif
    return -1;
}

static int ormqr_skinny(int m, int n, int nrhs)
{
    const int f = route_forced();
    return f >= 0 ? f : (nrhs <= QR_ORMQR_SKINNY && (long long) m >= 16LL * n);
}

static int trsm_skinny(int nrhs)
{
    const int f = route_forced();
    return f >= 0 ? f : nrhs <= QR_TRSM_SKINNY;
}

static int imin(int a, int b) { return a < b ? a : b; }

static void use_set0(qr_plan* p) { p->Vw = p->Vw2[0]; p->VT = p->VT2[0]; p->T = p->T2[0]; }

/* T of the panel at column k (w columns, mk rows) into T (ldt); V is left in p->Vw.  Tt (ld p->ldt): its transpose, or NULL */
static int panel_t(qr_plan* p, const double* dA, int lda, const double* dtau, int k, int mk, int w, double* T, int ldt, double* Tt)
{
    const double* Ak = dA + (size_t) k * lda + k;
    CHECK(qrd_extract_v(p->stream, Ak, lda, mk, w, p->Vw, p->ldv));
    CHECK(qrd_gemm_tn(p->stream, w, w, mk, 1.0, p->Vw, p->ldv, p->Vw, p->ldv, 0.0, p->G, p->nb, p->slabs, p->slab_cap, NULL, 0));
    return qrd_larft(p->stream, w, p->ib, p->G, p->nb, dtau + k, T, ldt, Tt, 1, p->X, p->nb);
}

int qr_build_t_dev(qr_plan* p, const double* dA, int m, int n, int lda, const double* dtau, double* dT, int ldt)
{
    if (!p || !dA || !dtau || !dT || n < 1 || m < n || m > p->m || n > p->n || lda < m || ldt < p->nb) return QR_E_ARG;
    use_set0(p);
    /* zeros below each block's diagonal: the nb x n block and no more (ldt * n doubles would run ldt - nb past its last column) */
    CHECK(qrd_zero_block(p->stream, dT, ldt, p->nb, n));
    for (int k = 0; k < n; k += p->nb) {
        const int w = imin(p->nb, n - k);
        CHECK(panel_t(p, dA, lda, dtau, k, m - k, w, dT + (size_t) k * ldt, ldt, NULL));
    }
    return 0;
}

int qr_ormqr_dev(qr_plan* p, char trans, const double* dA, int m, int n, int lda, const double* dtau, const double* dT, int ldt,
                 double* dC, int nrhs, int ldc)
{
    const int tr = (trans == 'T' || trans == 't') ? 1 : ((trans == 'N' || trans == 'n') ? 0 : -1);
    if (!p || tr < 0 || !dA || !dtau || !dC || n < 1 || m < n || m > p->m || n > p->n || lda < m || nrhs < 1 || ldc < m ||
        (dT && ldt < p->nb))
        return QR_E_ARG;
    const int nb = p->nb, ldv = p->ldv, npan = (n + nb - 1) / nb;
    const int skinny = ormqr_skinny(m, n, nrhs) && nb <= QRD_SOLVE_MAX_W;
    CHECK(qr_plan_ensure_w(p, skinny ? qrd_ormqr_skinny_ws(m, nb, nrhs) : (size_t) nb * nrhs));
    use_set0(p);
    for (int s = 0; s < npan; ++s) {
        const int pi = tr ? s : npan - 1 - s;             /* Q^T = H_{n-1} .. H_0 applied from panel 0 on; Q from the last panel */
        const int k = pi * nb, w = imin(nb, n - k), mk = m - k;
        const double* Ak = dA + (size_t) k * lda + k;
        double* Cs = dC + k;
        const double* Tk = dT ? dT + (size_t) k * ldt : p->T;
        const int ldtk = dT ? ldt : p->ldt;
        if (skinny) {
            if (!dT) CHECK(panel_t(p, dA, lda, dtau, k, mk, w, p->T, p->ldt, NULL));
            CHECK(qrd_ormqr_skinny(p->stream, Ak, lda, mk, w, Tk, ldtk, tr, Cs, ldc, nrhs, p->W));
            continue;
        }
        /* the MFMA route (qr_applyq_dev's): VT = V op(T)^T, W = VT^T C = op(T) V^T C, C -= V W */
        const double* M = Tk;
        int ldm = ldtk;
        if (!dT) CHECK(panel_t(p, dA, lda, dtau, k, mk, w, p->T, p->ldt, p->Tt));
        else {
            CHECK(qrd_extract_v(p->stream, Ak, lda, mk, w, p->Vw, ldv));
            if (!tr) CHECK(qrd_transpose(p->stream, w, w, Tk, ldt, p->Tt, p->ldt));
        }
        if (!tr) { M = p->Tt; ldm = p->ldt; }
        CHECK(qrd_gemm_nn(p->stream, mk, w, w, 1.0, p->Vw, ldv, M, ldm, 0.0, p->VT, ldv));
        CHECK(qrd_gemm_tn(p->stream, w, nrhs, mk, 1.0, p->VT, ldv, Cs, ldc, 0.0, p->W, w, p->slabs, p->slab_cap, NULL, 0));
        CHECK(qrd_gemm_nn(p->stream, mk, nrhs, w, -1.0, p->Vw, ldv, p->W, w, 1.0, Cs, ldc));
    }
    return 0;
}

/* rows [r0, r1) of the recursive back substitution (wide B): bottom part, one product for the top part's right-hand sides, top part */
static int solve_r_rec(qr_plan* p, const double* R, int lda, double* B, int ldb, int nrhs, int r0, int r1)
{
    if (r1 - r0 <= 64) return qrd_trsm_step(p->stream, R, lda, B, ldb, nrhs, r0, r0, r1, r0, r0);
    const int mid = r0 + ((r1 - r0) / 2 + 63) / 64 * 64;
    CHECK(solve_r_rec(p, R, lda, B, ldb, nrhs, mid, r1));
    CHECK(qrd_gemm_nn(p->stream, mid - r0, nrhs, r1 - mid, -1.0, R + (size_t) mid * lda + r0, lda, B + mid, ldb, 1.0, B + r0, ldb));
    return solve_r_rec(p, R, lda, B, ldb, nrhs, r0, mid);
}

int qr_solve_r_dev(qr_plan* p, const double* dA, int n, int lda, double* dB, int nrhs, int ldb)
{
    if (!p || !dA || !dB || n < 1 || n > p->n || lda < n || nrhs < 1 || ldb < n) return QR_E_ARG;
    if (!trsm_skinny(nrhs)) return solve_r_rec(p, dA, lda, dB, ldb, nrhs, 0, n);
    /* 64-row blocks q = [64 q, 64 q + 64) from the bottom: launch q updates every row above the block below it with that block's
     * solution and solves block q -- one launch per block */
    const int nl = (n + 63) / 64;
    for (int q = nl - 1; q >= 0; --q) {
        const int l0 = 64 * q, l1 = imin(n, l0 + 64);
        const int x0 = l1, x1 = q == nl - 1 ? l1 : imin(n, l1 + 64);
        CHECK(qrd_trsm_step(p->stream, dA, lda, dB, ldb, nrhs, 0, l0, l1, x0, x1));
    }
    return 0;
}

int qr_gels_dev(qr_plan* p, double* dA, int m, int n, int lda, double* dtau, double* dB, int nrhs, int ldb)
{
    if (!p || !dA || !dtau || !dB || n < 1 || m < n || m > p->m || n > p->n || lda < m || nrhs < 1 || ldb < m) return QR_E_ARG;
    CHECK(qr_geqrf_dev(p, dA, m, n, lda, dtau));
    CHECK(qr_ormqr_dev(p, 'T', dA, m, n, lda, dtau, NULL, 0, dB, nrhs, ldb));
    return qr_solve_r_dev(p, dA, n, lda, dB, nrhs, ldb);
}

int qr_lstsq(const double* A, int m, int n, const double* B, int nrhs, double* X, double* resid)
{
    if (!A || !B || !X || n < 1 || m < n || nrhs < 1) return QR_E_ARG;
    host_slot priv, *sl = NULL;
    CHECK(qr_host_slot_acquire(m, n, &priv, &sl));
    qr_plan* p = sl->p;
    const int latch0 = p->guard_latch;
    p->guard_latch = 0;                    /* a blocking entry point: a refused tall panel goes to the leaf chain (as in mmqr_status) */
    const size_t rows_b = (size_t) m;
    double* diag = (double*) malloc(sizeof(double) * (size_t) n);
    double* tail = (m > n && resid) ? (double*) malloc(sizeof(double) * (size_t) (m - n) * nrhs) : NULL;
    int rc = (!diag || (m > n && resid && !tail)) ? QR_E_ALLOC : 0;
    if (!rc) rc = qr_host_slot_need(&sl->dQ, &sl->q_cap, rows_b * nrhs);
    if (!rc) rc = qrd_h2d(p->stream, sl->dA, A, sizeof(double) * (size_t) m * n);
    if (!rc) rc = qrd_h2d(p->stream, sl->dQ, B, sizeof(double) * rows_b * nrhs);
    if (!rc) rc = qr_gels_dev(p, sl->dA, m, n, m, sl->dtau, sl->dQ, nrhs, m);
    if (!rc) rc = qrd_d2h_2d(p->stream, diag, sizeof(double), sl->dA, sizeof(double) * ((size_t) m + 1), sizeof(double), n);
    if (!rc) rc = qrd_d2h_2d(p->stream, X, sizeof(double) * n, sl->dQ, sizeof(double) * rows_b, sizeof(double) * n, nrhs);
    if (!rc && tail) rc = qrd_d2h_2d(p->stream, tail, sizeof(double) * (m - n), sl->dQ + n, sizeof(double) * rows_b,
                                     sizeof(double) * (m - n), nrhs);
    const int rs = qr_plan_sync(p);
    if (!rc) rc = rs;
    p->guard_latch = latch0;
    qr_host_slot_release(sl);
    for (int i = 0; !rc && i < n; ++i)
        if (diag[i] == 0.0) rc = QR_E_SINGULAR;
    if (!rc && resid)
        for (int j = 0; j < nrhs; ++j) {
            double scale = 0.0, ssq = 1.0;   /* scaled sum of squares (LAPACK dnrm2): no overflow for large residuals */
            for (int i = 0; i < m - n; ++i) {
                const double v = fabs(tail[(size_t) j * (m - n) + i]);
                if (v == 0.0) continue;
                if (scale < v) { ssq = 1.0 + ssq * (scale / v) * (scale / v); scale = v; }
                else ssq += (v / scale) * (v / scale);
            }
            resid[j] = scale * sqrt(ssq);
        }
    free(diag);
    free(tail);
    return rc;
}
