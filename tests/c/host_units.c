/* host_units.c -- TEST-ONLY driver of the seventeen per-interface host units (qr_solve.c ... qr_batched_lm.c, which holds sections 8m and 8n) over the stub device layer
 * (qrd_stub.c, qrd_stub_units.c; tests/test_units_stub.py; DESIGN "Host units over the stub").  One named configuration per process, as
 * in host_order.c: `host_units list` prints the names, `host_units <name>` runs one, `host_units threads` runs four host threads on
 * different host-pointer twins (the ThreadSanitizer build).  Every caller-side device buffer is allocated at exactly the minimum size the
 * public header documents for the leading dimensions and strides passed -- odd leading dimensions, strides with a gap -- so that a launch
 * handed a wrong count falls outside it.  The run ends with
 *   ORDER <reports>   LAUNCHES <n>   FAILHITS <n>   and one line per allocation the library made, in call order:  ALLOC <k> <bytes> <function>:<expression>
 * QRD_STUB_FAIL_MALLOC=k / QRD_STUB_SHRINK_MALLOC=k (qrd_stub.c) make the k-th of those fail / come out 8 bytes short. */
#define _POSIX_C_SOURCE 200809L
#include <limits.h>
#include <math.h>
#include "host_drive.h"

static void* g_host_buf[256];
static int g_host_nbuf;
static void* hostz(size_t bytes)
{
    void* p = calloc(1, bytes ? bytes : 8);
    if (!p || g_host_nbuf == 256) { fprintf(stderr, "driver: out of host buffers\n"); exit(1); }
    return g_host_buf[g_host_nbuf++] = p;
}
static double* hostd(size_t n) { return (double*) hostz(sizeof(double) * n); }
static int* hosti(size_t n) { return (int*) hostz(sizeof(int) * n); }
/* a packed batch of rows x cols matrices with d on the diagonals */
static double* host_mats(int rows, int cols, int batch, double d)
{
    double* A = hostd((size_t) rows * cols * batch);
    for (int q = 0; q < batch; ++q)
        for (int i = 0; i < rows && i < cols; ++i) A[((size_t) q * cols + i) * rows + i] = d;
    return A;
}
/* the stub's device memory is host memory: the driver may put a diagonal into a "device" matrix */
static void poke_diag(double* A, int ld, int n, double d) { for (int i = 0; i < n; ++i) A[(size_t) i * ld + i] = d; }
static const int g_nrhs_classes[] = {1, 4, 5, 16, 17};

/* ================================================= qr_solve.c ================================================= */
static void solve_on(int pm, int pn, int nb, int m, int n, const int* nrhs_list, int count)
{
    qr_plan* p = NULL;
    CALL(qr_plan_create(&p, pm, pn, nb, 0));
    int pnb = 0;
    const int lda = m + 1;
    double *A = dev_block(m, n, lda), *tau = dev_vec(n);
    CALL(qr_geqrf_dev(p, A, m, n, lda, tau));
    /* the plan's block size: dT is nbp x n at ldt >= nbp */
    { int ib, la; CALL(qr_plan_info(p, &pnb, &ib, &la)); }
    const int ldt = pnb + 1;
    double* T = dev_block(pnb, n, ldt);
    CALL(qr_build_t_dev(p, A, m, n, lda, tau, T, ldt));
    for (int i = 0; i < count; ++i) {
        const int nrhs = nrhs_list[i], ldb = m + 3;
        double* B = dev_block(m, nrhs, ldb);
        CALL(qr_ormqr_dev(p, 'T', A, m, n, lda, tau, T, ldt, B, nrhs, ldb));
        CALL(qr_ormqr_dev(p, 'T', A, m, n, lda, tau, NULL, 0, B, nrhs, ldb));
        CALL(qr_ormqr_dev(p, 'N', A, m, n, lda, tau, T, ldt, B, nrhs, ldb));
        CALL(qr_ormqr_dev(p, 'n', A, m, n, lda, tau, NULL, 0, B, nrhs, ldb));
        CALL(qr_solve_r_dev(p, A, n, lda, B, nrhs, ldb));
        CALL(qr_gels_dev(p, A, m, n, lda, tau, B, nrhs, ldb));
        CALL(qr_gels_dev(p, A, m, n, lda, tau, B, nrhs, ldb));      /* the second call reuses the grown workspace */
        ARG(qr_ormqr_dev(p, 'X', A, m, n, lda, tau, NULL, 0, B, nrhs, ldb));
        ARG(qr_ormqr_dev(p, 'T', A, m, n, lda, tau, T, pnb - 1, B, nrhs, ldb));
        ARG(qr_ormqr_dev(p, 'T', A, m, n, lda, tau, NULL, 0, B, nrhs, m - 1));
        ARG(qr_solve_r_dev(p, A, n, n - 1, B, nrhs, ldb));
        ARG(qr_gels_dev(p, A, m, n, lda, tau, B, 0, ldb));
    }
    ARG(qr_build_t_dev(p, A, m, n, lda, tau, T, pnb - 1));
    ARG(qr_build_t_dev(p, A, pm + 1, n, pm + 1, tau, T, ldt));
    ARG(qr_solve_r_dev(p, A, pn + 1, lda, A, 1, lda));
    CALL(qr_plan_sync(p));
    CALL(qr_plan_destroy(p));
}
static void solve_tall(void) { solve_on(528, 33, 32, 528, 33, g_nrhs_classes, 5); }                  /* m >= 16 n: the VALU route up to 4 right-hand sides */
static void solve_short(void) { const int l[] = {1, 4, 5}; solve_on(200, 70, 32, 200, 70, l, 3); }  /* m < 16 n: the MFMA route at every nrhs */
static void solve_aligned(void) { const int l[] = {5}; solve_on(256, 64, 32, 256, 64, l, 1); }          /* m a multiple of 128: V T fills its buffer to the last element */
static void solve_blocks(void) { const int l[] = {1, 64, 65}; solve_on(2096, 130, 64, 2096, 130, l, 3); }   /* three 64-row blocks; 65: the recursion */
static void solve_subplan(void) { const int l[] = {4, 17}; solve_on(1056, 66, 32, 528, 33, l, 2); }  /* a plan made for a larger shape */
static void solve_twin(void)
{
    const int m = 40, n = 7;
    double *A1 = host_mats(m, n, 1, 1.0), *A0 = host_mats(m, n, 1, 0.0), *B = hostd((size_t) m * 17), *X = hostd((size_t) n * 17), *res = hostd(17);
    CALL(qr_lstsq(A1, m, n, B, 1, X, res));
    CALL(qr_lstsq(A1, m, n, B, 17, X, NULL));                 /* the cached slot grows its right-hand-side buffer */
    CALL(qr_lstsq(A1, m, n, B, 5, X, res));
    CALLX(qr_lstsq(A0, m, n, B, 4, X, res), QR_E_SINGULAR);   /* a zero on R's diagonal (the stub leaves what was uploaded) */
    CALL(qr_lstsq(host_mats(n, n, 1, 1.0), n, n, B, 16, X, res));      /* square: no tail rows */
    ARG(qr_lstsq(A1, n - 1, n, B, 1, X, res));
    ARG(qr_lstsq(NULL, m, n, B, 1, X, res));
    ARG(qr_lstsq(A1, m, n, B, 0, X, res));
}

/* ================================================= qr_pivot.c ================================================= */
static void fill_script(const char* entry, double v, int n) { double q[128]; for (int i = 0; i < n; ++i) q[i] = v; qrd_stub_script(entry, q, n); }
static void pivot_on(int pm, int pn, int nb, int m, int n)
{
    qr_plan* p = NULL;
    CALL(qr_plan_create(&p, pm, pn, nb, 0));
    const int lda = m + (m % 2 ? 2 : 1);
    double *A = dev_block(m, n, lda), *tau = dev_vec(n);
    int* jp = dev_ints(n);
    CALL(qr_geqp3_dev(p, A, m, n, lda, jp, tau));
    CALL(qr_geqp3_dev(p, A, m, n, lda, jp, tau));
    /* every column of the first panel reports an early end after 5 columns; the recomputed norms end the next one after 3 */
    CALLS(fill_script("pivot_column", 5.0, 32), qr_geqp3_dev(p, A, m, n, lda, jp, tau), 0);
    fill_script("pivot_column", 0.0, 0);
    { const double q[2] = {(double) INT_MAX, 3.0}; CALLS(qrd_stub_script("pivot_norms", q, 2), qr_geqp3_dev(p, A, m, n, lda, jp, tau), 0); }
    qrd_stub_script("pivot_norms", NULL, 0);
    CALLS(fill_script("pivot_column", 0.0, 32), qr_geqp3_dev(p, A, m, n, lda, jp, tau), QR_E_INTERNAL);      /* a panel that factored nothing */
    fill_script("pivot_column", 0.0, 0);
    int rank = -1;
    CALL(qr_rank_dev(p, A, m, n, lda, -1.0, &rank));
    if (rank != 0) { fprintf(stderr, "rank %d of a zero diagonal\n", rank); exit(1); }
    for (int i = 0; i < 5; ++i) {
        const int nrhs = g_nrhs_classes[i], ldb = m + 3;
        double *B = dev_block(m, nrhs, ldb), *res = dev_vec(nrhs);
        CALL(qr_gelsp_dev(p, A, m, n, lda, jp, tau, B, nrhs, ldb, -1.0, res, &rank));            /* rank 0: no triangular solve */
        poke_diag(A, lda, n, 1.0);
        CALL(qr_gelsp_dev(p, A, m, n, lda, jp, tau, B, nrhs, ldb, 0.5, NULL, NULL));
        CALL(qr_rank_dev(p, A, m, n, lda, 0.5, &rank));
        if (rank != n) { fprintf(stderr, "rank %d of a unit diagonal\n", rank); exit(1); }
        poke_diag(A, lda, n, 0.0);
        ARG(qr_gelsp_dev(p, A, m, n, lda, jp, tau, B, nrhs, m - 1, -1.0, res, &rank));
    }
    ARG(qr_geqp3_dev(p, A, m, n, m - 1, jp, tau));
    ARG(qr_geqp3_dev(p, A, m, n, lda, NULL, tau));
    ARG(qr_rank_dev(p, A, m, n, lda, -1.0, NULL));
    CALL(qr_plan_sync(p));
    CALL(qr_plan_destroy(p));
}
static void pivot_general(void) { pivot_on(300, 70, 32, 300, 70); }       /* ragged: the block update goes through F^T and the general product */
static void pivot_nt(void) { pivot_on(160, 160, 32, 160, 160); }          /* 128 x 128 trailing block: qrd_gemm_nt */
static void pivot_subplan(void) { pivot_on(400, 300, 32, 300, 70); }      /* the workspace is bound for the plan's n, two candidate blocks */
static void pivot_twin(void)
{
    const int m = 40, n = 7;
    double *A1 = host_mats(m, n, 1, 1.0), *B = hostd((size_t) m * 17), *X = hostd((size_t) n * 17), *res = hostd(17);
    int rank = 0, *jp = hosti(n);
    CALL(qr_lstsq_pivoted(A1, m, n, B, 1, -1.0, X, res, &rank, jp));
    CALL(qr_lstsq_pivoted(A1, m, n, B, 17, -1.0, X, NULL, NULL, NULL));
    CALL(qr_lstsq_pivoted(A1, m, n, B, 4, 0.1, X, res, NULL, jp));
    ARG(qr_lstsq_pivoted(A1, n - 1, n, B, 1, -1.0, X, res, &rank, jp));
    ARG(qr_lstsq_pivoted(A1, m, n, NULL, 1, -1.0, X, res, &rank, jp));
}

/* ================================================= qr_minnorm.c ================================================= */
static void minnorm_on(int pm, int pn, int nb, int m, int n, const int* nrhs_list, int count)
{
    qr_plan* p = NULL;
    CALL(qr_plan_create(&p, pm, pn, nb, 0));
    int pnb = 0;
    { int ib, la; CALL(qr_plan_info(p, &pnb, &ib, &la)); }
    const int lda = m + 1, ldt = pnb + 2, ldw = n + 1;
    double *A = dev_block(m, n, lda), *tau = dev_vec(n), *T = dev_block(pnb, n, ldt), *Aw = dev_block(n, m, ldw);
    CALL(qr_geqrf_dev(p, A, m, n, lda, tau));
    CALL(qr_build_t_dev(p, A, m, n, lda, tau, T, ldt));
    for (int i = 0; i < count; ++i) {
        const int nrhs = nrhs_list[i], ldb = m + 3;
        double* B = dev_block(m, nrhs, ldb);
        CALL(qr_solve_rt_dev(p, A, n, lda, B, nrhs, ldb));
        CALL(qr_minnorm_dev(p, A, m, n, lda, tau, T, ldt, B, nrhs, ldb));
        CALL(qr_minnorm_dev(p, A, m, n, lda, tau, NULL, 0, B, nrhs, ldb));
        CALL(qr_gels_t_dev(p, A, m, n, lda, tau, B, nrhs, ldb));
        CALL(qr_gels_wide_dev(p, Aw, n, m, ldw, A, lda, tau, B, nrhs, ldb));      /* the wide matrix n x m, its transpose factored in A */
        ARG(qr_solve_rt_dev(p, A, n, lda, B, nrhs, n - 1));
        ARG(qr_minnorm_dev(p, A, m, n, lda, tau, T, pnb - 1, B, nrhs, ldb));
        ARG(qr_gels_t_dev(p, A, m, n, lda, tau, B, nrhs, m - 1));
        ARG(qr_gels_wide_dev(p, Aw, n, m, n - 1, A, lda, tau, B, nrhs, ldb));
    }
    CALL(qr_transpose_dev(p, Aw, n, m, ldw, A, lda));
    ARG(qr_transpose_dev(p, Aw, n, m, ldw, A, m - 1));
    CALL(qr_plan_sync(p));
    CALL(qr_plan_destroy(p));
}
static void minnorm_tall(void) { minnorm_on(528, 33, 32, 528, 33, g_nrhs_classes, 5); }
static void minnorm_blocks(void) { const int l[] = {1, 64, 65}; minnorm_on(2096, 130, 64, 2096, 130, l, 3); }
static void minnorm_subplan(void) { const int l[] = {4, 17}; minnorm_on(1056, 66, 32, 528, 33, l, 2); }
static void minnorm_twin(void)
{
    const int m = 7, n = 40;
    double *A1 = host_mats(m, n, 1, 1.0), *A0 = host_mats(m, n, 1, 0.0), *B = hostd((size_t) m * 17), *X = hostd((size_t) n * 17);
    CALL(qr_lstsq_minnorm(A1, m, n, B, 1, X));
    CALL(qr_lstsq_minnorm(A1, m, n, B, 17, X));
    CALLX(qr_lstsq_minnorm(A0, m, n, B, 5, X), QR_E_SINGULAR);
    CALL(qr_lstsq_minnorm(host_mats(m, m, 1, 1.0), m, m, B, 4, X));
    ARG(qr_lstsq_minnorm(A1, n + 1, n, B, 1, X));
    ARG(qr_lstsq_minnorm(A1, m, n, B, 1, NULL));
}

/* ================================================= qr_update.c, qr_downdate.c ================================================= */
static void update_primitives(void)
{
    qr_plan* p = NULL;
    const int n = 70, P = qr_tpqrt_max_rows();
    CALL(qr_plan_create(&p, 528, n, 32, 0));
    const int ldr = n + 1, ldt = QR_TPQRT_PANEL + 1;
    double *R = dev_block(n, n, ldr), *T = dev_block(QR_TPQRT_PANEL, n, ldt);
    const int rows_list[] = {1, 37, P};
    for (int i = 0; i < 3; ++i) {
        const int rows = rows_list[i], ldb = rows + 1;
        double* B = dev_block(rows, n, ldb);
        CALL(qr_tpqrt_dev(p, R, n, ldr, B, rows, ldb, T, ldt));
        CALL(qr_tpqrt_dev(p, R, 32, ldr, B, rows, ldb, T, ldt));      /* one whole panel: nothing to its right */
        for (int k = 0; k < 5; ++k) {
            const int nrhs = g_nrhs_classes[k], ldc1 = n + 2, ldc2 = rows + 2;
            double *C1 = dev_block(n, nrhs, ldc1), *C2 = dev_block(rows, nrhs, ldc2);
            CALL(qr_tpmqrt_dev(p, 'T', B, rows, n, ldb, T, ldt, C1, ldc1, C2, ldc2, nrhs));
            CALL(qr_tpmqrt_dev(p, 'N', B, rows, n, ldb, T, ldt, C1, ldc1, C2, ldc2, nrhs));
            ARG(qr_tpmqrt_dev(p, 'T', B, rows, n, ldb, T, ldt, C1, n - 1, C2, ldc2, nrhs));
            ARG(qr_tpmqrt_dev(p, 'Q', B, rows, n, ldb, T, ldt, C1, ldc1, C2, ldc2, nrhs));
        }
        ARG(qr_tpqrt_dev(p, R, n, ldr, B, rows, rows - 1, T, ldt));
    }
    ARG(qr_tpqrt_dev(p, R, n, ldr, R, P + 1, P + 1, T, ldt));
    ARG(qr_tpqrt_dev(p, R, n, ldr, R, 0, 1, T, ldt));
    ARG(qr_tpqrt_dev(p, R, n, ldr, R, 1, 1, T, QR_TPQRT_PANEL - 1));
    CALL(qr_plan_sync(p));
    CALL(qr_plan_destroy(p));
}
/* the accumulator: chunks shorter than n, of more than one row block, and taller than n; then rows leave and slide */
static void lsacc_on(int pm, int pn, int nb, int n, int nrhs, int short_rows, int tall_rows)
{
    qr_plan* p = NULL;
    qr_lsacc* a = NULL;
    CALL(qr_plan_create(&p, pm, pn, nb, 0));
    CALL(qr_lsacc_create(&a, p, n, nrhs));
    const int big = tall_rows > short_rows ? tall_rows : short_rows, lda = big + 1, ldb = big + 3, ldx = n + 1;
    double *A = dev_block(big, n, lda), *B = dev_block(big, nrhs, ldb), *X = dev_block(n, nrhs, ldx), *res = dev_vec(nrhs);
    CALL(qr_lsacc_push_dev(a, A, short_rows, lda, B, ldb));
    CALL(qr_lsacc_push_dev(a, A, tall_rows, lda, B, ldb));
    CALL(qr_lsacc_push_dev(a, A, 1, lda, B, ldb));
    long long rows = 0;
    CALL(qr_lsacc_rows(a, &rows));
    if (rows != short_rows + tall_rows + 1) { fprintf(stderr, "accumulator rows %lld\n", rows); exit(1); }
    const double *fR = NULL, *fZ = NULL;
    int fldr = 0, fldz = 0;
    CALL(qr_lsacc_factor_dev(a, &fR, &fldr, &fZ, &fldz));
    CALL(qr_lsacc_factor_dev(a, NULL, NULL, NULL, NULL));
    CALL(qr_lsacc_solve_dev(a, X, ldx, res));
    CALL(qr_lsacc_solve_dev(a, X, ldx, NULL));
    ARG(qr_lsacc_push_dev(a, A, 0, lda, B, ldb));
    ARG(qr_lsacc_push_dev(a, A, short_rows, short_rows - 1, B, ldb));
    ARG(qr_lsacc_push_dev(a, A, pm + 16 + n, pm + 16 + n, B, pm + 16 + n));          /* a chunk taller than the plan */
    ARG(qr_lsacc_solve_dev(a, X, n - 1, res));
    /* rows leave: 0 added and the row limit removed in one block; more than a block; beside new rows */
    const int P = qr_tpqrt_max_rows();
    const int po = big < P ? big : P;
    CALL(qr_lsacc_pop_dev(a, A, 1, lda, B, ldb));
    CALL(qr_lsacc_pop_dev(a, A, po, lda, B, ldb));
    CALL(qr_lsacc_slide_dev(a, A, po, lda, B, ldb, A, n < 40 ? 40 : po, lda, B, ldb));
    CALL(qr_lsacc_slide_dev(a, A, 3, lda, B, ldb, A, 1, lda, B, ldb));
    if (big > P) CALL(qr_lsacc_slide_dev(a, A, big, lda, B, ldb, A, P + 5, lda, B, ldb));
    /* a removal that fails in its second panel: QR_E_NOTPD, and no launch after it writes R, Z or the sums */
    const double fail2[2] = {0.0, 33.0};
    qrd_stub_guard(fR, sizeof(double) * (size_t) n * n);
    CALLS(qrd_stub_script("th_panel", fail2, n > 32 ? 2 : 1), qr_lsacc_pop_dev(a, A, 2, lda, B, ldb), n > 32 ? QR_E_NOTPD : 0);
    qrd_stub_guard(fZ, sizeof(double) * (size_t) n * nrhs);
    CALLS(qrd_stub_script("th_panel", fail2 + 1, 1), qr_lsacc_slide_dev(a, A, 2, lda, B, ldb, A, 2, lda, B, ldb), QR_E_NOTPD);
    qrd_stub_guard(fZ + (size_t) n * nrhs + (size_t) QR_TPQRT_PANEL * n + n, sizeof(double) * (size_t) nrhs);      /* the sums of squares */
    CALLS(qrd_stub_script("th_panel", fail2 + 1, 1), qr_lsacc_pop_dev(a, A, 1, lda, B, ldb), QR_E_NOTPD);
    qrd_stub_guard(NULL, 0);
    qrd_stub_script("th_panel", NULL, 0);
    CALL(qr_lsacc_rows(a, &rows));
    ARG(qr_lsacc_pop_dev(a, A, (int) rows + 1, (int) rows + 1, B, (int) rows + 1));
    ARG(qr_lsacc_slide_dev(a, A, 0, lda, B, ldb, A, 1, lda, B, ldb));
    CALL(qr_lsacc_reset(a));
    CALLX(qr_lsacc_slide_dev(a, A, 1, lda, B, ldb, A, 1, lda, B, ldb) == QR_E_ARG ? 0 : 1, 0);      /* nothing to remove from an empty accumulator */
    CALL(qr_lsacc_push_dev(a, A, n, lda, B, ldb));
    CALLX(qr_lsacc_slide_dev(a, A, 1, lda, B, ldb, A, 2, lda, B, ldb), QR_E_NOTPD);                  /* fewer than n rows would remain */
    CALL(qr_lsacc_destroy(a));
    CALL(qr_plan_destroy(p));
}
static void lsacc_small(void) { lsacc_on(528, 70, 32, 70, 3, 10, 528); }
static void lsacc_wide(void) { lsacc_on(608, 260, 32, 260, 17, 259, 600); }        /* n > 256: two row blocks of the chunk's triangle, a short chunk of two blocks */
static void lsacc_subplan(void) { lsacc_on(528, 70, 32, 33, 1, 5, 300); }
static void chunked_twin(void)
{
    const int m = 40, n = 7, lda = m + 1, ldb = m + 2;
    double *A = hostd((size_t) lda * n), *B = hostd((size_t) ldb * 17), *X = hostd((size_t) n * 17), *res = hostd(17);
    CALLX(qr_lstsq_chunked(A, m, n, lda, B, 1, ldb, 16, X, res), QR_E_SINGULAR);      /* the stub's triangle keeps its zero diagonal */
    qrd_stub_set_diag(1.0);
    CALL(qr_lstsq_chunked(A, m, n, lda, B, 1, ldb, 5, X, res));           /* chunks shorter than n */
    CALL(qr_lstsq_chunked(A, m, n, lda, B, 17, ldb, 16, X, NULL));        /* taller than n, a last chunk of 8 rows */
    CALL(qr_lstsq_chunked(A, m, n, lda, B, 4, ldb, 1000, X, res));        /* one chunk: the whole matrix */
    CALL(qr_lstsq_chunked(A, m, n, lda, B, 5, ldb, n, X, res));
    qrd_stub_set_diag(0.0);
    CALLX(qr_lstsq_chunked(A, n - 1, n, lda, B, 1, ldb, 4, X, res), QR_E_SINGULAR);
    ARG(qr_lstsq_chunked(A, m, n, m - 1, B, 1, ldb, 4, X, res));
    ARG(qr_lstsq_chunked(A, m, n, lda, B, 1, ldb, 0, X, res));
}
static void downdate_primitives(void)
{
    qr_plan* p = NULL;
    const int n = 70, P = qr_tpqrt_max_rows();
    CALL(qr_plan_create(&p, 528, n, 32, 0));
    const int ldr = n + 1, ldt = QR_TPQRT_PANEL + 1;
    double *R = dev_block(n, n, ldr), *T = dev_block(QR_TPQRT_PANEL, n, ldt);
    const int adds[] = {P, 0, 3, 1, 100}, dels[] = {0, P, 2, 0, 156};
    int info = -1;
    for (int i = 0; i < 5; ++i) {
        const int pa = adds[i], pd = dels[i], rows = pa + pd, ldb = rows + 1;
        double* B = dev_block(rows, n, ldb);
        CALL(qr_tphqrt_dev(p, R, n, ldr, B, pa, pd, ldb, T, ldt, &info));
        CALL(qr_tphqrt_dev(p, R, n, ldr, B, pa, pd, ldb, T, ldt, NULL));
        for (int k = 0; k < 5; ++k) {
            const int nrhs = g_nrhs_classes[k], ldc1 = n + 2, ldc2 = rows + 2;
            double *C1 = dev_block(n, nrhs, ldc1), *C2 = dev_block(rows, nrhs, ldc2);
            CALL(qr_tphmqrt_dev(p, B, pa, pd, n, ldb, T, ldt, C1, ldc1, C2, ldc2, nrhs));
            ARG(qr_tphmqrt_dev(p, B, pa, pd, n, ldb, T, ldt, C1, ldc1, C2, rows - 1, nrhs));
        }
        if (pd) {
            const double fail = 40.0;
            CALLS(qrd_stub_script("th_panel", &fail, 1), qr_tphqrt_dev(p, R, n, ldr, B, pa, pd, ldb, T, ldt, &info), QR_E_NOTPD);
            if (info != 40) { fprintf(stderr, "info %d\n", info); exit(1); }
            qrd_stub_script("th_panel", NULL, 0);
        }
        ARG(qr_tphqrt_dev(p, R, n, ldr, B, pa, pd, rows - 1, T, ldt, &info));
    }
    ARG(qr_tphqrt_dev(p, R, n, ldr, R, 0, 0, 1, T, ldt, &info));
    ARG(qr_tphqrt_dev(p, R, n, ldr, R, P, 1, P + 1, T, ldt, &info));
    ARG(qr_tphqrt_dev(p, R, n, ldr, R, -1, 2, 1, T, ldt, &info));
    CALL(qr_plan_sync(p));
    CALL(qr_plan_destroy(p));
}
static void rolling_twin(void)
{
    const int m = 30, n = 3, lda = m + 1, ldb = m + 2, window = 10, step = 4, nwin = m;      /* (room for a window a row) */
    double *A = hostd((size_t) lda * n), *B = hostd((size_t) ldb * 17), *X = hostd((size_t) n * 17 * nwin), *res = hostd((size_t) 17 * nwin);
    CALLX(qr_lstsq_rolling(A, m, n, lda, B, 1, ldb, window, step, X, res), QR_E_SINGULAR);
    qrd_stub_set_diag(1.0);
    CALL(qr_lstsq_rolling(A, m, n, lda, B, 1, ldb, window, step, X, res));
    CALL(qr_lstsq_rolling(A, m, n, lda, B, 17, ldb, window, step, X, NULL));
    CALL(qr_lstsq_rolling(A, m, n, lda, B, 5, ldb, n, 1, X, res));                /* the smallest window, one row a step */
    CALL(qr_lstsq_rolling(A, m, n, lda, B, 4, ldb, window, window, X, res));      /* a whole window a step */
    CALL(qr_lstsq_rolling(A, m, n, lda, B, 16, ldb, m, 1, X, res));               /* one window */
    { const double fail[2] = {0.0, 2.0}; CALLS(qrd_stub_script("th_panel", fail, 2), qr_lstsq_rolling(A, m, n, lda, B, 1, ldb, window, step, X, res), QR_E_NOTPD); }
    qrd_stub_script("th_panel", NULL, 0);
    qrd_stub_set_diag(0.0);
    ARG(qr_lstsq_rolling(A, m, n, lda, B, 1, ldb, n - 1, 1, X, res));
    ARG(qr_lstsq_rolling(A, m, n, lda, B, 1, ldb, window, window + 1, X, res));
    ARG(qr_lstsq_rolling(A, m, n, lda, B, 1, ldb, m + 1, 1, X, res));
}

/* ================================================= qr_svd.c ================================================= */
static void svd_on(int pm, int pn, int r, int n)
{
    qr_plan* p = NULL;
    CALL(qr_plan_create(&p, pm, pn, 32, 0));
    const int ldg = r + 1, ldv = n + 1, ldu = r + 3;
    double *G = dev_block(r, n, ldg), *S = dev_vec(n), *V = dev_block(n, n, ldv), *U = dev_block(r, n, ldu), *tau = dev_vec(n);
    int sweeps = 0;
    CALL(qr_gesvj_dev(p, 'V', G, r, n, ldg, S, V, ldv, &sweeps));
    if (sweeps != 1) { fprintf(stderr, "sweeps %d\n", sweeps); exit(1); }
    { const double w[4] = {1.0, 0.5, 1e-3, 0.0}; CALLS(qrd_stub_script("jsvd_fold", w, 4), qr_gesvj_dev(p, 'N', G, r, n, ldg, S, NULL, 0, &sweeps), 0); }
    if (sweeps != 4) { fprintf(stderr, "sweeps %d\n", sweeps); exit(1); }
    CALLS(fill_script("jsvd_fold", 1.0, QR_JSVD_MAX_SWEEPS), qr_gesvj_dev(p, 'v', G, r, n, ldg, S, V, ldv, &sweeps), QR_E_NOCONV);
    if (sweeps != QR_JSVD_MAX_SWEEPS) { fprintf(stderr, "sweeps %d\n", sweeps); exit(1); }
    fill_script("jsvd_fold", 0.0, 0);
    /* norms in ascending order: the sort moves every column, G and V are permuted */
    { double w[128]; for (int i = 0; i < n && i < 128; ++i) w[i] = 1.0 + i; CALLS(qrd_stub_script("jsvd_colnorms", w, n < 128 ? n : 128), qr_gesvj_dev(p, 'V', G, r, n, ldg, S, V, ldv, NULL), 0); }
    const char jobs[4][2] = {{'U', 'V'}, {'N', 'V'}, {'U', 'N'}, {'N', 'N'}};
    for (int j = 0; j < 4; ++j) {
        double w[128]; for (int i = 0; i < n && i < 128; ++i) w[i] = (double) ((i * 7) % 11);
        CALLS(qrd_stub_script("jsvd_colnorms", w, j < 2 ? (n < 128 ? n : 128) : 0),
              qr_gesvd_dev(p, jobs[j][0], jobs[j][1], G, r, n, ldg, tau, S, jobs[j][0] == 'U' ? U : NULL, ldu, jobs[j][1] == 'V' ? V : NULL, ldv, &sweeps), 0);
    }
    qrd_stub_script("jsvd_colnorms", NULL, 0);
    double cond = 0.0;
    CALL(qr_cond_dev(p, G, r, n, ldg, tau, &cond));
    if (!isinf(cond)) { fprintf(stderr, "cond %g of a zero diagonal\n", cond); exit(1); }
    poke_diag(G, ldg, n, 2.0);
    { double w[128]; for (int i = 0; i < n && i < 128; ++i) w[i] = 4.0 - i * 0.01; CALLS(qrd_stub_script("jsvd_colnorms", w, n < 128 ? n : 128), qr_cond_dev(p, G, r, n, ldg, tau, &cond), 0); }
    if (!(cond > 1.0 && cond < 100.0)) { fprintf(stderr, "cond %g\n", cond); exit(1); }
    qrd_stub_script("jsvd_colnorms", NULL, 0);
    for (int k = 0; k < 5; ++k) {
        const int nrhs = g_nrhs_classes[k], ldb = r + 2;
        double* B = dev_block(r, nrhs, ldb);
        int rank = -1;
        CALL(qr_gelss_dev(p, G, r, n, ldg, tau, B, nrhs, ldb, -1.0, S, &rank));
        CALL(qr_gelss_dev(p, G, r, n, ldg, tau, B, nrhs, ldb, 0.1, S, NULL));
        ARG(qr_gelss_dev(p, G, r, n, ldg, tau, B, nrhs, r - 1, 0.1, S, NULL));
    }
    ARG(qr_gesvj_dev(p, 'V', G, r, n, ldg, S, NULL, ldv, &sweeps));
    ARG(qr_gesvj_dev(p, 'Q', G, r, n, ldg, S, V, ldv, &sweeps));
    ARG(qr_gesvd_dev(p, 'U', 'V', G, r, n, ldg, tau, S, U, r - 1, V, ldv, &sweeps));
    ARG(qr_cond_dev(p, G, r, n, ldg, tau, NULL));
    CALL(qr_plan_sync(p));
    CALL(qr_plan_destroy(p));
}
static void svd_three_blocks(void) { svd_on(200, 70, 200, 70); }      /* an odd number of column blocks */
static void svd_two_blocks(void) { svd_on(100, 64, 100, 64); }        /* an even number: one block stays in the middle */
static void svd_one_block(void) { svd_on(200, 70, 60, 20); }          /* the self-pair, on a plan made for more */
static void svd_twin(void)
{
    const int m = 40, n = 7;
    double *A = host_mats(m, n, 1, 1.0), *S = hostd(n), *U = hostd((size_t) m * n), *V = hostd((size_t) n * n), *B = hostd((size_t) m * 17),
           *X = hostd((size_t) n * 17), *res = hostd(17);
    int rank = 0;
    CALL(qr_svd(A, m, n, S, U, V));
    CALL(qr_svd(A, m, n, S, NULL, V));
    CALL(qr_svd(A, m, n, S, U, NULL));
    CALL(qr_svd(A, m, n, S, NULL, NULL));
    CALL(qr_lstsq_svd(A, m, n, B, 1, -1.0, X, res, &rank, S));
    CALL(qr_lstsq_svd(A, m, n, B, 17, 0.1, X, NULL, NULL, NULL));
    CALL(qr_lstsq_svd(host_mats(n, n, 1, 1.0), n, n, B, 5, -1.0, X, res, NULL, S));
    CALLS(fill_script("jsvd_fold", 1.0, QR_JSVD_MAX_SWEEPS), qr_svd(A, m, n, S, U, V), QR_E_NOCONV);
    CALLS(fill_script("jsvd_fold", 1.0, QR_JSVD_MAX_SWEEPS), qr_lstsq_svd(A, m, n, B, 4, -1.0, X, res, &rank, S), QR_E_NOCONV);
    fill_script("jsvd_fold", 0.0, 0);
    ARG(qr_svd(A, n - 1, n, S, U, V));
    ARG(qr_lstsq_svd(A, m, n, B, 0, -1.0, X, res, &rank, S));
}

/* ================================================= the batched units ================================================= */
/* one shape of a batched configuration: m x n members, nrhs right-hand sides, `batch` of them, leading dimensions with `pad` extra rows and
 * member strides with `gap` extra doubles */
typedef struct { int m, n, nrhs, batch, pad, gap; } bshape;
#define LD(rows) ((rows) + s->pad)
#define ST(ld, cols) ((long long) (ld) * (cols) + s->gap)
#define DB(rows, cols) dev_blocks(rows, cols, LD(rows), s->batch, ST(LD(rows), cols))
#define DV(len) dev_blocks(len, 1, len, s->batch, (len) + s->gap)
#define DI(len) ((int*) dev_bytes(sizeof(int) * (size_t) ((s->batch - 1) * ((len) + s->gap) + (len))))
#define PK(len) dev_vec((long) (len) * s->batch)          /* packed: len per member */
#define PI(len) dev_ints((long) (len) * s->batch)

static void batched_core(const bshape* s)
{
    qr_plan* p = NULL;
    CALL(qr_plan_create(&p, 64, 8, 0, 0));          /* the plan supplies the stream: its shape bounds nothing */
    const int m = s->m, n = s->n, nrhs = s->nrhs, b = s->batch, lda = LD(m), ldn = LD(n);
    const long long sA = ST(lda, n), sB = ST(lda, nrhs), st = n + s->gap, sV = ST(ldn, n);
    double *A = DB(m, n), *tau = DV(n), *B = DB(m, nrhs), *Q = DB(m, n), *S = DV(n), *V = DB(n, n), *res = PK(nrhs);
    int *info = PI(1), *jp = DI(n), *rank = PI(1), *sweeps = PI(1);
    CALL(qr_geqrf_batched_dev(p, A, m, n, lda, sA, tau, st, b));
    CALL(qr_ormqr_batched_dev(p, 'T', A, m, n, lda, sA, tau, st, B, nrhs, lda, sB, b));
    CALL(qr_ormqr_batched_dev(p, 'N', A, m, n, lda, sA, tau, st, B, nrhs, lda, sB, b));
    CALL(qr_orgqr_batched_dev(p, A, m, n, lda, sA, tau, st, Q, lda, sA, b));
    CALL(qr_gels_batched_dev(p, A, m, n, lda, sA, tau, st, B, nrhs, lda, sB, info, b));
    CALL(qr_geqp3_batched_dev(p, A, m, n, lda, sA, jp, st, tau, st, b));
    CALL(qr_rank_batched_dev(p, A, m, n, lda, sA, -1.0, rank, b));
    CALL(qr_gelsp_batched_dev(p, A, m, n, lda, sA, jp, st, tau, st, B, nrhs, lda, sB, -1.0, res, rank, b));
    CALL(qr_gelsp_batched_dev(p, A, m, n, lda, sA, jp, st, tau, st, B, nrhs, lda, sB, 0.1, NULL, NULL, b));
    CALL(qr_gelsy_batched_dev(p, A, m, n, lda, sA, jp, st, tau, st, B, nrhs, lda, sB, -1.0, res, NULL, b));
    CALL(qr_gesvd_batched_dev(p, 'U', 'V', A, m, n, lda, sA, jp, st, tau, st, S, st, Q, lda, sA, V, ldn, sV, rank, sweeps, info, b));
    CALL(qr_gesvd_batched_dev(p, 'N', 'V', A, m, n, lda, sA, jp, st, tau, st, S, st, NULL, 0, 0, V, ldn, sV, NULL, NULL, info, b));
    CALL(qr_gesvd_batched_dev(p, 'U', 'N', A, m, n, lda, sA, jp, st, tau, st, S, st, Q, lda, sA, NULL, 0, 0, rank, NULL, info, b));
    CALL(qr_gesvd_batched_dev(p, 'N', 'N', A, m, n, lda, sA, jp, st, tau, st, S, st, NULL, 0, 0, NULL, 0, 0, NULL, sweeps, info, b));
    CALL(qr_geqrf_batched_dev(p, A, m, n, lda, sA, tau, st, 0));
    ARG(qr_geqrf_batched_dev(p, A, m, n, m - 1, sA, tau, st, b));
    ARG(qr_geqrf_batched_dev(p, A, m, n, lda, (long long) lda * n - 1, tau, st, b));
    ARG(qr_ormqr_batched_dev(p, 'Q', A, m, n, lda, sA, tau, st, B, nrhs, lda, sB, b));
    ARG(qr_gels_batched_dev(p, A, m, n, lda, sA, tau, st, B, nrhs, lda, sB, NULL, b));
    ARG(qr_gelsp_batched_dev(p, A, m, n, lda, sA, jp, n - 1, tau, st, B, nrhs, lda, sB, -1.0, res, rank, b));
    ARG(qr_gesvd_batched_dev(p, 'U', 'V', A, m, n, lda, sA, jp, st, tau, st, S, st, NULL, lda, sA, V, ldn, sV, rank, sweeps, info, b));
    ARG(qr_rank_batched_dev(p, A, m, n, lda, sA, NAN, rank, b));
    CALL(qr_plan_sync(p));
    CALL(qr_plan_destroy(p));
}
static void batched_wave(void) { const bshape s = {40, 7, 1, 5, 1, 3}; batched_core(&s); }
static void batched_wave_edge(void) { const bshape s = {64, 15, 17, 1, 3, 0}; batched_core(&s); }       /* n + nrhs == 32, batch 1 */
static void batched_wg33(void) { const bshape s = {64, 17, 16, 5, 1, 1}; batched_core(&s); }            /* n + nrhs == 33: a workgroup per matrix */
static void batched_wg64(void) { const bshape s = {256, 60, 4, 3, 1, 7}; batched_core(&s); }            /* n + nrhs == 64 at the row limit of the class */
static void batched_composed(void) { const bshape s = {300, 30, 5, 2, 1, 1}; batched_core(&s); }        /* n + nrhs == 35 columns of 300 rows do not fit: geqrf, ormqr, trsm */
static void batched_composed_wide_rhs(void) { const bshape s = {70, 50, 17, 5, 3, 5}; batched_core(&s); }      /* n + nrhs > 64 */
static void batched_twins(void)
{
    const int m = 40, n = 7, b = 5;
    double *A = host_mats(m, n, b, 1.0), *Q = hostd((size_t) m * n * b), *R = hostd((size_t) n * n * b), *B = hostd((size_t) m * 17 * b),
           *X = hostd((size_t) n * 17 * b), *res = hostd((size_t) 17 * b), *S = hostd((size_t) n * b), *V = hostd((size_t) n * n * b);
    int *info = hosti(b), *jp = hosti((size_t) n * b), *rank = hosti(b);
    const int nrhs_list[] = {1, 17, 60};
    CALL(qr_thin_batched(A, m, n, b, Q, R));
    CALL(qr_thin_pivoted_batched(A, m, n, b, Q, R, jp));
    for (int i = 0; i < 3; ++i) {
        const int nrhs = nrhs_list[i];
        if (nrhs > 17) { B = hostd((size_t) m * nrhs * b); X = hostd((size_t) n * nrhs * b); res = hostd((size_t) nrhs * b); }
        CALL(qr_lstsq_batched(A, m, n, B, nrhs, b, X, res, info));
        CALL(qr_lstsq_batched(A, m, n, B, nrhs, 1, X, NULL, info));
        CALL(qr_lstsq_pivoted_batched(A, m, n, B, nrhs, b, -1.0, 0, X, res, rank, jp));
        CALL(qr_lstsq_pivoted_batched(A, m, n, B, nrhs, b, 0.1, 1, X, NULL, NULL, NULL));
    }
    CALL(qr_svd_batched(A, m, n, b, S, Q, V, rank));
    CALL(qr_svd_batched(A, m, n, b, S, NULL, NULL, NULL));
    CALL(qr_svd_batched(A, m, n, 1, S, Q, NULL, rank));
    qrd_stub_set_info(2);
    CALLX(qr_lstsq_batched(A, m, n, B, 1, b, X, res, info), QR_E_SINGULAR);
    CALLX(qr_svd_batched(A, m, n, b, S, Q, V, rank), QR_E_NOCONV);
    qrd_stub_set_info(0);
    CALL(qr_thin_batched(A, m, n, 0, Q, R));
    ARG(qr_thin_batched(A, n - 1, n, b, Q, R));
    ARG(qr_thin_batched(A, 513, n, b, Q, R));
    ARG(qr_lstsq_batched(A, m, n, B, 0, b, X, res, info));
    ARG(qr_lstsq_pivoted_batched(A, m, n, B, 1, b, NAN, 0, X, res, rank, jp));
    ARG(qr_svd_batched(A, m, 65, b, S, Q, V, rank));
    ARG(qr_thin_pivoted_batched(A, m, n, b, Q, R, NULL));
}

/* ---- qr_batched_update.c: p_add rows added, p_del removed, nrhs right-hand sides riding along ---- */
static void bupdate_on(const bshape* s, int p_add, int p_del)
{
    qr_plan* pl = NULL;
    CALL(qr_plan_create(&pl, 64, 8, 0, 0));
    const int n = s->n, nrhs = s->nrhs, b = s->batch, p = p_add + p_del, ldr = LD(n), ldb = LD(p);
    const long long sR = ST(ldr, n), sB = ST(ldb, n), sC1 = ST(ldr, nrhs), sC2 = ST(ldb, nrhs), st = n + s->gap;
    double *R = DB(n, n), *Bk = DB(p, n), *tau = DV(n), *C1 = DB(n, nrhs), *C2 = DB(p, nrhs);
    int* info = PI(1);
    CALL(qr_tphqrt_batched_dev(pl, R, n, ldr, sR, Bk, p_add, p_del, ldb, sB, tau, st, C1, ldr, sC1, C2, ldb, sC2, nrhs, info, b));
    CALL(qr_tphqrt_batched_dev(pl, R, n, ldr, sR, Bk, p_add, p_del, ldb, sB, tau, st, NULL, 0, 0, NULL, 0, 0, 0, info, b));
    if (!p_del) {
        CALL(qr_tpqrt_batched_dev(pl, R, n, ldr, sR, Bk, p, ldb, sB, tau, st, C1, ldr, sC1, C2, ldb, sC2, nrhs, b));
        CALL(qr_tpmqrt_batched_dev(pl, 'N', Bk, p_add, 0, n, ldb, sB, tau, st, C1, ldr, sC1, C2, ldb, sC2, nrhs, b));
    } else {
        ARG(qr_tpmqrt_batched_dev(pl, 'N', Bk, p_add, p_del, n, ldb, sB, tau, st, C1, ldr, sC1, C2, ldb, sC2, nrhs, b));
        ARG(qr_tphqrt_batched_dev(pl, R, n, ldr, sR, Bk, p_add, p_del, ldb, sB, tau, st, C1, ldr, sC1, C2, ldb, sC2, nrhs, NULL, b));
    }
    CALL(qr_tpmqrt_batched_dev(pl, 'T', Bk, p_add, p_del, n, ldb, sB, tau, st, C1, ldr, sC1, C2, ldb, sC2, nrhs, b));
    ARG(qr_tpmqrt_batched_dev(pl, 'T', Bk, p_add, p_del, n, p - 1, sB, tau, st, C1, ldr, sC1, C2, ldb, sC2, nrhs, b));
    ARG(qr_tphqrt_batched_dev(pl, R, n, ldr, sR, Bk, p_add, p_del, ldb, (long long) ldb * n - 1, tau, st, C1, ldr, sC1, C2, ldb, sC2, nrhs, info, b));
    ARG(qr_tphqrt_batched_dev(pl, R, n, ldr, sR, Bk, qr_tpqrt_batched_max_rows(n + nrhs) + 1, 0, ldb, sB, tau, st, C1, ldr, sC1, C2, ldb, sC2, nrhs, info, b));
    /* the accumulator: push of more rows than one launch takes, pop, slide, the plain, the damped and the trust solve, the covariance */
    qr_lsacc_batched* a = NULL;
    CALL(qr_lsacc_batched_create(&a, pl, n, nrhs, b));
    const int cap = qr_tpqrt_batched_max_rows(n + nrhs), big = cap + 3, lda = LD(big), ldx = LD(n);
    const long long sA = ST(lda, n), sAB = ST(lda, nrhs), sX = ST(ldx, nrhs), sres = nrhs + s->gap;
    double *A = DB(big, n), *AB = DB(big, nrhs), *X = DB(n, nrhs), *res = DV(nrhs);
    CALL(qr_lsacc_batched_push_dev(a, A, big, lda, sA, AB, lda, sAB));
    CALL(qr_lsacc_batched_push_dev(a, A, 1, lda, sA, AB, lda, sAB));
    CALL(qr_lsacc_batched_pop_dev(a, A, cap, lda, sA, AB, lda, sAB, info));
    CALL(qr_lsacc_batched_slide_dev(a, A, cap / 2, lda, sA, AB, lda, sAB, A, cap - cap / 2, lda, sA, AB, lda, sAB, info));
    CALL(qr_lsacc_batched_solve_dev(a, X, ldx, sX, res, sres, info));
    CALL(qr_lsacc_batched_solve_dev(a, X, ldx, sX, NULL, 0, info));
    const double* fR = NULL; const int* frows = NULL; int fl = 0; long long fs = 0;
    CALL(qr_lsacc_batched_factor_dev(a, &fR, &fl, &fs, NULL, NULL, NULL, NULL, &frows));
    CALL(qr_lsacc_batched_factor_dev(a, NULL, NULL, NULL, &fR, &fl, &fs, &fR, NULL));
    {   /* qr_batched_damped.c, qr_batched_trust.c and qr_batched_stats.c on the accumulator */
        const int nlam = 3, cols = nlam * nrhs;
        double *D = DV(n), *lam = DV(nlam), *Xd = dev_blocks(n, cols, ldx, b, (long long) ldx * cols + s->gap), *xn = PK(cols), *rs = PK(cols);
        int* infod = PI(nlam);
        CALL(qr_lsacc_batched_solve_damped_dev(a, D, n + s->gap, lam, nlam, nlam + s->gap, Xd, ldx, (long long) ldx * cols + s->gap, xn, rs, infod));
        CALL(qr_lsacc_batched_solve_damped_dev(a, D, 0, lam, 1, 0, Xd, ldx, (long long) ldx * cols + s->gap, NULL, NULL, infod));
        CALL(qr_lsacc_batched_solve_damped_dev(a, NULL, 0, lam, nlam, 0, Xd, ldx, (long long) ldx * cols + s->gap, xn, NULL, infod));
        ARG(qr_lsacc_batched_solve_damped_dev(a, D, n - 1, lam, nlam, 0, Xd, ldx, (long long) ldx * cols + s->gap, xn, rs, infod));
        double *C = DB(n, n), *se = DV(n), *sig = PK(1);
        CALL(qr_lsacc_batched_covar_dev(a, QR_COV_SCALED, nrhs - 1, C, ldr, sR, se, st, sig, info));
        CALL(qr_lsacc_batched_covar_dev(a, QR_COV_UNSCALED, 0, NULL, 0, 0, se, st, NULL, info));
        CALL(qr_lsacc_batched_covar_dev(a, QR_COV_UNSCALED, 0, C, ldr, sR, NULL, 0, NULL, info));
        ARG(qr_lsacc_batched_covar_dev(a, QR_COV_SCALED, nrhs, C, ldr, sR, se, st, sig, info));
        ARG(qr_lsacc_batched_covar_dev(a, QR_COV_SCALED, 0, NULL, 0, 0, NULL, 0, sig, info));
        double *del = PK(1), *l0 = PK(1), *lo = PK(1), *Xt = dev_blocks(n, 1, ldx, b, ldx + s->gap);
        int *it = PI(1), *stt = PI(1);
        if (nrhs == 1) {
            CALL(qr_lsacc_batched_solve_trust_dev(a, D, n + s->gap, del, 1, l0, 1, 0.1, 10, Xt, ldx, ldx + s->gap, lo, xn, rs, it, stt, info));
            CALL(qr_lsacc_batched_solve_trust_dev(a, NULL, 0, del, 0, NULL, 0, 0.1, 1, Xt, ldx, ldx + s->gap, lo, NULL, NULL, NULL, NULL, info));
            ARG(qr_lsacc_batched_solve_trust_dev(a, D, n + s->gap, del, 1, l0, 1, 1.5, 10, Xt, ldx, ldx + s->gap, lo, xn, rs, it, stt, info));
        } else
            ARG(qr_lsacc_batched_solve_trust_dev(a, D, n + s->gap, del, 1, l0, 1, 0.1, 10, Xt, ldx, ldx + s->gap, lo, xn, rs, it, stt, info));
    }
    ARG(qr_lsacc_batched_pop_dev(a, A, cap + 1, lda, sA, AB, lda, sAB, info));
    ARG(qr_lsacc_batched_pop_dev(a, A, 1, lda, sA, AB, lda, sAB, NULL));
    ARG(qr_lsacc_batched_slide_dev(a, A, cap, lda, sA, AB, lda, sAB, A, 1, lda, sA, AB, lda, sAB, info));
    ARG(qr_lsacc_batched_push_dev(a, A, 0, lda, sA, AB, lda, sAB));
    ARG(qr_lsacc_batched_solve_dev(a, X, n - 1, sX, res, sres, info));
    CALL(qr_lsacc_batched_reset(a));
    CALL(qr_lsacc_batched_destroy(a));
    ARG(qr_lsacc_batched_create(&a, pl, n, QR_BATCHED_MAX_N - n + 1, b));
    CALL(qr_lsacc_batched_create(&a, pl, n, nrhs, 0));          /* an empty batch: nothing is allocated, nothing launched */
    CALL(qr_lsacc_batched_push_dev(a, A, 1, lda, sA, AB, lda, sAB));
    CALL(qr_lsacc_batched_destroy(a));
    CALL(qr_plan_sync(pl));
    CALL(qr_plan_destroy(pl));
}
static void bupdate_wave(void) { const bshape s = {0, 7, 1, 5, 1, 3}; bupdate_on(&s, 3, 2); }
static void bupdate_wave_edge(void) { const bshape s = {0, 28, 4, 1, 3, 0}; bupdate_on(&s, 64, 0); }        /* n + nrhs == 32, p == 64 */
static void bupdate_wg_rows(void) { const bshape s = {0, 7, 1, 5, 1, 1}; bupdate_on(&s, 0, 65); }           /* p == 65: a workgroup per member; nothing added */
static void bupdate_wg33(void) { const bshape s = {0, 17, 16, 3, 1, 5}; bupdate_on(&s, 5, 0); }             /* n + nrhs == 33 */
static void bupdate_limit(void) { const bshape s = {0, 30, 2, 2, 1, 1}; bupdate_on(&s, 200, 56); }          /* the row limit of the class, 256 */
static void bupdate_wide_limit(void) { const bshape s = {0, 47, 17, 2, 3, 1}; bupdate_on(&s, 226, 0); }     /* n + nrhs == 64 at its limit, 226 */
static void brolling_twin(void)
{
    const int m = 30, n = 3, b = 5, window = 10, step = 4, nwin = (m - window) / step + 1;
    double *A = hostd((size_t) m * n * b), *B = hostd((size_t) m * 17 * b), *X = hostd((size_t) n * 17 * nwin * b), *res = hostd((size_t) 17 * nwin * b);
    int* info = hosti((size_t) nwin * b);
    CALL(qr_lstsq_rolling_batched(A, m, n, B, 1, b, window, step, X, res, info));
    CALL(qr_lstsq_rolling_batched(A, m, n, B, 17, 1, window, step, X, NULL, info));
    CALL(qr_lstsq_rolling_batched(A, m, n, B, 4, b, m, 1, X, res, info));
    CALL(qr_lstsq_rolling_batched(A, m, n, B, 4, 0, window, step, X, res, info));
    qrd_stub_set_info(-1);
    CALLX(qr_lstsq_rolling_batched(A, m, n, B, 5, b, window, step, X, res, info), QR_E_NOTPD);
    qrd_stub_set_info(0);
    ARG(qr_lstsq_rolling_batched(A, m, n, B, 1, b, n - 1, 1, X, res, info));
    ARG(qr_lstsq_rolling_batched(A, m, n, B, 62, b, window, step, X, res, info));
    ARG(qr_lstsq_rolling_batched(A, 600, n, B, 1, b, 300, 129, X, res, info));
}

/* ---- qr_batched_minnorm.c, _damped.c, _trust.c: the tall matrix F (m x n) is what is factored ---- */
static void bminnorm_on(const bshape* s)
{
    qr_plan* p = NULL;
    CALL(qr_plan_create(&p, 64, 8, 0, 0));
    const int m = s->m, n = s->n, nrhs = s->nrhs, b = s->batch, lda = LD(m), ldw = LD(n);
    const long long sA = ST(lda, n), sB = ST(lda, nrhs), st = n + s->gap, sW = ST(ldw, m);
    double *A = DB(m, n), *tau = DV(n), *B = DB(m, nrhs), *W = DB(n, m);
    int* info = PI(1);
    CALL(qr_geqrf_batched_dev(p, A, m, n, lda, sA, tau, st, b));
    CALL(qr_minnorm_batched_dev(p, A, m, n, lda, sA, tau, st, B, nrhs, lda, sB, info, b));
    CALL(qr_gels_t_batched_dev(p, A, m, n, lda, sA, tau, st, B, nrhs, lda, sB, info, b));
    CALL(qr_transpose_batched_dev(p, W, n, m, ldw, sW, A, lda, sA, b));
    CALL(qr_gels_wide_batched_dev(p, W, n, m, ldw, sW, A, lda, sA, tau, st, B, nrhs, lda, sB, info, b));
    CALL(qr_gels_wide_batched_dev(p, W, n, m, ldw, sW, A, lda, sA, tau, st, B, nrhs, lda, sB, info, 0));
    ARG(qr_minnorm_batched_dev(p, A, m, n, lda, sA, tau, st, B, nrhs, m - 1, sB, info, b));
    ARG(qr_gels_t_batched_dev(p, A, m, n, lda, sA, tau, st, B, nrhs, lda, sB, NULL, b));
    ARG(qr_transpose_batched_dev(p, W, n, 513, ldw, sW, A, lda, sA, b));
    ARG(qr_gels_wide_batched_dev(p, W, n, m, n - 1, sW, A, lda, sA, tau, st, B, nrhs, lda, sB, info, b));
    /* damped and trust-region solves on the same shapes: from factors, factoring, and the wide form (m < n there: W is the n x m input) */
    const int nlam = 3, cols = nlam * nrhs, ldx = LD(n), ldxw = LD(m);
    const long long sX = (long long) ldx * cols + s->gap, sXw = (long long) ldxw * cols + s->gap, sD = n + s->gap, sl = nlam + s->gap;
    double *D = DV(n), *lam = DV(nlam), *X = dev_blocks(n, cols, ldx, b, sX), *Xw = dev_blocks(m, cols, ldxw, b, sXw), *xn = PK(cols), *rs = PK(cols),
           *rss = PK(nrhs), *Bw = DB(n, nrhs);
    int *infod = PI(nlam), *jp = DI(n);
    if (n + nrhs <= QR_BATCHED_MAX_N) {
        CALL(qr_damped_batched_dev(p, A, n, lda, sA, B, nrhs, lda, sB, rss, jp, st, D, sD, lam, nlam, sl, 0, X, ldx, sX, xn, rs, infod, b));
        CALL(qr_damped_batched_dev(p, A, n, lda, sA, B, nrhs, lda, sB, NULL, NULL, 0, NULL, 0, lam, 1, 0, 1, X, ldx, sX, NULL, NULL, infod, b));
        CALL(qr_damped_batched_dev(p, A, n, lda, sA, B, nrhs, lda, sB, rss, NULL, 0, D, 0, lam, nlam, 0, 0, X, ldx, sX, xn, NULL, infod, b));
        CALL(qr_gels_damped_batched_dev(p, A, m, n, lda, sA, tau, st, B, nrhs, lda, sB, D, sD, lam, nlam, sl, X, ldx, sX, xn, rs, infod, b));
        CALL(qr_gels_damped_batched_dev(p, A, m, n, lda, sA, tau, st, B, nrhs, lda, sB, NULL, 0, lam, 1, 0, X, ldx, sX, NULL, NULL, infod, b));
        ARG(qr_damped_batched_dev(p, A, n, lda, sA, B, nrhs, lda, sB, rss, jp, st, D, sD, lam, nlam, sl, 1, X, ldx, sX, xn, rs, infod, b));
        ARG(qr_damped_batched_dev(p, A, n, lda, sA, B, nrhs, lda, sB, rss, jp, st, D, sD, lam, nlam, nlam - 1, 0, X, ldx, sX, xn, rs, infod, b));
        ARG(qr_gels_damped_batched_dev(p, A, m, n, lda, sA, tau, st, B, nrhs, lda, sB, D, sD, lam, 0, sl, X, ldx, sX, xn, rs, infod, b));
        if (n < m && n + nrhs <= QR_BATCHED_MAX_N) {
            CALL(qr_gels_damped_wide_batched_dev(p, W, n, m, ldw, sW, A, lda, sA, tau, st, Bw, nrhs, ldw, ST(ldw, nrhs), lam, nlam, sl, Xw, ldxw, sXw, xn, rs, infod, b));
            CALL(qr_gels_damped_wide_batched_dev(p, W, n, m, ldw, sW, A, lda, sA, tau, st, Bw, nrhs, ldw, ST(ldw, nrhs), lam, 1, 0, Xw, ldxw, sXw, NULL, NULL, infod, b));
            ARG(qr_gels_damped_wide_batched_dev(p, W, n, m, ldw, sW, A, lda, sA, tau, st, Bw, nrhs, ldw, ST(ldw, nrhs), lam, nlam, sl, Xw, m - 1, sXw, xn, rs, infod, b));
        }
    }
    if (n <= QR_BATCHED_MAX_N - 1) {
        double *del = DV(1), *l0 = DV(1), *lo = PK(1), *x1 = dev_blocks(n, 1, ldx, b, ldx + s->gap), *xw1 = dev_blocks(m, 1, ldxw, b, ldxw + s->gap), *b1 = DB(m, 1),
               *bw1 = DB(n, 1);
        int *it = PI(1), *stt = PI(1);
        const long long s1 = 1 + s->gap, sb1 = ST(lda, 1), sx1 = ldx + s->gap;
        CALL(qr_trust_batched_dev(p, A, n, lda, sA, b1, lda, sb1, rss, jp, st, D, sD, del, s1, l0, s1, 0.1, 10, 0, x1, ldx, sx1, lo, xn, rs, it, stt, info, b));
        CALL(qr_trust_batched_dev(p, A, n, lda, sA, b1, lda, sb1, NULL, NULL, 0, NULL, 0, del, 0, NULL, 0, 0.1, 1, 1, x1, ldx, sx1, lo, NULL, NULL, NULL, NULL, info, b));
        CALL(qr_gels_trust_batched_dev(p, A, m, n, lda, sA, tau, st, b1, lda, sb1, D, sD, del, s1, l0, s1, 0.1, 10, x1, ldx, sx1, lo, xn, rs, it, stt, info, b));
        CALL(qr_gels_trust_batched_dev(p, A, m, n, lda, sA, tau, st, b1, lda, sb1, NULL, 0, del, 0, NULL, 0, 0.1, 10, x1, ldx, sx1, lo, NULL, NULL, NULL, NULL, info, b));
        ARG(qr_trust_batched_dev(p, A, n, lda, sA, b1, lda, sb1, rss, jp, st, D, sD, del, s1, l0, s1, 1.0, 10, 0, x1, ldx, sx1, lo, xn, rs, it, stt, info, b));
        ARG(qr_gels_trust_batched_dev(p, A, m, n, lda, sA, tau, st, b1, lda, sb1, D, sD, del, s1, l0, s1, 0.1, 0, x1, ldx, sx1, lo, xn, rs, it, stt, info, b));
        if (n < m) {
            CALL(qr_gels_trust_wide_batched_dev(p, W, n, m, ldw, sW, A, lda, sA, tau, st, bw1, ldw, ST(ldw, 1), del, s1, l0, s1, 0.1, 10, xw1, ldxw, ldxw + s->gap, lo, xn, rs, it, stt, info, b));
            CALL(qr_gels_trust_wide_batched_dev(p, W, n, m, ldw, sW, A, lda, sA, tau, st, bw1, ldw, ST(ldw, 1), del, 0, NULL, 0, 0.1, 10, xw1, ldxw, ldxw + s->gap, lo, NULL, NULL, NULL, NULL, info, b));
            ARG(qr_gels_trust_wide_batched_dev(p, W, n, m, ldw, sW, A, lda, sA, tau, st, bw1, ldw, ST(ldw, 1), del, s1, l0, s1, 0.1, 10, xw1, m - 1, ldxw + s->gap, lo, xn, rs, it, stt, info, b));
        }
    }
    CALL(qr_plan_sync(p));
    CALL(qr_plan_destroy(p));
}
static void bminnorm_wave(void) { const bshape s = {40, 7, 1, 5, 1, 3}; bminnorm_on(&s); }
static void bminnorm_wave_edge(void) { const bshape s = {64, 15, 17, 1, 3, 0}; bminnorm_on(&s); }
static void bminnorm_wg33(void) { const bshape s = {64, 17, 16, 5, 1, 1}; bminnorm_on(&s); }
static void bminnorm_wg_rows(void) { const bshape s = {65, 7, 4, 3, 1, 5}; bminnorm_on(&s); }                /* m == 65: no fused damped / trust launch */
static void bminnorm_narrow_fit(void) { const bshape s = {300, 30, 5, 2, 1, 1}; bminnorm_on(&s); }          /* past the class limit of 35 columns, but 300 rows fit: fused */
static void bminnorm_composed(void) { const bshape s = {500, 33, 5, 2, 1, 1}; bminnorm_on(&s); }            /* 38 columns of 500 rows do not fit */
static void bminnorm_wide_rhs(void) { const bshape s = {70, 50, 17, 5, 3, 5}; bminnorm_on(&s); }            /* n + nrhs > 64: no damped call takes it */
static void bdamped_twins(void)
{
    const int b = 5, nlam = 3;
    const int shapes[4][3] = {{40, 7, 1}, {65, 7, 17}, {7, 40, 4}, {64, 15, 17}};      /* tall fused, tall composed, wide, the wave edge */
    for (int i = 0; i < 4; ++i) {
        const int m = shapes[i][0], n = shapes[i][1], nrhs = shapes[i][2], wide = m < n;
        double *A = hostd((size_t) m * n * b), *B = hostd((size_t) m * nrhs * b), *D = hostd((size_t) n * b), *lam = hostd((size_t) nlam * b),
               *X = hostd((size_t) n * nlam * nrhs * b), *xn = hostd((size_t) nlam * nrhs * b), *rs = hostd((size_t) nlam * nrhs * b);
        int* info = hosti((size_t) nlam * b);
        CALL(qr_lstsq_damped_batched(A, m, n, B, nrhs, b, wide ? NULL : D, lam, nlam, X, xn, rs, info));
        CALL(qr_lstsq_damped_batched(A, m, n, B, nrhs, 1, NULL, lam, 1, X, NULL, NULL, info));
        if (wide) ARG(qr_lstsq_damped_batched(A, m, n, B, nrhs, b, D, lam, nlam, X, xn, rs, info));
        if (nrhs == 1) {
            double *del = hostd(b), *l0 = hostd(b), *lo = hostd(b);
            int *it = hosti(b), *st = hosti(b);
            for (int q = 0; q < b; ++q) del[q] = 1.0;
            CALL(qr_lstsq_trust_batched(A, m, n, B, b, D, del, l0, 0.1, 10, X, lo, xn, rs, it, st, info));
            CALL(qr_lstsq_trust_batched(A, m, n, B, 1, NULL, del, NULL, 0.1, 10, X, lo, NULL, NULL, NULL, NULL, info));
            qrd_stub_set_info(1);
            CALLX(qr_lstsq_trust_batched(A, m, n, B, b, D, del, l0, 0.1, 10, X, lo, xn, rs, it, st, info), QR_E_SINGULAR);
            qrd_stub_set_info(0);
            ARG(qr_lstsq_trust_batched(A, m, n, B, b, D, del, l0, 1.0, 10, X, lo, xn, rs, it, st, info));
        }
        if (wide) {
            double *del = hostd(b), *lo = hostd(b);
            CALL(qr_lstsq_trust_batched(A, m, n, B, b, NULL, del, NULL, 0.1, 10, X, lo, xn, rs, NULL, NULL, info));
            CALL(qr_lstsq_trust_batched(hostd((size_t) 65 * 7 * b), 65, 7, hostd((size_t) 65 * b), b, NULL, del, NULL, 0.1, 10, X, lo, xn, rs, NULL, NULL, info));      /* tall, composed */
            ARG(qr_lstsq_trust_batched(A, m, n, B, b, del, del, NULL, 0.1, 10, X, lo, xn, rs, NULL, NULL, info));
        }
        qrd_stub_set_info(3);
        CALLX(qr_lstsq_damped_batched(A, m, n, B, nrhs, b, NULL, lam, nlam, X, xn, rs, info), QR_E_SINGULAR);
        qrd_stub_set_info(0);
        ARG(qr_lstsq_damped_batched(A, m, n, B, nrhs, b, NULL, lam, 0, X, xn, rs, info));
        ARG(qr_lstsq_damped_batched(A, m, n, B, 64, b, NULL, lam, nlam, X, xn, rs, info));
    }
    double* A = hostd(8);
    int info = 0;
    CALL(qr_lstsq_damped_batched(A, 2, 1, A, 1, 0, NULL, A, 1, A, NULL, NULL, &info));
}

/* ---- qr_batched_lse.c, _bvls.c, _irls.c, _stats.c, _lsei.c: one launch each; device call with optional outputs present and absent, the twin ---- */
static void bconstrained_on(const bshape* s, int pc, int mg, int neq)
{
    qr_plan* p = NULL;
    CALL(qr_plan_create(&p, 64, 8, 0, 0));
    const int m = s->m, n = s->n, nrhs = s->nrhs, b = s->batch, lda = LD(m), ldc = LD(pc), ldx = LD(n), ldg = LD(mg);
    const long long sA = ST(lda, n), sC = ST(ldc, n), sB = ST(lda, nrhs), sD = ST(ldc, nrhs), sX = ST(ldx, nrhs), sn = n + s->gap, sm = m + s->gap, sg = mg + s->gap;
    double *A = DB(m, n), *C = DB(pc, n), *B = DB(m, nrhs), *D = DB(pc, nrhs), *X = DB(n, nrhs), *L = DB(pc, nrhs), *res = DV(nrhs);
    int* info = PI(1);
    /* gglse */
    CALL(qr_gglse_batched_dev(p, A, m, n, lda, sA, C, pc, ldc, sC, B, lda, sB, D, ldc, sD, nrhs, X, ldx, sX, L, ldc, sD, res, nrhs + s->gap, info, b));
    CALL(qr_gglse_batched_dev(p, A, m, n, lda, sA, C, pc, ldc, sC, B, lda, sB, D, ldc, sD, nrhs, X, ldx, sX, NULL, 0, 0, NULL, 0, info, b));
    CALL(qr_gglse_batched_dev(p, A, m, n, lda, sA, C, pc, ldc, sC, B, lda, sB, D, ldc, sD, nrhs, X, ldx, sX, L, ldc, sD, res, nrhs + s->gap, info, 0));
    ARG(qr_gglse_batched_dev(p, A, m, n, lda, sA, C, pc, pc - 1, sC, B, lda, sB, D, ldc, sD, nrhs, X, ldx, sX, L, ldc, sD, res, nrhs + s->gap, info, b));
    ARG(qr_gglse_batched_dev(p, A, m, n, lda, sA, C, n + 1, n + 1, sC, B, lda, sB, D, ldc, sD, nrhs, X, ldx, sX, L, ldc, sD, res, nrhs + s->gap, info, b));
    ARG(qr_gglse_batched_dev(p, A, qr_gglse_batched_max_rows(n, pc, nrhs) + 1, n, 600, 600LL * n, C, pc, ldc, sC, B, 600, 600LL * nrhs, D, ldc, sD, nrhs, X, ldx, sX, L, ldc, sD, res, nrhs + s->gap, info, b));
    if (n <= QR_BATCHED_MAX_N - 1 && m >= n) {
        double *b1 = DV(m), *lo = DV(n), *hi = DV(n), *x1 = DV(n), *w1 = DV(n), *r1 = PK(1), *wm = DV(m), *prior = DV(m), *sc = PK(1), *E = DV(m), *H = DV(m),
               *Cv = DB(n, n), *se = DV(n), *x0 = DV(n);
        int *state = DI(n), *it = PI(1), *stt = PI(1), *dof = PI(1);
        /* bvls */
        CALL(qr_bvls_batched_dev(p, A, m, n, lda, sA, b1, sm, lo, hi, sn, 0, x1, sn, w1, sn, state, sn, r1, it, info, b));
        CALL(qr_bvls_batched_dev(p, A, m, n, lda, sA, b1, sm, lo, NULL, 0, 5, x1, sn, NULL, 0, NULL, 0, NULL, NULL, info, b));
        CALL(qr_bvls_batched_dev(p, A, m, n, lda, sA, b1, sm, NULL, hi, 0, INT_MAX, x1, sn, w1, sn, NULL, 0, r1, NULL, info, b));
        ARG(qr_bvls_batched_dev(p, A, m, n, lda, sA, b1, m - 1, lo, hi, sn, 0, x1, sn, w1, sn, state, sn, r1, it, info, b));
        ARG(qr_bvls_batched_dev(p, A, m, n, lda, sA, b1, sm, lo, hi, n - 1, 0, x1, sn, w1, sn, state, sn, r1, it, info, b));
        ARG(qr_bvls_batched_dev(p, A, qr_bvls_batched_max_rows(n) + 1, n, 600, 600LL * n, b1, 600, lo, hi, sn, 0, x1, sn, w1, sn, state, sn, r1, it, info, b));
        /* irls */
        for (int loss = QR_LOSS_LS; loss <= QR_LOSS_BISQUARE; ++loss) {
            CALL(qr_irls_batched_dev(p, loss, 0.0, A, m, n, lda, sA, b1, sm, prior, sm, sc, x0, sn, 1e-8, 0, x1, sn, wm, sm, sc, r1, it, stt, info, b));
            CALL(qr_irls_batched_dev(p, loss, 2.0, A, m, n, lda, sA, b1, sm, prior, 0, NULL, NULL, 0, 0.0, 3, x1, sn, NULL, 0, NULL, NULL, NULL, NULL, info, b));
        }
        CALL(qr_gels_weighted_batched_dev(p, A, m, n, lda, sA, b1, sm, prior, sm, x1, sn, r1, info, b));
        CALL(qr_gels_weighted_batched_dev(p, A, m, n, lda, sA, b1, sm, NULL, 0, x1, sn, NULL, info, b));
        ARG(qr_irls_batched_dev(p, 3, 0.0, A, m, n, lda, sA, b1, sm, prior, sm, sc, x0, sn, 1e-8, 0, x1, sn, wm, sm, sc, r1, it, stt, info, b));
        ARG(qr_irls_batched_dev(p, 1, 0.0, A, m, n, lda, sA, b1, sm, prior, m - 1, sc, x0, sn, 1e-8, 0, x1, sn, wm, sm, sc, r1, it, stt, info, b));
        ARG(qr_irls_batched_dev(p, 1, 0.0, A, m, n, lda, sA, b1, sm, prior, sm, sc, x0, sn, -1.0, 0, x1, sn, wm, sm, sc, r1, it, stt, info, b));
        /* stats */
        CALL(qr_covar_batched_dev(p, A, n, lda, sA, state, sn, it, r1, Cv, ldx, ST(ldx, n), se, sn, info, b));
        CALL(qr_covar_batched_dev(p, A, n, lda, sA, NULL, 0, NULL, NULL, NULL, 0, 0, se, sn, info, b));
        CALL(qr_covar_batched_dev(p, A, n, lda, sA, NULL, 0, NULL, NULL, Cv, ldx, ST(ldx, n), NULL, 0, info, b));
        CALL(qr_leverage_batched_dev(p, A, n, lda, sA, state, sn, it, A, m, lda, sA, prior, sm, H, sm, info, b));
        CALL(qr_leverage_batched_dev(p, A, n, lda, sA, NULL, 0, NULL, A, m, lda, sA, NULL, 0, H, sm, info, b));
        for (int scaled = QR_COV_UNSCALED; scaled <= QR_COV_SCALED; ++scaled) {
            CALL(qr_gels_stats_batched_dev(p, scaled, A, m, n, lda, sA, b1, sm, prior, sm, x1, sn, E, sm, H, sm, sc, dof, Cv, ldx, ST(ldx, n), se, sn, info, b));
            CALL(qr_gels_stats_batched_dev(p, scaled, A, m, n, lda, sA, b1, sm, NULL, 0, x1, sn, NULL, 0, NULL, 0, NULL, NULL, NULL, 0, 0, NULL, 0, info, b));
        }
        ARG(qr_covar_batched_dev(p, A, n, lda, sA, NULL, 0, NULL, NULL, NULL, 0, 0, NULL, 0, info, b));
        ARG(qr_covar_batched_dev(p, A, n, n - 1, sA, NULL, 0, NULL, NULL, Cv, ldx, ST(ldx, n), se, sn, info, b));
        ARG(qr_leverage_batched_dev(p, A, n, lda, sA, NULL, 0, NULL, A, m, m - 1, sA, NULL, 0, H, sm, info, b));
        ARG(qr_gels_stats_batched_dev(p, 2, A, m, n, lda, sA, b1, sm, prior, sm, x1, sn, E, sm, H, sm, sc, dof, Cv, ldx, ST(ldx, n), se, sn, info, b));
        /* lsei */
        if (mg >= 1) {
            double *G = DB(mg, n), *h = DV(mg), *MU = DV(mg), *Sl = DV(mg);
            int* stg = DI(mg);
            CALL(qr_lsei_batched_dev(p, A, m, n, lda, sA, b1, sm, G, mg, neq, ldg, ST(ldg, n), h, sg, 0, 0.0, x1, sn, MU, sg, Sl, sg, stg, sg, r1, it, info, b));
            CALL(qr_lsei_batched_dev(p, A, m, n, lda, sA, b1, sm, G, mg, neq, ldg, 0, h, 0, 7, 1e-10, x1, sn, NULL, 0, NULL, 0, NULL, 0, NULL, NULL, info, b));
            ARG(qr_lsei_batched_dev(p, A, m, n, lda, sA, b1, sm, G, mg, mg + 1, ldg, ST(ldg, n), h, sg, 0, 0.0, x1, sn, MU, sg, Sl, sg, stg, sg, r1, it, info, b));
            ARG(qr_lsei_batched_dev(p, A, m, n, lda, sA, b1, sm, G, mg, neq, mg - 1, ST(ldg, n), h, sg, 0, 0.0, x1, sn, MU, sg, Sl, sg, stg, sg, r1, it, info, b));
            ARG(qr_lsei_batched_dev(p, A, m, n, lda, sA, b1, sm, G, 65, neq, 65, 65LL * n, h, 65, 0, 0.0, x1, sn, MU, sg, Sl, sg, stg, sg, r1, it, info, b));
        }
    }
    CALL(qr_plan_sync(p));
    CALL(qr_plan_destroy(p));
}
static void bconstrained_wave(void) { const bshape s = {40, 7, 1, 5, 1, 3}; bconstrained_on(&s, 2, 9, 2); }
static void bconstrained_wave_edge(void) { const bshape s = {64, 31, 1, 1, 3, 0}; bconstrained_on(&s, 31, 64, 31); }      /* n + 1 == 32, p == n, mg at its limit */
static void bconstrained_wg(void) { const bshape s = {65, 7, 17, 5, 1, 1}; bconstrained_on(&s, 1, 1, 0); }               /* m == 65: a workgroup per member */
static void bconstrained_wg_cols(void) { const bshape s = {64, 32, 1, 3, 1, 5}; bconstrained_on(&s, 5, 3, 3); }         /* n + 1 == 33 */
static void bconstrained_limit(void) { const bshape s = {256, 60, 4, 2, 1, 1}; bconstrained_on(&s, 3, 2, 1); }
static void bconstrained_twins(void)
{
    const int m = 40, n = 7, b = 5, pc = 2, mg = 9, neq = 2;
    double *A = hostd((size_t) m * n * b), *C = hostd((size_t) pc * n * b), *B = hostd((size_t) m * 17 * b), *d = hostd((size_t) pc * 17 * b),
           *X = hostd((size_t) n * 17 * b), *L = hostd((size_t) pc * 17 * b), *res = hostd((size_t) 17 * b), *lo = hostd((size_t) n * b),
           *W = hostd((size_t) m * b), *sc = hostd(b), *E = hostd((size_t) m * b), *H = hostd((size_t) m * b), *Cv = hostd((size_t) n * n * b),
           *se = hostd((size_t) n * b), *G = hostd((size_t) mg * n * b), *h = hostd((size_t) mg * b), *MU = hostd((size_t) mg * b), *Sl = hostd((size_t) mg * b);
    int *info = hosti(b), *state = hosti((size_t) mg * b), *it = hosti(b), *st = hosti(b), *dof = hosti(b);
    CALL(qr_lstsq_constrained_batched(A, m, n, C, pc, B, d, 17, b, X, L, res, info));
    CALL(qr_lstsq_constrained_batched(A, m, n, C, pc, B, d, 1, 1, X, NULL, NULL, info));
    CALL(qr_lstsq_constrained_batched(A, 5, n, C, pc, B, d, 1, b, X, L, res, info));          /* m < n: the plan is n x n */
    CALL(qr_lstsq_bounded_batched(A, m, n, B, lo, lo, 0, b, X, W, state, res, it, info));
    CALL(qr_lstsq_bounded_batched(A, m, n, B, NULL, NULL, 3, 1, X, NULL, NULL, NULL, NULL, info));
    CALL(qr_lstsq_robust_batched(A, m, n, B, QR_LOSS_HUBER, 0.0, W, sc, lo, 1e-8, 0, b, X, W, sc, res, it, st, info));
    CALL(qr_lstsq_robust_batched(A, m, n, B, QR_LOSS_LS, 0.0, NULL, NULL, NULL, 0.0, 0, 1, X, NULL, NULL, NULL, NULL, NULL, info));
    CALL(qr_lstsq_stats_batched(A, m, n, B, W, QR_COV_SCALED, b, X, E, H, sc, dof, Cv, se, info));
    CALL(qr_lstsq_stats_batched(A, m, n, B, NULL, QR_COV_UNSCALED, 1, X, NULL, NULL, NULL, NULL, NULL, NULL, info));
    CALL(qr_lstsq_inequality_batched(A, m, n, B, G, mg, neq, h, 0, 0.0, b, X, MU, Sl, state, res, it, info));
    CALL(qr_lstsq_inequality_batched(A, 5, n, B, G, mg, neq, h, 4, 1e-9, 1, X, NULL, NULL, NULL, NULL, NULL, info));
    qrd_stub_set_info(1);
    CALLX(qr_lstsq_constrained_batched(A, m, n, C, pc, B, d, 1, b, X, L, res, info), QR_E_SINGULAR);
    CALLX(qr_lstsq_bounded_batched(A, m, n, B, lo, lo, 0, b, X, W, state, res, it, info), QR_E_SINGULAR);
    CALLX(qr_lstsq_robust_batched(A, m, n, B, QR_LOSS_BISQUARE, 0.0, W, sc, lo, 1e-8, 0, b, X, W, sc, res, it, st, info), QR_E_SINGULAR);
    CALLX(qr_lstsq_stats_batched(A, m, n, B, W, QR_COV_SCALED, b, X, E, H, sc, dof, Cv, se, info), QR_E_SINGULAR);
    CALLX(qr_lstsq_inequality_batched(A, m, n, B, G, mg, neq, h, 0, 0.0, b, X, MU, Sl, state, res, it, info), QR_E_SINGULAR);
    qrd_stub_set_info(0);
    CALL(qr_lstsq_constrained_batched(A, m, n, C, pc, B, d, 1, 0, X, L, res, info));
    ARG(qr_lstsq_constrained_batched(A, m, n, C, n + 1, B, d, 1, b, X, L, res, info));
    ARG(qr_lstsq_bounded_batched(A, n - 1, n, B, lo, lo, 0, b, X, W, state, res, it, info));
    ARG(qr_lstsq_robust_batched(A, m, n, B, 5, 0.0, W, sc, lo, 1e-8, 0, b, X, W, sc, res, it, st, info));
    ARG(qr_lstsq_stats_batched(A, m, n, B, W, 7, b, X, E, H, sc, dof, Cv, se, info));
    ARG(qr_lstsq_inequality_batched(A, m, n, B, G, mg, mg + 1, h, 0, 0.0, b, X, MU, Sl, state, res, it, info));
}

/* ---- qr_batched_lm.c ---- */
static int lm_model(void* user, int what, const double* X, int batch, double* F, double* J)
{
    (void) X; (void) batch; (void) F; (void) J;
    int* calls = (int*) user;
    ++calls[what];
    return calls[0] && calls[what] > calls[0] ? 77 : 0;          /* calls[0]: the call of this kind that fails (0: none) */
}
/* a handle of either section behind the calls the two share */
typedef struct { int bounded; qr_lm_batched* u; qr_lmb_batched* b; } lm_any;
static int any_create(lm_any* a, qr_plan* p, int m, int n, int batch, const qr_lm_options* o)
{ return a->bounded ? qr_lmb_batched_create(&a->b, p, m, n, batch, o) : qr_lm_batched_create(&a->u, p, m, n, batch, o); }
static int any_start(lm_any* a, const double* X0, int ldx, long long sX, const double* D0, long long sD)
{ return a->bounded ? qr_lmb_batched_start_dev(a->b, X0, ldx, sX, D0, sD, NULL, 0, NULL, 0) : qr_lm_batched_start_dev(a->u, X0, ldx, sX, D0, sD); }
static int any_step(lm_any* a, double* J, int ldj, long long sJ, double* F, int ldf, long long sF)
{ return a->bounded ? qr_lmb_batched_step_dev(a->b, J, ldj, sJ, F, ldf, sF) : qr_lm_batched_step_dev(a->u, J, ldj, sJ, F, ldf, sF); }
static int any_update(lm_any* a, const double* F, int ldf, long long sF)
{ return a->bounded ? qr_lmb_batched_update_dev(a->b, F, ldf, sF) : qr_lm_batched_update_dev(a->u, F, ldf, sF); }
static int any_running(lm_any* a, int* count) { return a->bounded ? qr_lmb_batched_running(a->b, count) : qr_lm_batched_running(a->u, count); }
static int any_destroy(lm_any* a) { return a->bounded ? qr_lmb_batched_destroy(a->b) : qr_lm_batched_destroy(a->u); }
static void blm_on(const bshape* s, int bounded)
{
    qr_plan* p = NULL;
    lm_any h = {bounded, NULL, NULL};
    const char* upd = bounded ? "blmb_update" : "blm_update";
    CALL(qr_plan_create(&p, 64, 8, 0, 0));
    const int m = s->m, n = s->n, b = s->batch, ldj = LD(m), ldx = LD(n);
    const long long sJ = ST(ldj, n), sF = ST(ldj, 1), sX = ldx + s->gap, sn = n + s->gap;
    double *J = DB(m, n), *F = DB(m, 1), *X0 = dev_blocks(n, 1, ldx, b, sX), *D0 = DV(n), *Lo = DV(n), *Hi = dev_vec(n), *rss = PK(1);
    int* jp = DI(n);
    qr_lm_options o;
    qr_lm_options_default(&o);
    for (int mode = 1; mode <= 2; ++mode) {
        o.mode = mode;
        CALL(any_create(&h, p, m, n, b, mode == 1 ? NULL : &o));
        int count = -1;
        ARG(any_running(&h, &count));
        ARG(any_step(&h, J, ldj, sJ, F, ldj, sF));      /* before start */
        CALL(any_start(&h, X0, ldx, sX, D0, mode == 2 ? 0 : sn));
        CALL(any_start(&h, X0, ldx, sX, mode == 2 ? D0 : NULL, sn));
        if (bounded) {          /* the bounds: per member, one vector shared by all (stride 0), one side or both absent */
            CALL(qr_lmb_batched_start_dev(h.b, X0, ldx, sX, D0, sn, Lo, sn, Hi, 0));
            CALL(qr_lmb_batched_start_dev(h.b, X0, ldx, sX, D0, sn, Hi, 0, Lo, sn));
            CALL(qr_lmb_batched_start_dev(h.b, X0, ldx, sX, D0, sn, Lo, sn, NULL, -1));
            CALL(qr_lmb_batched_start_dev(h.b, X0, ldx, sX, D0, sn, NULL, -1, Hi, 0));
            ARG(qr_lmb_batched_start_dev(h.b, X0, ldx, sX, D0, sn, Lo, n - 1, Hi, 0));
            ARG(qr_lmb_batched_start_dev(h.b, X0, ldx, sX, D0, sn, Lo, sn, Hi, -1));
            /* a handle of section 8n is refused by every call of section 8m */
            qr_lm_batched* wrong = (qr_lm_batched*) h.b;
            qr_lm_batched_state wv;
            ARG(qr_lm_batched_start_dev(wrong, X0, ldx, sX, D0, sn));
            ARG(qr_lm_batched_step_dev(wrong, J, ldj, sJ, F, ldj, sF));
            ARG(qr_lm_step_batched_dev(wrong, J, ldj, sJ, F, m, ldj, sF, rss, jp, sn));
            ARG(qr_lm_batched_update_dev(wrong, F, ldj, sF));
            ARG(qr_lm_batched_running(wrong, &count));
            ARG(qr_lm_batched_view(wrong, &wv));
            ARG(qr_lm_batched_destroy(wrong));
        } else {                /* and the other way round */
            qr_lmb_batched* wrong = (qr_lmb_batched*) h.u;
            qr_lmb_batched_state wv;
            ARG(qr_lmb_batched_start_dev(wrong, X0, ldx, sX, D0, sn, NULL, 0, NULL, 0));
            ARG(qr_lmb_batched_step_dev(wrong, J, ldj, sJ, F, ldj, sF));
            ARG(qr_lmb_batched_update_dev(wrong, F, ldj, sF));
            ARG(qr_lmb_batched_running(wrong, &count));
            ARG(qr_lmb_batched_view(wrong, &wv));
            ARG(qr_lmb_batched_destroy(wrong));
        }
        CALL(any_step(&h, J, ldj, sJ, F, ldj, sF));
        ARG(any_step(&h, J, ldj, sJ, F, ldj, sF));      /* a step behind a step */
        const double keep = b > 1 ? b - 1 : 1;
        CALLS(qrd_stub_script(upd, &keep, 1), any_update(&h, F, ldj, sF), 0);
        CALL(any_running(&h, &count));
        if (count != (int) keep) { fprintf(stderr, "running %d\n", count); exit(1); }
        /* (the step from factors that exist is section 8m's alone) */
        CALL(bounded ? any_step(&h, J, ldj, sJ, F, ldj, sF) : qr_lm_step_batched_dev(h.u, J, ldj, sJ, F, m, ldj, sF, rss, jp, sn));
        ARG(any_update(&h, F, m - 1, sF));
        CALL(any_update(&h, F, ldj, sF));
        CALL(bounded ? any_step(&h, J, ldj, sJ, F, ldj, sF) : qr_lm_step_batched_dev(h.u, J, ldj, sJ, F, n, ldj, sF, NULL, NULL, 0));
        CALL(any_update(&h, F, ldj, sF));
        CALL(any_running(&h, &count));
        if (count != 0) { fprintf(stderr, "running %d after the last update\n", count); exit(1); }
        if (bounded) {
            qr_lmb_batched_state v;
            CALL(qr_lmb_batched_view(h.b, &v));
            if (!v.lo || !v.hi || !v.alpha || !v.peg || !v.clipped) { fprintf(stderr, "the view of a bounded handle lacks the bounds\n"); exit(1); }
        } else {
            qr_lm_batched_state v;
            CALL(qr_lm_batched_view(h.u, &v));
            ARG(qr_lm_step_batched_dev(h.u, J, n - 1, sJ, F, m, ldj, sF, rss, jp, sn));
        }
        ARG(any_start(&h, X0, n - 1, sX, D0, sn));
        CALL(any_destroy(&h));
    }
    ARG(any_create(&h, p, m, 64, b, NULL));
    ARG(any_create(&h, p, qr_batched_max_rows(n + 1) + 1, n, b, NULL));
    o.par_rtol = 1.0;
    ARG(any_create(&h, p, m, n, b, &o));
    CALL(any_create(&h, p, m, n, 0, NULL));
    CALL(any_start(&h, X0, ldx, sX, NULL, 0));
    CALL(any_destroy(&h));
    CALL(qr_plan_sync(p));
    CALL(qr_plan_destroy(p));
}
static void blm_wave(void) { const bshape s = {40, 7, 1, 5, 1, 3}; blm_on(&s, 0); }
static void blm_wave_edge(void) { const bshape s = {64, 31, 1, 1, 3, 0}; blm_on(&s, 0); }
static void blm_wg(void) { const bshape s = {256, 63, 1, 3, 1, 1}; blm_on(&s, 0); }
static void blmb_wave(void) { const bshape s = {40, 7, 1, 5, 1, 3}; blm_on(&s, 1); }
static void blmb_wave_edge(void) { const bshape s = {64, 31, 1, 1, 3, 0}; blm_on(&s, 1); }
static void blmb_wg(void) { const bshape s = {256, 63, 1, 3, 1, 1}; blm_on(&s, 1); }
/* the host-pointer twin of either section; lo, hi: section 8n's bounds (either may be NULL) */
static int twin_solve(int bounded, int* calls, int m, int n, int b, double* X, const double* lo, const double* hi, const double* D,
                      const qr_lm_options* o, double* fn, int* nfev, int* njev, int* st, int* info)
{
    return bounded ? qr_lstsq_lm_bounded_batched(lm_model, calls, m, n, b, X, lo, hi, D, o, fn, nfev, njev, st, info)
                   : qr_lstsq_lm_batched(lm_model, calls, m, n, b, X, D, o, fn, nfev, njev, st, info);
}
static void twin_on(int bounded)
{
    const int m = 40, n = 7, b = 5;
    const char* upd = bounded ? "blmb_update" : "blm_update";
    double *X = hostd((size_t) n * b), *D = hostd((size_t) n * b), *fn = hostd(b), *lo = hostd((size_t) n * b), *hi = hostd((size_t) n * b);
    int *nfev = hosti(b), *njev = hosti(b), *st = hosti(b), *info = hosti(b), calls[4] = {0, 0, 0, 0};
    qr_lm_options o;
    qr_lm_options_default(&o);
    CALL(twin_solve(bounded, calls, m, n, b, X, NULL, NULL, NULL, NULL, fn, nfev, njev, st, info));          /* every member finishes in the first round */
    /* four rounds: all running, one finished, a rejected step with two left, then the end */
    { const double w[4] = {5.0, 4.0, -2.0, 0.0}; memset(calls, 0, sizeof calls);
      CALLS(qrd_stub_script(upd, w, 4), twin_solve(bounded, calls, m, n, b, X, lo, hi, NULL, &o, NULL, NULL, NULL, NULL, info), 0);
      if (calls[3] < 4 && !g_fail_hits) { fprintf(stderr, "%d rounds\n", calls[3]); exit(1); } }
    o.mode = 2; o.maxfev = 3;          /* the round limit: maxfev + 2 rounds with every member still running */
    { memset(calls, 0, sizeof calls); CALLS(fill_script(upd, (double) b, 8), twin_solve(bounded, calls, m, n, b, X, lo, NULL, D, &o, fn, nfev, njev, st, info), 0);
      if (calls[3] != 5 && !g_fail_hits) { fprintf(stderr, "%d rounds at the limit\n", calls[3]); exit(1); } }
    fill_script(upd, 0.0, 0);
    for (int what = 1; what <= 3; ++what) {          /* the model fails: its code comes back, nothing leaks */
        memset(calls, 0, sizeof calls);
        calls[what] = 1; calls[0] = 1;
        CALLX(twin_solve(bounded, calls, m, n, b, X, NULL, hi, D, &o, fn, nfev, njev, st, info), 77);
    }
    memset(calls, 0, sizeof calls);
    qrd_stub_set_info(4);
    CALLX(twin_solve(bounded, calls, m, n, b, X, NULL, NULL, NULL, NULL, fn, nfev, njev, st, info), QR_E_SINGULAR);
    qrd_stub_set_info(0);
    if (bounded) {          /* two members that start refuses: QR_E_SINGULAR, and their X returns byte for byte as it came */
        const double refused = 2.0;
        double* X1 = hostd((size_t) n * b);
        for (int i = 0; i < n * b; ++i) X[i] = X1[i] = 1.5 + i;
        CALLS(qrd_stub_script("blmb_start", &refused, 1), twin_solve(1, calls, m, n, b, X, lo, hi, NULL, NULL, fn, nfev, njev, st, info), QR_E_SINGULAR);
        if (memcmp(X, X1, sizeof(double) * 2 * (size_t) n) || info[0] != -2 || info[1] != -2 || info[2] != 0) {
            fprintf(stderr, "a refused member's X or info: %d %d %d\n", info[0], info[1], info[2]); exit(1); }
    }
    CALL(twin_solve(bounded, calls, m, n, 0, X, NULL, NULL, NULL, NULL, fn, nfev, njev, st, info));
    ARG(bounded ? qr_lstsq_lm_bounded_batched(NULL, calls, m, n, b, X, lo, hi, NULL, NULL, fn, nfev, njev, st, info)
                : qr_lstsq_lm_batched(NULL, calls, m, n, b, X, NULL, NULL, fn, nfev, njev, st, info));
    ARG(twin_solve(bounded, calls, m, n, b, X, lo, hi, NULL, &o, fn, nfev, njev, st, info));          /* mode 2 without D */
    ARG(twin_solve(bounded, calls, n - 1, n, b, X, lo, hi, NULL, NULL, fn, nfev, njev, st, info));
}
static void blm_twin(void) { twin_on(0); }
static void blmb_twin(void) { twin_on(1); }

/* ================================================= threads (ThreadSanitizer) ================================================= */
/* four host threads, different host-pointer twins: two share a shape (one cached slot, one private plan), two grow the slot's buffers; the
 * first also runs the bounded Levenberg-Marquardt twin (a plan and a handle of its own per call) */
static void* thread_body(void* arg)
{
    const int id = (int) (size_t) arg, m = 40, n = 7, b = 5;
    double *A = (double*) calloc((size_t) m * n * b, sizeof(double)), *B = (double*) calloc((size_t) m * 17 * b, sizeof(double)),
           *X = (double*) calloc((size_t) m * 17 * b, sizeof(double)), *S = (double*) calloc(64, sizeof(double));
    int* info = (int*) calloc(64, sizeof(int));
    for (int i = 0; i < n; ++i) A[(size_t) i * m + i] = 1.0;
    for (int it = 0; it < 6; ++it) {
        const int nrhs = 1 + (it * 5 + id) % 17;
        switch (id) {
        case 0: { int calls[4] = {0, 0, 0, 0}; OK(qr_lstsq(A, m, n, B, nrhs, X, S));
                  OK(qr_lstsq_lm_bounded_batched(lm_model, calls, m, n, b, X, NULL, B, NULL, NULL, NULL, NULL, NULL, NULL, info)); break; }
        case 1: OK(qr_lstsq_svd(A, m, n, B, nrhs, -1.0, X, NULL, info, S)); break;          /* the same shape: the same slot, or a private plan */
        case 2: OK(qr_lstsq_pivoted(A, m, n, B, nrhs, -1.0, X, S, info, NULL)); OK(qr_lstsq_batched(A, m, n, B, 1, b, X, NULL, info)); break;
        default: { const int rc = qr_lstsq_minnorm(A, n, m, B, nrhs, X); if (rc && rc != QR_E_SINGULAR) OK(rc); OK(qr_svd(A, m, n, S, NULL, NULL)); break; }
        }
    }
    free(A); free(B); free(X); free(S); free(info);
    return NULL;
}
static void threads_run(void)
{
    pthread_t th[4];
    for (size_t i = 0; i < 4; ++i) pthread_create(&th[i], NULL, thread_body, (void*) i);
    for (int i = 0; i < 4; ++i) pthread_join(th[i], NULL);
}

typedef struct { const char* name; void (*run)(void); } config;
static const config g_cfg[] = {
    {"solve_tall", solve_tall}, {"solve_short", solve_short}, {"solve_aligned", solve_aligned}, {"solve_blocks", solve_blocks}, {"solve_subplan", solve_subplan}, {"solve_twin", solve_twin},
    {"pivot_general", pivot_general}, {"pivot_nt", pivot_nt}, {"pivot_subplan", pivot_subplan}, {"pivot_twin", pivot_twin},
    {"minnorm_tall", minnorm_tall}, {"minnorm_blocks", minnorm_blocks}, {"minnorm_subplan", minnorm_subplan}, {"minnorm_twin", minnorm_twin},
    {"update_primitives", update_primitives}, {"lsacc_small", lsacc_small}, {"lsacc_wide", lsacc_wide}, {"lsacc_subplan", lsacc_subplan},
    {"chunked_twin", chunked_twin}, {"downdate_primitives", downdate_primitives}, {"rolling_twin", rolling_twin},
    {"svd_three_blocks", svd_three_blocks}, {"svd_two_blocks", svd_two_blocks}, {"svd_one_block", svd_one_block}, {"svd_twin", svd_twin},
    {"batched_wave", batched_wave}, {"batched_wave_edge", batched_wave_edge}, {"batched_wg33", batched_wg33}, {"batched_wg64", batched_wg64},
    {"batched_composed", batched_composed}, {"batched_composed_wide_rhs", batched_composed_wide_rhs}, {"batched_twins", batched_twins},
    {"bupdate_wave", bupdate_wave}, {"bupdate_wave_edge", bupdate_wave_edge}, {"bupdate_wg_rows", bupdate_wg_rows}, {"bupdate_wg33", bupdate_wg33},
    {"bupdate_limit", bupdate_limit}, {"bupdate_wide_limit", bupdate_wide_limit}, {"brolling_twin", brolling_twin},
    {"bminnorm_wave", bminnorm_wave}, {"bminnorm_wave_edge", bminnorm_wave_edge}, {"bminnorm_wg33", bminnorm_wg33}, {"bminnorm_wg_rows", bminnorm_wg_rows},
    {"bminnorm_narrow_fit", bminnorm_narrow_fit}, {"bminnorm_composed", bminnorm_composed}, {"bminnorm_wide_rhs", bminnorm_wide_rhs},
    {"bdamped_twins", bdamped_twins},
    {"bconstrained_wave", bconstrained_wave}, {"bconstrained_wave_edge", bconstrained_wave_edge}, {"bconstrained_wg", bconstrained_wg},
    {"bconstrained_wg_cols", bconstrained_wg_cols}, {"bconstrained_limit", bconstrained_limit}, {"bconstrained_twins", bconstrained_twins},
    {"blm_wave", blm_wave}, {"blm_wave_edge", blm_wave_edge}, {"blm_wg", blm_wg}, {"blm_twin", blm_twin},
    {"blmb_wave", blmb_wave}, {"blmb_wave_edge", blmb_wave_edge}, {"blmb_wg", blmb_wg}, {"blmb_twin", blmb_twin},
};

int main(int argc, char** argv)
{
    const int ncfg = (int) (sizeof g_cfg / sizeof g_cfg[0]);
    if (argc < 2) { fprintf(stderr, "usage: host_units <configuration> | list | all | threads\n"); return 2; }
    if (!strcmp(argv[1], "list")) { for (int i = 0; i < ncfg; ++i) printf("%s\n", g_cfg[i].name); return 0; }
    setenv("QRD_STUB_ORDER", "count", 0);
    int ran = 0;
    if (!strcmp(argv[1], "threads")) { threads_run(); ran = 1; }
    for (int i = 0; i < ncfg; ++i)
        if (!strcmp(argv[1], "all") || !strcmp(argv[1], g_cfg[i].name)) {
            g_cfg[i].run();
            ++ran;
            dev_free_all();
            while (g_host_nbuf) free(g_host_buf[--g_host_nbuf]);
        }
    if (!ran) { fprintf(stderr, "host_units: no configuration '%s'\n", argv[1]); return 2; }
    OK(qr_release_cached_plans());
    if (qrd_stub_live_allocations() != 0) { fprintf(stderr, "device-memory leak: %d allocations still live\n", qrd_stub_live_allocations()); return 6; }
    printf("ORDER %ld\nLAUNCHES %ld\nFAILHITS %d\n", qrd_stub_order_reports(), qrd_stub_launches(), g_fail_hits);
    const long na = qrd_stub_alloc_count();
    for (long k = 1; k <= na; ++k) {
        size_t bytes = 0;
        const char *f = NULL, *e = NULL;
        if (qrd_stub_alloc_site(k, &bytes, &f, &e)) break;
        printf("ALLOC %ld %zu %s:%s\n", k, bytes, f, e);
    }
    return 0;
}
