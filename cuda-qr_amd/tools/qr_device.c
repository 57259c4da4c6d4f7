/* qr_device.c -- command-line timing harness in the shape of the reference's GPU binary
 * (reference qr.cu:709-806: `./qr_device m n`, srand(12) input, `trials` = 3 timed calls of the host-pointer
 * mmqr, average seconds printed as " MMQR ran QR on MxN matrix in T s (avg over 3)").
 *
 * Like the reference's timed region (qr.cu:776-789, which wraps cudaMalloc + H2D + kernels + D2H), the first
 * figure times the whole host-pointer call.  The second figure is the same factorisation with the matrix already
 * resident in HBM (what bench.py reports).  The reference silently rounds m and n to fit its window ladder
 * (qr.cu:722-734); this library takes any m >= n, so the sizes are used as given.
 *
 * `./qr_device m n --compare` adds the vendor line the reference prints under ENABLE_MAGMA (qr.cu:790-806, "MAGMA ran QR on ..."):
 * rocSOLVER's dgeqrf on the same matrix, resident in HBM.  rocSOLVER / rocBLAS are dlopen()ed by THIS tool only when the flag is
 * given: the library never links or loads them.
 *
 * `./qr_device m n --pivot` adds a line for the column-pivoted factorisation (qr_geqp3_dev, matrix resident in HBM): time, numerical
 * rank and the residual ||A P - Q R||_F / ||A||_F with Q and the product formed on the device.
 *
 * `./qr_device m n --minnorm` reads m n as a WIDE shape (m <= n) and does nothing else: the minimum-norm solution of A x = b for one
 * right-hand side (qr_gels_wide_dev, matrix resident in HBM, transpose included), time and ||A x - b|| / (||A||_F ||x||).
 *
 * `./qr_device m n --append [chunk_rows]` does nothing else either: the rows of the matrix are pushed into a least-squares accumulator
 * chunk_rows at a time (default 4096; qr_lsacc_push_dev, chunks resident in HBM), beside one qr_gels_dev on the whole matrix: both
 * times, the factor error ||R_acc^T R_acc - R^T R||_F / ||R^T R||_F and the solution error ||x_acc - x||_2 / ||x||_2.
 *
 * `./qr_device m n --svd` does nothing else either: the SVD of the matrix (qr_gesvd_dev with U and V, matrix resident in HBM): time,
 * sigma_max, sigma_min, the Jacobi sweeps, ||A - U S V^T||_F / ||A||_F and the two orthogonality errors ||U^T U - I||_F, ||V^T V - I||_F
 * (products formed on the host).
 *
 * `./qr_device m n --slide window step` does nothing else either: least squares over the windows [k step, k step + window) of the rows.
 * The first window is pushed into an accumulator, every later one is one qr_lsacc_slide_dev (step rows in, step rows out, rows resident
 * in HBM), beside one qr_gels_dev per window (window resident in HBM): both wall times, the time of the host-pointer qr_lstsq_rolling,
 * the largest solution error against the per-window solve, and the Gram drift ||R_acc^T R_acc - R^T R||_F / ||R^T R||_F at the last window.
 *
 * `./qr_device m n --batched count` does nothing else either: `count` seeded m x n matrices are factored in one qr_geqrf_batched_dev
 * call (batch resident in HBM), Q formed by qr_orgqr_batched_dev: the time of the factorisation and the worst backward error
 * ||A - Q R||_F / ||A||_F and orthogonality error ||Q^T Q - I||_F over the batch (products formed on the host).
 *
 * `./qr_device m n --batched count --pivot [rank]` does nothing else either: `count` seeded m x n matrices of that rank (products of
 * m x rank and rank x n factors; default n) and one right-hand side each go through one qr_gelsy_batched_dev call: the time, the
 * smallest and largest rank found, and the worst ||A^T (A x - b)|| / (||A||_F^2 ||x|| + ||A||_F ||b||) over the batch (zero at a
 * least-squares solution; formed on the host).
 *
 * `./qr_device m n --batched count --svd` does nothing else either: `count` seeded m x n matrices go through one qr_gesvd_batched_dev call
 * with U and V (batch resident in HBM): the time, the largest sweep count, and the worst ||A - U S V^T||_F / ||A||_F over the batch
 * (formed on the host).
 *
 * `./qr_device m n --batched count --minnorm` does nothing else either: m n is read as a wide shape (m <= n), `count` seeded m x n
 * matrices and one right-hand side each (resident in HBM) go through one qr_gels_wide_batched_dev call: the time, the worst
 * ||A x - b|| / (||A|| ||x||) and the worst distance of x from the row space of A.
 *
 * `./qr_device m n --batched count --damped nlam` does nothing else either: `count` seeded m x n matrices (m >= n), one right-hand side
 * and nlam values of lambda each (resident in HBM) go through one qr_gels_damped_batched_dev call: the time, and the worst forward error
 * ||x - x_s|| / ||x_s|| against nlam qr_gels_batched_dev solves of the stacked systems [A ; lambda I].
 *
 * `./qr_device m n --batched count --lse p` does nothing else either: `count` seeded m x n matrices A, p x n constraint matrices C and one
 * pair (b, d) each (resident in HBM) go through one qr_gglse_batched_dev call: the time, the worst ||C x - d|| / (||C|| ||x|| + ||d||), the
 * worst KKT residual ||A^T (A x - b) + C^T lambda|| / (||A|| (||A|| ||x|| + ||b||) + ||C|| ||lambda||) (Frobenius norms, formed on the host)
 * and the number of non-zero info words.
 *
 * `./qr_device m n --batched count --bvls` does nothing else either: `count` seeded planted problems min ||A x - b|| subject to
 * lo <= x <= hi (resident in HBM) go through one qr_bvls_batched_dev call.  A member is planted on the host: about half its variables are
 * drawn active, the residual r is a random vector made orthogonal to the free columns (Gram-Schmidt, twice), every active variable sits at
 * lo where a_j^T r < 0 and at hi where it is > 0, b = A x* + r: x* and the state are then the unique solution.  Printed: the time, the worst
 * stationarity measure max over free j of |a_j^T (b - A x)| / (||a_j|| (||A|| ||x|| + ||b||)) (Frobenius norms, formed on the host), the
 * number of variables whose state is not the planted one (and of non-zero info words), the mean and the largest elimination count.
 *
 * `./qr_device m n --batched count --lsei mg [neq]` does nothing else either: `count` seeded planted problems min ||A x - b|| subject to
 * G(0:neq) x = h(0:neq), G(neq:mg) x >= h(neq:mg) (resident in HBM; m >= n; neq defaults to 0) go through one qr_lsei_batched_dev call.  A
 * member is planted on the host: x* is drawn, min(floor(min(n, mg - neq) / 2), n - neq) inequality rows are active with multipliers in
 * [0.5, 1.5] (equality rows carry +-[0.5, 1.5]), the other rows have slack in [0.5, 1.5], h = G x* - slack and b = A x* - A z with
 * (A^T A) z = G^T mu* (Cholesky on the host): x*, mu* and the set are then the unique solution.  Printed: the time, the worst constraint
 * violation (|G_i x - h_i| on the rows of the set, its negative part elsewhere, over |G_i| |x| + |h_i|), the worst KKT residual
 * max_j |A^T (A x - b) - G^T mu|_j / (||a_j|| (||A|| ||x|| + ||b||) + (|G|^T |mu|)_j), the number of rows whose state is not the planted one,
 * the mean and the largest candidate count, and the number of non-zero info words.
 *
 * `./qr_device m n --batched count --robust frac` does nothing else either: `count` seeded planted problems b = A x* + 0.01 noise with a
 * fraction `frac` of the rows shifted by +-[0.1, 0.5] (resident in HBM) go through one qr_irls_batched_dev call with the Huber loss and its
 * defaults.  Printed: the time, the worst error ||x - x*|| / ||x*|| beside that of one qr_gels_batched_dev on copies of the same members,
 * the mean and the largest solve count, and the number of non-zero info words.
 *
 * `./qr_device m n --batched count --stats` does nothing else either: `count` seeded members b = A x* + 0.01 noise (resident in HBM) go
 * through one qr_gels_stats_batched_dev call with every output (QR_COV_UNSCALED, no weights).  Printed: the time, the worst |sum h - n|,
 * the worst ||C A^T A - I||_F (formed on the host), and the number of non-zero info words.
 *
 * `./qr_device m 3 --batched count --lm` does nothing else either: `count` seeded exponential-decay fits y = a exp(-b t) + c on m points of
 * [0, 4] (planted (a, b, c), zero residual, the start the planted values times 1.2 or 0.8) go through qr_lstsq_lm_batched, the host twin of
 * the batched Levenberg-Marquardt solver: the model runs on the host between the device calls, so the time is dominated by it and by the
 * copies.  Printed: the time, the worst ||x - planted||, the mean and the largest nfev, the number of non-zero info words and a histogram
 * of status.  With `--box` the fits go through qr_lstsq_lm_bounded_batched with 0 <= a, 0 <= b <= 0.8 planted b and 0 <= c (the rate bound
 * cuts off the free minimiser; b starts at half its bound): also printed are the fits that end with b on its bound and the entries
 * outside the box (0).
 *
 * `./qr_device m n --batched count --slide window step` does nothing else either: `count` seeded series of m rows, n unknowns and one
 * right-hand side each (resident in HBM) go through one batched accumulator -- the first window pushed, every later one ONE
 * qr_lsacc_batched_slide_dev for the whole batch -- beside one qr_gels_batched_dev per window on copies of the windows: both wall times
 * and the largest solution error ||x_acc - x||_2 / ||x||_2 over every window and series.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <dlfcn.h>

#include "mi355x_qr.h"

#define TRIALS 3

static double now(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

/* the comparator (qr.cu:555-565 magmaQR, timed at qr.cu:790-806): rocsolver_dgeqrf(handle, m, n, dA, lda, dtau), column-major in place */
static int vendor_line(const double* A, double* dA, double* dtau, int m, int n, double flops)
{
    void* hb = dlopen("librocblas.so.5", RTLD_NOW | RTLD_GLOBAL);
    if (!hb) hb = dlopen("librocblas.so", RTLD_NOW | RTLD_GLOBAL);
    void* hs = dlopen("librocsolver.so.0", RTLD_NOW | RTLD_GLOBAL);
    if (!hs) hs = dlopen("librocsolver.so", RTLD_NOW | RTLD_GLOBAL);
    void* hh = dlopen("libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!hb || !hs || !hh) { printf("rocSOLVER not available on this machine (%s)\n", dlerror()); return 0; }
    int (*create)(void**) = (int (*)(void**)) dlsym(hb, "rocblas_create_handle");
    int (*destroy)(void*) = (int (*)(void*)) dlsym(hb, "rocblas_destroy_handle");
    int (*geqrf)(void*, int, int, double*, int, double*) = (int (*)(void*, int, int, double*, int, double*)) dlsym(hs, "rocsolver_dgeqrf");
    int (*devsync)(void) = (int (*)(void)) dlsym(hh, "hipDeviceSynchronize");
    void* handle = NULL;
    if (!create || !destroy || !geqrf || !devsync || create(&handle)) { printf("rocSOLVER not usable on this machine\n"); return 0; }
    double el = 0.0;
    for (int t = -1; t < TRIALS; t++) {             /* t = -1: untimed first call (workspace, kernel loading) */
        if (qr_copy_to_device(dA, A, sizeof(double) * (size_t) m * n)) return 1;
        devsync();
        const double t0 = now();
        if (geqrf(handle, m, n, dA, m, dtau) || devsync()) { fprintf(stderr, "rocsolver_dgeqrf failed\n"); destroy(handle); return 1; }
        if (t >= 0) el += now() - t0;
    }
    destroy(handle);
    printf("rocSOLVER ran QR on %dx%d matrix in %f s (avg over %d)   [matrix resident in HBM, %.1f GFLOP/s fp64]\n",
           m, n, el / TRIALS, TRIALS, flops / (el / TRIALS) / 1e9);
    return 0;
}

/* qr_geqp3_dev on the resident matrix: time, rank, ||A P - Q R||_F / ||A||_F */
static int pivot_line(qr_plan* p, const double* A, double* dA, double* dtau, int m, int n)
{
    const size_t cnt = (size_t) m * n;
    int* djpvt = NULL;
    double *dQ = NULL, *dR = NULL, *dC = NULL;
    if (qr_device_malloc((void**) &djpvt, sizeof(int) * n) || qr_device_malloc((void**) &dQ, sizeof(double) * cnt) ||
        qr_device_malloc((void**) &dR, sizeof(double) * (size_t) n * n) || qr_device_malloc((void**) &dC, sizeof(double) * cnt)) {
        fprintf(stderr, "device setup failed\n");
        return 1;
    }
    double el = 0.0;
    for (int t = -1; t < TRIALS; t++) {
        if (qr_copy_to_device(dA, A, sizeof(double) * cnt)) { fprintf(stderr, "copy failed\n"); return 1; }
        const double t0 = now();
        if (qr_geqp3_dev(p, dA, m, n, m, djpvt, dtau) || qr_plan_sync(p)) { fprintf(stderr, "qr_geqp3_dev failed\n"); return 1; }
        if (t >= 0) el += now() - t0;
    }
    int rank = -1;
    int* jpvt = malloc(sizeof(int) * n);
    double* QR = malloc(sizeof(double) * cnt);
    if (!jpvt || !QR || qr_rank_dev(p, dA, m, n, m, -1.0, &rank) || qr_applyq_dev(p, dA, m, n, m, dtau, dQ, n, m, 1) ||
        qr_extract_r_dev(p, dA, m, n, m, dR, n, n) || qr_gemm_dev(p, 'N', m, n, n, 1.0, dQ, m, dR, n, 0.0, dC, m) || qr_plan_sync(p) ||
        qr_copy_to_host(QR, dC, sizeof(double) * cnt) || qr_copy_to_host(jpvt, djpvt, sizeof(int) * n)) {
        fprintf(stderr, "pivoted check failed\n");
        return 1;
    }
    double num = 0.0, den = 0.0;
    for (int j = 0; j < n; j++)
        for (int i = 0; i < m; i++) {
            const double a = A[(size_t) jpvt[j] * m + i], d = a - QR[(size_t) j * m + i];
            num += d * d; den += a * a;
        }
    printf(" MMQR ran pivoted QR on %dx%d matrix in %f s (avg over %d)   [matrix resident in HBM, rank %d, residual %.2e]\n",
           m, n, el / TRIALS, TRIALS, rank, sqrt(num / den));
    free(jpvt); free(QR);
    qr_device_free(djpvt); qr_device_free(dQ); qr_device_free(dR); qr_device_free(dC);
    return 0;
}

/* the wide m x n system (m <= n), one right-hand side: qr_gels_wide_dev on the resident matrix */
static int minnorm_main(int m, int n)
{
    if (m < 1 || m > n) { fprintf(stderr, "--minnorm needs 1 <= m <= n\n"); return 1; }
    printf("Exact problem size: %dx%d (wide)\n", m, n);
    const size_t cnt = (size_t) m * n;
    double* A = malloc(sizeof(double) * cnt);
    double* b = malloc(sizeof(double) * n);
    double* x = malloc(sizeof(double) * n);
    if (!A || !b || !x) { fprintf(stderr, "out of memory\n"); return 1; }
    srand(12);
    for (size_t i = 0; i < cnt; i++) A[i] = (double) rand() / RAND_MAX;
    for (int i = 0; i < n; i++) b[i] = i < m ? (double) rand() / RAND_MAX : 0.0;
    qr_plan* p = NULL;
    double *dA = NULL, *dF = NULL, *dtau = NULL, *dB = NULL;
    if (qr_plan_create(&p, n, m, 0, 0) || qr_device_malloc((void**) &dA, sizeof(double) * cnt) ||
        qr_device_malloc((void**) &dF, sizeof(double) * cnt) || qr_device_malloc((void**) &dtau, sizeof(double) * m) ||
        qr_device_malloc((void**) &dB, sizeof(double) * n) || qr_copy_to_device(dA, A, sizeof(double) * cnt)) {
        fprintf(stderr, "device setup failed\n");
        return 1;
    }
    double el = 0.0;
    for (int t = -1; t < TRIALS; t++) {
        if (qr_copy_to_device(dB, b, sizeof(double) * n)) { fprintf(stderr, "copy failed\n"); return 1; }
        const double t0 = now();
        if (qr_gels_wide_dev(p, dA, m, n, m, dF, n, dtau, dB, 1, n) || qr_plan_sync(p)) { fprintf(stderr, "qr_gels_wide_dev failed\n"); return 1; }
        if (t >= 0) el += now() - t0;
    }
    if (qr_copy_to_host(x, dB, sizeof(double) * n)) { fprintf(stderr, "copy failed\n"); return 1; }
    double na = 0.0, nx = 0.0, nr = 0.0;
    for (size_t i = 0; i < cnt; i++) na += A[i] * A[i];
    for (int j = 0; j < n; j++) nx += x[j] * x[j];
    for (int i = 0; i < m; i++) {
        double r = -b[i];
        for (int j = 0; j < n; j++) r += A[(size_t) j * m + i] * x[j];
        nr += r * r;
    }
    printf(" MMQR ran minimum-norm solve on %dx%d matrix in %f s (avg over %d)   [matrix resident in HBM, ||A x - b|| / (||A|| ||x||) = %.2e]\n",
           m, n, el / TRIALS, TRIALS, sqrt(nr) / (sqrt(na) * sqrt(nx)));
    qr_device_free(dA); qr_device_free(dF); qr_device_free(dtau); qr_device_free(dB);
    qr_plan_destroy(p);
    free(A); free(b); free(x);
    return 0;
}

/* R^T R of the n x n upper triangle in the leading rows of F (ld ldf) into G (n x n) */
static void gram_of_triangle(const double* F, int ldf, int n, double* G)
{
    for (int j = 0; j < n; j++)
        for (int i = 0; i <= j; i++) {
            double s = 0.0;
            for (int k = 0; k <= i; k++) s += F[(size_t) i * ldf + k] * F[(size_t) j * ldf + k];
            G[(size_t) j * n + i] = G[(size_t) i * n + j] = s;
        }
}

/* m x n, one right-hand side: the rows pushed chunk by chunk into a qr_lsacc against one qr_gels_dev on the whole matrix */
static int append_main(int m, int n, int chunk)
{
    if (n < 1 || m < n || chunk < 1) { fprintf(stderr, "--append needs m >= n >= 1 and chunk_rows >= 1\n"); return 1; }
    if (chunk > m) chunk = m;
    printf("Exact problem size: %dx%d, pushed %d rows at a time\n", m, n, chunk);
    const size_t cnt = (size_t) m * n, nn = (size_t) n * n;
    double *A = malloc(sizeof(double) * cnt), *b = malloc(sizeof(double) * m), *F = malloc(sizeof(double) * cnt), *xb = malloc(sizeof(double) * m);
    double *Ra = malloc(sizeof(double) * nn), *xa = malloc(sizeof(double) * n), *G0 = malloc(sizeof(double) * nn), *G1 = malloc(sizeof(double) * nn);
    double *Ac = malloc(sizeof(double) * (size_t) chunk * n);
    if (!A || !b || !F || !xb || !Ra || !xa || !G0 || !G1 || !Ac) { fprintf(stderr, "out of memory\n"); return 1; }
    srand(12);
    for (size_t i = 0; i < cnt; i++) A[i] = (double) rand() / RAND_MAX - 0.5;
    for (int i = 0; i < m; i++) b[i] = (double) rand() / RAND_MAX - 0.5;
    const int pm = chunk > n ? chunk : n;
    qr_plan *p = NULL, *pc = NULL;
    qr_lsacc* acc = NULL;
    double *dA = NULL, *dtau = NULL, *dB = NULL, *dAc = NULL, *dBc = NULL, *dX = NULL;
    if (qr_plan_create(&p, m, n, 0, 0) || qr_plan_create(&pc, pm, n, 0, 0) || qr_lsacc_create(&acc, pc, n, 1) ||
        qr_device_malloc((void**) &dA, sizeof(double) * cnt) || qr_device_malloc((void**) &dtau, sizeof(double) * n) ||
        qr_device_malloc((void**) &dB, sizeof(double) * m) || qr_device_malloc((void**) &dAc, sizeof(double) * (size_t) chunk * n) ||
        qr_device_malloc((void**) &dBc, sizeof(double) * chunk) || qr_device_malloc((void**) &dX, sizeof(double) * n)) {
        fprintf(stderr, "device setup failed\n");
        return 1;
    }
    double el = 0.0, ela = 0.0;
    for (int t = -1; t < TRIALS; t++) {
        if (qr_copy_to_device(dA, A, sizeof(double) * cnt) || qr_copy_to_device(dB, b, sizeof(double) * m)) { fprintf(stderr, "copy failed\n"); return 1; }
        const double t0 = now();
        if (qr_gels_dev(p, dA, m, n, m, dtau, dB, 1, m) || qr_plan_sync(p)) { fprintf(stderr, "qr_gels_dev failed\n"); return 1; }
        if (t >= 0) el += now() - t0;
        if (qr_lsacc_reset(acc) || qr_plan_sync(pc)) { fprintf(stderr, "qr_lsacc_reset failed\n"); return 1; }
        for (int r = 0; r < m; r += chunk) {          /* the uploads are not timed: the chunks count as resident, like the matrix above */
            const int h = m - r < chunk ? m - r : chunk;
            for (int j = 0; j < n; j++) memcpy(Ac + (size_t) j * h, A + (size_t) j * m + r, sizeof(double) * h);
            if (qr_copy_to_device(dAc, Ac, sizeof(double) * (size_t) h * n) || qr_copy_to_device(dBc, b + r, sizeof(double) * h)) { fprintf(stderr, "copy failed\n"); return 1; }
            const double t1 = now();
            if (qr_lsacc_push_dev(acc, dAc, h, h, dBc, h) || qr_plan_sync(pc)) { fprintf(stderr, "qr_lsacc_push_dev failed\n"); return 1; }
            if (t >= 0) ela += now() - t1;
        }
        const double t2 = now();
        if (qr_lsacc_solve_dev(acc, dX, n, NULL) || qr_plan_sync(pc)) { fprintf(stderr, "qr_lsacc_solve_dev failed\n"); return 1; }
        if (t >= 0) ela += now() - t2;
    }
    const double* dR = NULL;
    int ldr = 0;
    if (qr_lsacc_factor_dev(acc, &dR, &ldr, NULL, NULL) || qr_copy_to_host(Ra, dR, sizeof(double) * nn) || qr_copy_to_host(xa, dX, sizeof(double) * n) ||
        qr_copy_to_host(F, dA, sizeof(double) * cnt) || qr_copy_to_host(xb, dB, sizeof(double) * m)) { fprintf(stderr, "copy failed\n"); return 1; }
    gram_of_triangle(F, m, n, G0);
    gram_of_triangle(Ra, ldr, n, G1);
    double gn = 0.0, gd = 0.0, xn = 0.0, xd = 0.0;
    for (size_t i = 0; i < nn; i++) { gn += (G1[i] - G0[i]) * (G1[i] - G0[i]); gd += G0[i] * G0[i]; }
    for (int i = 0; i < n; i++) { xn += (xa[i] - xb[i]) * (xa[i] - xb[i]); xd += xb[i] * xb[i]; }
    printf(" MMQR ran least squares on %dx%d matrix in %f s (avg over %d)   [qr_gels_dev, matrix resident in HBM]\n", m, n, el / TRIALS, TRIALS);
    printf(" MMQR ran the same in chunks of %d rows in %f s (avg over %d)   [accumulator; factor error %.2e, solution error %.2e]\n",
           chunk, ela / TRIALS, TRIALS, sqrt(gn / gd), sqrt(xn / xd));
    qr_lsacc_destroy(acc);
    qr_device_free(dA); qr_device_free(dtau); qr_device_free(dB); qr_device_free(dAc); qr_device_free(dBc); qr_device_free(dX);
    qr_plan_destroy(p); qr_plan_destroy(pc);
    free(A); free(b); free(F); free(xb); free(Ra); free(xa); free(G0); free(G1); free(Ac);
    return 0;
}

/* m x n, one right-hand side, windows of `window` rows every `step` rows: an accumulator that slides against one qr_gels_dev per window */
static int slide_main(int m, int n, int window, int step)
{
    if (n < 1 || window < n || window > m || step < 1 || step > window) { fprintf(stderr, "--slide needs m >= window >= n >= 1 and 1 <= step <= window\n"); return 1; }
    const int nwin = (m - window) / step + 1;
    printf("Exact problem size: %dx%d, %d windows of %d rows, %d rows apart\n", m, n, nwin, window, step);
    const size_t cnt = (size_t) m * n, wc = (size_t) window * n, sc = (size_t) step * n, nn = (size_t) n * n;
    double *A = malloc(sizeof(double) * cnt), *b = malloc(sizeof(double) * m), *Aw = malloc(sizeof(double) * wc), *F = malloc(sizeof(double) * wc);
    double *xs = malloc(sizeof(double) * (size_t) nwin * n), *xg = malloc(sizeof(double) * (size_t) nwin * n), *xr = malloc(sizeof(double) * (size_t) nwin * n);
    double *Ra = malloc(sizeof(double) * nn), *G0 = malloc(sizeof(double) * nn), *G1 = malloc(sizeof(double) * nn);
    if (!A || !b || !Aw || !F || !xs || !xg || !xr || !Ra || !G0 || !G1) { fprintf(stderr, "out of memory\n"); return 1; }
    srand(12);
    for (size_t i = 0; i < cnt; i++) A[i] = (double) rand() / RAND_MAX - 0.5;
    for (int i = 0; i < m; i++) b[i] = (double) rand() / RAND_MAX - 0.5;
    qr_plan* p = NULL;
    qr_lsacc* acc = NULL;
    double *dA = NULL, *dtau = NULL, *dB = NULL, *dN = NULL, *dO = NULL, *dbN = NULL, *dbO = NULL, *dX = NULL;
    if (qr_plan_create(&p, window, n, 0, 0) || qr_lsacc_create(&acc, p, n, 1) || qr_device_malloc((void**) &dA, sizeof(double) * wc) ||
        qr_device_malloc((void**) &dtau, sizeof(double) * n) || qr_device_malloc((void**) &dB, sizeof(double) * window) ||
        qr_device_malloc((void**) &dN, sizeof(double) * sc) || qr_device_malloc((void**) &dO, sizeof(double) * sc) ||
        qr_device_malloc((void**) &dbN, sizeof(double) * step) || qr_device_malloc((void**) &dbO, sizeof(double) * step) ||
        qr_device_malloc((void**) &dX, sizeof(double) * n)) {
        fprintf(stderr, "device setup failed\n");
        return 1;
    }
    double elg = 0.0, els = 0.0, elr = 0.0;
    for (int t = -1; t < TRIALS; t++) {
        /* one qr_gels_dev per window; the uploads are not timed: the rows count as resident on both sides */
        for (int k = 0; k < nwin; k++) {
            for (int j = 0; j < n; j++) memcpy(Aw + (size_t) j * window, A + (size_t) j * m + (size_t) k * step, sizeof(double) * window);
            if (qr_copy_to_device(dA, Aw, sizeof(double) * wc) || qr_copy_to_device(dB, b + (size_t) k * step, sizeof(double) * window)) { fprintf(stderr, "copy failed\n"); return 1; }
            const double t0 = now();
            if (qr_gels_dev(p, dA, window, n, window, dtau, dB, 1, window) || qr_plan_sync(p)) { fprintf(stderr, "qr_gels_dev failed\n"); return 1; }
            if (t >= 0) elg += now() - t0;
            if (qr_copy_to_host(xg + (size_t) k * n, dB, sizeof(double) * n)) { fprintf(stderr, "copy failed\n"); return 1; }
        }
        if (qr_copy_to_host(F, dA, sizeof(double) * wc)) { fprintf(stderr, "copy failed\n"); return 1; }       /* the last window's factor */
        /* the accumulator: window 0 pushed (dA, dB are its workspace), then one slide per window */
        for (int j = 0; j < n; j++) memcpy(Aw + (size_t) j * window, A + (size_t) j * m, sizeof(double) * window);
        if (qr_lsacc_reset(acc) || qr_copy_to_device(dA, Aw, sizeof(double) * wc) || qr_copy_to_device(dB, b, sizeof(double) * window)) { fprintf(stderr, "copy failed\n"); return 1; }
        for (int k = 0; k < nwin; k++) {
            int rc = 0;
            if (k > 0) {
                const size_t o = (size_t) (k - 1) * step, e = o + window;
                for (int j = 0; j < n; j++) {
                    memcpy(Aw + (size_t) j * step, A + (size_t) j * m + e, sizeof(double) * step);
                    memcpy(Aw + sc + (size_t) j * step, A + (size_t) j * m + o, sizeof(double) * step);
                }
                if (qr_copy_to_device(dN, Aw, sizeof(double) * sc) || qr_copy_to_device(dO, Aw + sc, sizeof(double) * sc) ||
                    qr_copy_to_device(dbN, b + e, sizeof(double) * step) || qr_copy_to_device(dbO, b + o, sizeof(double) * step)) { fprintf(stderr, "copy failed\n"); return 1; }
            }
            const double t1 = now();
            rc = k ? qr_lsacc_slide_dev(acc, dN, step, step, dbN, step, dO, step, step, dbO, step) : qr_lsacc_push_dev(acc, dA, window, window, dB, window);
            if (!rc) rc = qr_lsacc_solve_dev(acc, dX, n, NULL);
            if (!rc) rc = qr_plan_sync(p);
            if (rc) { fprintf(stderr, "window %d failed: %s\n", k, qr_strerror(rc)); return 1; }
            if (t >= 0) els += now() - t1;
            if (qr_copy_to_host(xs + (size_t) k * n, dX, sizeof(double) * n)) { fprintf(stderr, "copy failed\n"); return 1; }
        }
        const double t2 = now();
        const int rr = qr_lstsq_rolling(A, m, n, m, b, 1, m, window, step, xr, NULL);
        if (rr) { fprintf(stderr, "qr_lstsq_rolling failed: %s\n", qr_strerror(rr)); return 1; }
        if (t >= 0) elr += now() - t2;
    }
    const double* dR = NULL;
    int ldr = 0;
    if (qr_lsacc_factor_dev(acc, &dR, &ldr, NULL, NULL) || qr_copy_to_host(Ra, dR, sizeof(double) * nn)) { fprintf(stderr, "copy failed\n"); return 1; }
    gram_of_triangle(F, window, n, G0);
    gram_of_triangle(Ra, ldr, n, G1);
    double gn = 0.0, gd = 0.0, worst = 0.0, worst_r = 0.0;
    for (size_t i = 0; i < nn; i++) { gn += (G1[i] - G0[i]) * (G1[i] - G0[i]); gd += G0[i] * G0[i]; }
    for (int k = 0; k < nwin; k++) {
        double xn = 0.0, xd = 0.0, rn = 0.0;
        for (int i = 0; i < n; i++) {
            const double g = xg[(size_t) k * n + i], ds = xs[(size_t) k * n + i] - g, dr = xr[(size_t) k * n + i] - g;
            xn += ds * ds; rn += dr * dr; xd += g * g;
        }
        if (sqrt(xn / xd) > worst) worst = sqrt(xn / xd);
        if (sqrt(rn / xd) > worst_r) worst_r = sqrt(rn / xd);
    }
    printf(" MMQR ran least squares on %d windows of %dx%d in %f s (avg over %d)   [one qr_gels_dev per window, window resident in HBM]\n",
           nwin, window, n, elg / TRIALS, TRIALS);
    printf(" MMQR ran the same by sliding %d rows at a time in %f s (avg over %d)   [accumulator, rows resident in HBM; largest solution error %.2e, Gram drift at the last window %.2e]\n",
           step, els / TRIALS, TRIALS, worst, sqrt(gn / gd));
    printf(" MMQR ran the same from host memory in %f s (avg over %d)   [qr_lstsq_rolling, uploads included; largest solution error %.2e]\n",
           elr / TRIALS, TRIALS, worst_r);
    qr_lsacc_destroy(acc);
    qr_device_free(dA); qr_device_free(dtau); qr_device_free(dB); qr_device_free(dN); qr_device_free(dO); qr_device_free(dbN); qr_device_free(dbO); qr_device_free(dX);
    qr_plan_destroy(p);
    qr_release_cached_plans();
    free(A); free(b); free(Aw); free(F); free(xs); free(xg); free(xr); free(Ra); free(G0); free(G1);
    return 0;
}

/* ||X^T X - I||_F of the rows x cols column-major X */
static double orth_err(const double* X, int rows, int cols)
{
    double e = 0.0;
    for (int j = 0; j < cols; j++)
        for (int i = 0; i <= j; i++) {
            double s = i == j ? -1.0 : 0.0;
            for (int k = 0; k < rows; k++) s += X[(size_t) i * rows + k] * X[(size_t) j * rows + k];
            e += (i == j ? 1.0 : 2.0) * s * s;
        }
    return sqrt(e);
}

/* m x n, m >= n: qr_gesvd_dev with both sets of vectors on the resident matrix */
static int svd_main(int m, int n)
{
    if (n < 1 || m < n) { fprintf(stderr, "--svd needs m >= n >= 1\n"); return 1; }
    printf("Exact problem size: %dx%d\n", m, n);
    const size_t cnt = (size_t) m * n, nn = (size_t) n * n;
    double *A = malloc(sizeof(double) * cnt), *U = malloc(sizeof(double) * cnt), *V = malloc(sizeof(double) * nn), *S = malloc(sizeof(double) * n);
    if (!A || !U || !V || !S) { fprintf(stderr, "out of memory\n"); return 1; }
    srand(12);
    for (size_t i = 0; i < cnt; i++) A[i] = (double) rand() / RAND_MAX - 0.5;
    qr_plan* p = NULL;
    double *dA = NULL, *dtau = NULL, *dS = NULL, *dU = NULL, *dV = NULL;
    if (qr_plan_create(&p, m, n, 0, 0) || qr_device_malloc((void**) &dA, sizeof(double) * cnt) || qr_device_malloc((void**) &dtau, sizeof(double) * n) ||
        qr_device_malloc((void**) &dS, sizeof(double) * n) || qr_device_malloc((void**) &dU, sizeof(double) * cnt) ||
        qr_device_malloc((void**) &dV, sizeof(double) * nn)) {
        fprintf(stderr, "device setup failed\n");
        return 1;
    }
    double el = 0.0;
    int sweeps = 0;
    for (int t = -1; t < TRIALS; t++) {
        if (qr_copy_to_device(dA, A, sizeof(double) * cnt)) { fprintf(stderr, "copy failed\n"); return 1; }
        const double t0 = now();
        const int rc = qr_gesvd_dev(p, 'U', 'V', dA, m, n, m, dtau, dS, dU, m, dV, n, &sweeps);
        if (rc || qr_plan_sync(p)) { fprintf(stderr, "qr_gesvd_dev failed: %s\n", qr_strerror(rc)); return 1; }
        if (t >= 0) el += now() - t0;
    }
    if (qr_copy_to_host(U, dU, sizeof(double) * cnt) || qr_copy_to_host(V, dV, sizeof(double) * nn) || qr_copy_to_host(S, dS, sizeof(double) * n)) {
        fprintf(stderr, "copy failed\n");
        return 1;
    }
    double na = 0.0, nr = 0.0;
    for (int j = 0; j < n; j++)
        for (int i = 0; i < m; i++) {
            double s = -A[(size_t) j * m + i];
            for (int k = 0; k < n; k++) s += U[(size_t) k * m + i] * S[k] * V[(size_t) k * n + j];
            nr += s * s;
            na += A[(size_t) j * m + i] * A[(size_t) j * m + i];
        }
    printf(" MMQR ran SVD on %dx%d matrix in %f s (avg over %d)   [matrix resident in HBM, U and V formed]\n", m, n, el / TRIALS, TRIALS);
    printf(" sigma_max = %.6e  sigma_min = %.6e  sweeps = %d\n", S[0], S[n - 1], sweeps);
    printf(" ||A - U S V^T|| / ||A|| = %.2e   ||U^T U - I|| = %.2e   ||V^T V - I|| = %.2e\n", sqrt(nr / na), orth_err(U, m, n), orth_err(V, n, n));
    qr_device_free(dA); qr_device_free(dtau); qr_device_free(dS); qr_device_free(dU); qr_device_free(dV);
    qr_plan_destroy(p);
    free(A); free(U); free(V); free(S);
    return 0;
}

/* count matrices of m x n in one batched call */
static int batched_main(int m, int n, int count)
{
    if (n < 1 || n > QR_BATCHED_MAX_N || m < n || count < 1) {     /* (how tall a matrix may be is the library's answer: QR_E_ARG below) */
        fprintf(stderr, "--batched needs count >= 1 and 1 <= n <= %d, n <= m\n", QR_BATCHED_MAX_N);
        return 1;
    }
    printf("Exact problem size: %d matrices of %dx%d\n", count, m, n);
    const size_t mn = (size_t) m * n, cnt = mn * count;
    double *A = malloc(sizeof(double) * cnt), *F = malloc(sizeof(double) * cnt), *Q = malloc(sizeof(double) * cnt);
    if (!A || !F || !Q) { fprintf(stderr, "out of memory\n"); return 1; }
    srand(12);
    for (size_t i = 0; i < cnt; i++) A[i] = (double) rand() / RAND_MAX - 0.5;
    qr_plan* p = NULL;
    double *dA = NULL, *dQ = NULL, *dtau = NULL;
    if (qr_plan_create(&p, m, n, 0, 0) || qr_device_malloc((void**) &dA, sizeof(double) * cnt) || qr_device_malloc((void**) &dQ, sizeof(double) * cnt) ||
        qr_device_malloc((void**) &dtau, sizeof(double) * (size_t) n * count)) {
        fprintf(stderr, "device setup failed\n");
        return 1;
    }
    double el = 0.0;
    for (int t = -1; t < TRIALS; t++) {
        if (qr_copy_to_device(dA, A, sizeof(double) * cnt)) { fprintf(stderr, "copy failed\n"); return 1; }
        const double t0 = now();
        int rc = qr_geqrf_batched_dev(p, dA, m, n, m, (long long) mn, dtau, n, count);
        if (!rc) rc = qr_plan_sync(p);
        if (rc) {
            fprintf(stderr, "qr_geqrf_batched_dev failed: %s%s\n", qr_strerror(rc), rc == QR_E_ARG ? " (the matrix does not fit the LDS: see qr_batched_max_rows)" : "");
            return 1;
        }
        if (t >= 0) el += now() - t0;
    }
    if (qr_orgqr_batched_dev(p, dA, m, n, m, (long long) mn, dtau, n, dQ, m, (long long) mn, count) || qr_plan_sync(p) ||
        qr_copy_to_host(F, dA, sizeof(double) * cnt) || qr_copy_to_host(Q, dQ, sizeof(double) * cnt)) {
        fprintf(stderr, "qr_orgqr_batched_dev failed\n");
        return 1;
    }
    double worst = 0.0, worst_o = 0.0;
    for (int q = 0; q < count; q++) {
        const double *a = A + q * mn, *f = F + q * mn, *qq = Q + q * mn;
        double num = 0.0, den = 0.0;
        for (int j = 0; j < n; j++)
            for (int i = 0; i < m; i++) {
                double s = -a[(size_t) j * m + i];
                for (int k = 0; k <= j; k++) s += qq[(size_t) k * m + i] * f[(size_t) j * m + k];
                num += s * s;
                den += a[(size_t) j * m + i] * a[(size_t) j * m + i];
            }
        if (sqrt(num / den) > worst) worst = sqrt(num / den);
        const double o = orth_err(qq, m, n);
        if (o > worst_o) worst_o = o;
    }
    const double flops = (2.0 * m * (double) n * n - 2.0 * (double) n * n * n / 3.0) * count;
    printf(" MMQR ran QR on %d %dx%d matrices in %f s (avg over %d)   [batch resident in HBM, %.1f GFLOP/s fp64]\n", count, m, n, el / TRIALS,
           TRIALS, flops / (el / TRIALS) / 1e9);
    printf(" worst ||A - Q R|| / ||A|| = %.2e   worst ||Q^T Q - I|| = %.2e\n", worst, worst_o);
    qr_device_free(dA); qr_device_free(dQ); qr_device_free(dtau);
    qr_plan_destroy(p);
    free(A); free(F); free(Q);
    return 0;
}

/* count series of m rows through one batched accumulator, window by window, beside one batched solve per window */
static int batched_slide_main(int m, int n, int count, int window, int step)
{
    const int nrhs = 1;
    if (n < 1 || n + nrhs > QR_BATCHED_MAX_N || count < 1 || window < n || window > m || step < 1 || step > window ||
        2 * step > qr_tpqrt_batched_max_rows(n + nrhs) || window > qr_batched_max_rows(n + nrhs)) {
        fprintf(stderr, "--batched count --slide window step needs count >= 1, 1 <= n < %d, n <= window <= min(m, %d), 1 <= step <= window and "
                        "2 step <= %d\n", QR_BATCHED_MAX_N, qr_batched_max_rows(n + nrhs), qr_tpqrt_batched_max_rows(n + nrhs));
        return 1;
    }
    const int nwin = (m - window) / step + 1;
    printf("Exact problem size: %d series of %dx%d, %d windows of %d rows, step %d\n", count, m, n, nwin, window, step);
    const size_t mn = (size_t) m * n, wn = (size_t) window * n, nb = (size_t) count;
    double *A = malloc(sizeof(double) * nb * mn), *B = malloc(sizeof(double) * nb * m), *X = malloc(sizeof(double) * nb * n),
           *C = malloc(sizeof(double) * nb * window);
    int* info = malloc(sizeof(int) * nb);
    if (!A || !B || !X || !C || !info) { fprintf(stderr, "out of memory\n"); return 1; }
    srand(12);
    for (size_t i = 0; i < nb * mn; i++) A[i] = (double) rand() / RAND_MAX - 0.5;
    for (size_t i = 0; i < nb * m; i++) B[i] = (double) rand() / RAND_MAX - 0.5;
    qr_plan* p = NULL;
    qr_lsacc_batched* acc = NULL;
    double *dA = NULL, *dB = NULL, *dW = NULL, *dC = NULL, *dtau = NULL, *dX = NULL;
    int* dinfo = NULL;
    if (qr_plan_create(&p, window, n, 0, 0) || qr_lsacc_batched_create(&acc, p, n, nrhs, count) ||
        qr_device_malloc((void**) &dA, sizeof(double) * nb * mn) || qr_device_malloc((void**) &dB, sizeof(double) * nb * m) ||
        qr_device_malloc((void**) &dW, sizeof(double) * nb * wn) || qr_device_malloc((void**) &dC, sizeof(double) * nb * window) ||
        qr_device_malloc((void**) &dtau, sizeof(double) * nb * n) || qr_device_malloc((void**) &dX, sizeof(double) * nb * n) ||
        qr_device_malloc((void**) &dinfo, sizeof(int) * nb) || qr_copy_to_device(dA, A, sizeof(double) * nb * mn) ||
        qr_copy_to_device(dB, B, sizeof(double) * nb * m)) {
        fprintf(stderr, "device setup failed\n");
        return 1;
    }
    double el_acc = 0.0, el_ref = 0.0, worst = 0.0;
    int bad = 0;
    for (int k = 0; k < nwin; k++) {
        const size_t o = (size_t) (k - 1) * step, e = o + window;
        double t0 = now();
        int rc = k == 0 ? qr_lsacc_batched_push_dev(acc, dA, window, m, (long long) mn, dB, m, m)
                        : qr_lsacc_batched_slide_dev(acc, dA + e, step, m, (long long) mn, dB + e, m, m, dA + o, step, m, (long long) mn, dB + o,
                                                     m, m, dinfo);
        if (!rc && k > 0) rc = qr_copy_to_host(info, dinfo, sizeof(int) * nb);         /* (waits: the slide's info words) */
        for (size_t q = 0; !rc && k > 0 && q < nb; q++) bad += info[q] != 0;
        if (!rc) rc = qr_lsacc_batched_solve_dev(acc, dX, n, n, NULL, 0, dinfo);
        if (!rc) rc = qr_plan_sync(p);
        if (rc) { fprintf(stderr, "the batched accumulator failed at window %d: %s\n", k, qr_strerror(rc)); return 1; }
        el_acc += now() - t0;
        if (qr_copy_to_host(X, dX, sizeof(double) * nb * n)) { fprintf(stderr, "copy failed\n"); return 1; }
        /* the same window from scratch: copies of its rows, one fused qr_gels_batched_dev */
        for (size_t q = 0; q < nb; q++) {
            for (int j = 0; j < n; j++)
                if (qr_copy_to_device(dW + q * wn + (size_t) j * window, A + q * mn + (size_t) j * m + (size_t) k * step, sizeof(double) * window)) return 1;
            if (qr_copy_to_device(dC + q * window, B + q * m + (size_t) k * step, sizeof(double) * window)) return 1;
        }
        t0 = now();
        rc = qr_gels_batched_dev(p, dW, window, n, window, (long long) wn, dtau, n, dC, nrhs, window, window, dinfo, count);
        if (!rc) rc = qr_plan_sync(p);
        if (rc) { fprintf(stderr, "qr_gels_batched_dev failed: %s\n", qr_strerror(rc)); return 1; }
        el_ref += now() - t0;
        if (qr_copy_to_host(C, dC, sizeof(double) * nb * window)) { fprintf(stderr, "copy failed\n"); return 1; }
        for (size_t q = 0; q < nb; q++) {
            double num = 0.0, den = 0.0;
            for (int i = 0; i < n; i++) {
                const double x = C[q * window + i], d = X[q * n + i] - x;
                num += d * d;
                den += x * x;
            }
            if (sqrt(num / den) > worst) worst = sqrt(num / den);
        }
    }
    printf(" MMQR slid %d series of n=%d over %d windows in %f s (one launch per slide, the info words read back each time)\n", count, n, nwin,
           el_acc);
    printf(" one qr_gels_batched_dev per window instead: %f s\n", el_ref);
    printf(" largest ||x_acc - x|| / ||x|| over every window and series = %.2e   (%d slides refused)\n", worst, bad);
    qr_lsacc_batched_destroy(acc);
    qr_device_free(dA); qr_device_free(dB); qr_device_free(dW); qr_device_free(dC); qr_device_free(dtau); qr_device_free(dX); qr_device_free(dinfo);
    qr_plan_destroy(p);
    free(A); free(B); free(X); free(C); free(info);
    return 0;
}

/* count matrices of m x n and of rank `rank` through one pivoted least-squares call */
static int batched_pivot_main(int m, int n, int count, int rank)
{
    if (n < 1 || n > QR_BATCHED_MAX_N || m < n || count < 1 || rank < 1 || rank > n) {
        fprintf(stderr, "--batched count --pivot [rank] needs count >= 1, 1 <= rank <= n <= %d, n <= m\n", QR_BATCHED_MAX_N);
        return 1;
    }
    printf("Exact problem size: %d matrices of %dx%d, rank %d\n", count, m, n, rank);
    const size_t mn = (size_t) m * n, cnt = mn * count;
    double *A = malloc(sizeof(double) * cnt), *B = malloc(sizeof(double) * (size_t) m * count), *X = malloc(sizeof(double) * (size_t) m * count);
    double *U = malloc(sizeof(double) * (size_t) m * rank), *W = malloc(sizeof(double) * (size_t) rank * n);
    int* rk = malloc(sizeof(int) * (size_t) count);
    if (!A || !B || !X || !U || !W || !rk) { fprintf(stderr, "out of memory\n"); return 1; }
    srand(12);
    for (int q = 0; q < count; q++) {
        double* a = A + q * mn;
        if (rank == n) {
            for (size_t i = 0; i < mn; i++) a[i] = (double) rand() / RAND_MAX - 0.5;
        } else {
            for (size_t i = 0; i < (size_t) m * rank; i++) U[i] = (double) rand() / RAND_MAX - 0.5;
            for (size_t i = 0; i < (size_t) rank * n; i++) W[i] = (double) rand() / RAND_MAX - 0.5;
            for (int j = 0; j < n; j++)
                for (int i = 0; i < m; i++) {
                    double s = 0.0;
                    for (int k = 0; k < rank; k++) s += U[(size_t) k * m + i] * W[(size_t) j * rank + k];
                    a[(size_t) j * m + i] = s;
                }
        }
        for (int i = 0; i < m; i++) B[(size_t) q * m + i] = (double) rand() / RAND_MAX - 0.5;
    }
    qr_plan* p = NULL;
    double *dA = NULL, *dB = NULL, *dtau = NULL;
    int *dj = NULL, *drank = NULL;
    if (qr_plan_create(&p, m, n, 0, 0) || qr_device_malloc((void**) &dA, sizeof(double) * cnt) ||
        qr_device_malloc((void**) &dB, sizeof(double) * (size_t) m * count) || qr_device_malloc((void**) &dtau, sizeof(double) * (size_t) n * count) ||
        qr_device_malloc((void**) &dj, sizeof(int) * (size_t) n * count) || qr_device_malloc((void**) &drank, sizeof(int) * (size_t) count)) {
        fprintf(stderr, "device setup failed\n");
        return 1;
    }
    double el = 0.0;
    for (int t = -1; t < TRIALS; t++) {
        if (qr_copy_to_device(dA, A, sizeof(double) * cnt) || qr_copy_to_device(dB, B, sizeof(double) * (size_t) m * count)) {
            fprintf(stderr, "copy failed\n");
            return 1;
        }
        const double t0 = now();
        int rc = qr_gelsy_batched_dev(p, dA, m, n, m, (long long) mn, dj, n, dtau, n, dB, 1, m, m, -1.0, NULL, drank, count);
        if (!rc) rc = qr_plan_sync(p);
        if (rc) {
            fprintf(stderr, "qr_gelsy_batched_dev failed: %s%s\n", qr_strerror(rc), rc == QR_E_ARG ? " (the matrix does not fit the LDS: see qr_batched_max_rows)" : "");
            return 1;
        }
        if (t >= 0) el += now() - t0;
    }
    if (qr_copy_to_host(X, dB, sizeof(double) * (size_t) m * count) || qr_copy_to_host(rk, drank, sizeof(int) * (size_t) count)) {
        fprintf(stderr, "copy back failed\n");
        return 1;
    }
    int rmin = rk[0], rmax = rk[0];
    double worst = 0.0;
    for (int q = 0; q < count; q++) {
        const double *a = A + q * mn, *b = B + (size_t) q * m, *x = X + (size_t) q * m;
        if (rk[q] < rmin) rmin = rk[q];
        if (rk[q] > rmax) rmax = rk[q];
        double na = 0.0, nx = 0.0, nb = 0.0, ng = 0.0;
        for (size_t i = 0; i < mn; i++) na += a[i] * a[i];
        for (int j = 0; j < n; j++) nx += x[j] * x[j];
        for (int i = 0; i < m; i++) nb += b[i] * b[i];
        for (int i = 0; i < m; i++) {         /* U's first m entries as scratch: the residual A x - b */
            double s = -b[i];
            for (int j = 0; j < n; j++) s += a[(size_t) j * m + i] * x[j];
            U[i] = s;
        }
        for (int j = 0; j < n; j++) {
            double s = 0.0;
            for (int i = 0; i < m; i++) s += a[(size_t) j * m + i] * U[i];
            ng += s * s;
        }
        const double den = na * sqrt(nx) + sqrt(na) * sqrt(nb);
        if (den > 0.0 && sqrt(ng) / den > worst) worst = sqrt(ng) / den;
    }
    printf(" MMQR ran pivoted least squares on %d %dx%d matrices in %f s (avg over %d)   [batch resident in HBM, one right-hand side each]\n", count,
           m, n, el / TRIALS, TRIALS);
    printf(" ranks found: %d .. %d (built with rank %d)   worst ||A^T (A x - b)|| / (||A||^2 ||x|| + ||A|| ||b||) = %.2e\n", rmin, rmax, rank, worst);
    qr_device_free(dA); qr_device_free(dB); qr_device_free(dtau); qr_device_free(dj); qr_device_free(drank);
    qr_plan_destroy(p);
    free(A); free(B); free(X); free(U); free(W); free(rk);
    return 0;
}

/* count matrices of m x n through one batched SVD call */
static int batched_svd_main(int m, int n, int count)
{
    if (n < 1 || n > QR_BATCHED_MAX_N || m < n || count < 1) {
        fprintf(stderr, "--batched count --svd needs count >= 1 and 1 <= n <= %d, n <= m\n", QR_BATCHED_MAX_N);
        return 1;
    }
    printf("Exact problem size: %d matrices of %dx%d\n", count, m, n);
    const size_t mn = (size_t) m * n, nn = (size_t) n * n, cnt = mn * count;
    double *A = malloc(sizeof(double) * cnt), *U = malloc(sizeof(double) * cnt), *V = malloc(sizeof(double) * nn * count);
    double* S = malloc(sizeof(double) * (size_t) n * count);
    int *sw = malloc(sizeof(int) * (size_t) count), *info = malloc(sizeof(int) * (size_t) count);
    if (!A || !U || !V || !S || !sw || !info) { fprintf(stderr, "out of memory\n"); return 1; }
    srand(12);
    for (size_t i = 0; i < cnt; i++) A[i] = (double) rand() / RAND_MAX - 0.5;
    qr_plan* p = NULL;
    double *dA = NULL, *dtau = NULL, *dS = NULL, *dU = NULL, *dV = NULL;
    int *dj = NULL, *dsw = NULL, *dinfo = NULL;
    if (qr_plan_create(&p, m, n, 0, 0) || qr_device_malloc((void**) &dA, sizeof(double) * cnt) || qr_device_malloc((void**) &dU, sizeof(double) * cnt) ||
        qr_device_malloc((void**) &dV, sizeof(double) * nn * count) || qr_device_malloc((void**) &dtau, sizeof(double) * (size_t) n * count) ||
        qr_device_malloc((void**) &dS, sizeof(double) * (size_t) n * count) || qr_device_malloc((void**) &dj, sizeof(int) * (size_t) n * count) ||
        qr_device_malloc((void**) &dsw, sizeof(int) * (size_t) count) || qr_device_malloc((void**) &dinfo, sizeof(int) * (size_t) count)) {
        fprintf(stderr, "device setup failed\n");
        return 1;
    }
    double el = 0.0;
    for (int t = -1; t < TRIALS; t++) {
        if (qr_copy_to_device(dA, A, sizeof(double) * cnt)) { fprintf(stderr, "copy failed\n"); return 1; }
        const double t0 = now();
        int rc = qr_gesvd_batched_dev(p, 'U', 'V', dA, m, n, m, (long long) mn, dj, n, dtau, n, dS, n, dU, m, (long long) mn, dV, n, (long long) nn,
                                      NULL, dsw, dinfo, count);
        if (!rc) rc = qr_plan_sync(p);
        if (rc) {
            fprintf(stderr, "qr_gesvd_batched_dev failed: %s%s\n", qr_strerror(rc), rc == QR_E_ARG ? " (the matrix does not fit the LDS: see qr_batched_max_rows)" : "");
            return 1;
        }
        if (t >= 0) el += now() - t0;
    }
    if (qr_copy_to_host(U, dU, sizeof(double) * cnt) || qr_copy_to_host(V, dV, sizeof(double) * nn * count) ||
        qr_copy_to_host(S, dS, sizeof(double) * (size_t) n * count) || qr_copy_to_host(sw, dsw, sizeof(int) * (size_t) count) ||
        qr_copy_to_host(info, dinfo, sizeof(int) * (size_t) count)) {
        fprintf(stderr, "copy back failed\n");
        return 1;
    }
    int swmax = 0, noconv = 0;
    double worst = 0.0;
    for (int q = 0; q < count; q++) {
        const double *a = A + q * mn, *u = U + q * mn, *v = V + q * nn, *sg = S + (size_t) q * n;
        if (sw[q] > swmax) swmax = sw[q];
        noconv += info[q] != 0;
        double num = 0.0, den = 0.0;
        for (int j = 0; j < n; j++)
            for (int i = 0; i < m; i++) {
                double s = -a[(size_t) j * m + i];
                for (int k = 0; k < n; k++) s += u[(size_t) k * m + i] * sg[k] * v[(size_t) k * n + j];
                num += s * s;
                den += a[(size_t) j * m + i] * a[(size_t) j * m + i];
            }
        if (den > 0.0 && sqrt(num / den) > worst) worst = sqrt(num / den);
    }
    printf(" MMQR ran the SVD of %d %dx%d matrices in %f s (avg over %d)   [batch resident in HBM, U and V formed]\n", count, m, n, el / TRIALS,
           TRIALS);
    printf(" largest sweep count = %d   not converged = %d   worst ||A - U S V^T|| / ||A|| = %.2e\n", swmax, noconv, worst);
    qr_device_free(dA); qr_device_free(dU); qr_device_free(dV); qr_device_free(dtau); qr_device_free(dS); qr_device_free(dj);
    qr_device_free(dsw); qr_device_free(dinfo);
    qr_plan_destroy(p);
    free(A); free(U); free(V); free(S); free(sw); free(info);
    return noconv ? 1 : 0;
}

/* count wide matrices of m x n through one batched minimum-norm call */
static int batched_minnorm_main(int m, int n, int count)
{
    if (m < 1 || m > QR_BATCHED_MAX_N || n < m || count < 1) {
        fprintf(stderr, "--batched count --minnorm needs count >= 1 and 1 <= m <= %d, m <= n\n", QR_BATCHED_MAX_N);
        return 1;
    }
    printf("Exact problem size: %d matrices of %dx%d\n", count, m, n);
    const size_t mn = (size_t) m * n, cnt = mn * count;
    double *A = malloc(sizeof(double) * cnt), *B = malloc(sizeof(double) * (size_t) n * count), *X = malloc(sizeof(double) * (size_t) n * count);
    double *F = malloc(sizeof(double) * cnt), *W = malloc(sizeof(double) * (size_t) n);
    int* info = malloc(sizeof(int) * (size_t) count);
    if (!A || !B || !X || !F || !W || !info) { fprintf(stderr, "out of memory\n"); return 1; }
    srand(12);
    for (size_t i = 0; i < cnt; i++) A[i] = (double) rand() / RAND_MAX - 0.5;
    for (int q = 0; q < count; q++)          /* dB is n rows tall: the right-hand side on top of zeros */
        for (int i = 0; i < n; i++) B[(size_t) q * n + i] = i < m ? (double) rand() / RAND_MAX - 0.5 : 0.0;
    qr_plan* p = NULL;
    double *dA = NULL, *dF = NULL, *dB = NULL, *dtau = NULL;
    int* dinfo = NULL;
    if (qr_plan_create(&p, n, m, 0, 0) || qr_device_malloc((void**) &dA, sizeof(double) * cnt) || qr_device_malloc((void**) &dF, sizeof(double) * cnt) ||
        qr_device_malloc((void**) &dB, sizeof(double) * (size_t) n * count) || qr_device_malloc((void**) &dtau, sizeof(double) * (size_t) m * count) ||
        qr_device_malloc((void**) &dinfo, sizeof(int) * (size_t) count) || qr_copy_to_device(dA, A, sizeof(double) * cnt)) {
        fprintf(stderr, "device setup failed\n");
        return 1;
    }
    double el = 0.0;
    for (int t = -1; t < TRIALS; t++) {
        if (qr_copy_to_device(dB, B, sizeof(double) * (size_t) n * count)) { fprintf(stderr, "copy failed\n"); return 1; }
        const double t0 = now();
        int rc = qr_gels_wide_batched_dev(p, dA, m, n, m, (long long) mn, dF, n, (long long) mn, dtau, m, dB, 1, n, n, dinfo, count);
        if (!rc) rc = qr_plan_sync(p);
        if (rc) {
            fprintf(stderr, "qr_gels_wide_batched_dev failed: %s%s\n", qr_strerror(rc), rc == QR_E_ARG ? " (the transpose does not fit the LDS: see qr_batched_max_rows)" : "");
            return 1;
        }
        if (t >= 0) el += now() - t0;
    }
    if (qr_copy_to_host(X, dB, sizeof(double) * (size_t) n * count) || qr_copy_to_host(F, dF, sizeof(double) * cnt) ||
        qr_copy_to_host(info, dinfo, sizeof(int) * (size_t) count)) {
        fprintf(stderr, "copy back failed\n");
        return 1;
    }
    int singular = 0;
    double worst = 0.0, worst_row = 0.0;
    for (int q = 0; q < count; q++) {
        if (info[q]) { singular++; continue; }
        const double *a = A + q * mn, *b = B + (size_t) q * n, *x = X + (size_t) q * n;
        double na = 0.0, nx = 0.0, nr = 0.0;
        for (size_t i = 0; i < mn; i++) na += a[i] * a[i];
        for (int j = 0; j < n; j++) nx += x[j] * x[j];
        for (int i = 0; i < m; i++) {
            double s = -b[i];
            for (int j = 0; j < n; j++) s += a[(size_t) j * m + i] * x[j];
            nr += s * s;
        }
        const double den = sqrt(na) * sqrt(nx);
        if (den > 0.0 && sqrt(nr) / den > worst) worst = sqrt(nr) / den;
        /* the distance of x from the row space of A: x minus its projection on the rows, by modified Gram-Schmidt twice over */
        double* rows = F + q * mn;            /* (the factors are needed no more: m orthonormalised rows of n entries each) */
        for (int i = 0; i < m; i++) {
            double* ri = rows + (size_t) i * n;
            for (int j = 0; j < n; j++) ri[j] = a[(size_t) j * m + i];
            for (int pass = 0; pass < 2; pass++)
                for (int k = 0; k < i; k++) {
                    const double* rk = rows + (size_t) k * n;
                    double d = 0.0;
                    for (int j = 0; j < n; j++) d += rk[j] * ri[j];
                    for (int j = 0; j < n; j++) ri[j] -= d * rk[j];
                }
            double nn = 0.0;
            for (int j = 0; j < n; j++) nn += ri[j] * ri[j];
            nn = sqrt(nn);
            for (int j = 0; j < n; j++) ri[j] = nn > 0.0 ? ri[j] / nn : 0.0;
        }
        memcpy(W, x, sizeof(double) * (size_t) n);
        for (int pass = 0; pass < 2; pass++)
            for (int k = 0; k < m; k++) {
                const double* rk = rows + (size_t) k * n;
                double d = 0.0;
                for (int j = 0; j < n; j++) d += rk[j] * W[j];
                for (int j = 0; j < n; j++) W[j] -= d * rk[j];
            }
        double nw = 0.0;
        for (int j = 0; j < n; j++) nw += W[j] * W[j];
        if (nx > 0.0 && sqrt(nw / nx) > worst_row) worst_row = sqrt(nw / nx);
    }
    printf(" MMQR ran minimum-norm solves of %d %dx%d systems in %f s (avg over %d)   [batch resident in HBM, one right-hand side each]\n", count,
           m, n, el / TRIALS, TRIALS);
    printf(" singular = %d   worst ||A x - b|| / (||A|| ||x||) = %.2e   worst distance of x from the row space / ||x|| = %.2e\n", singular, worst,
           worst_row);
    qr_device_free(dA); qr_device_free(dF); qr_device_free(dB); qr_device_free(dtau); qr_device_free(dinfo);
    qr_plan_destroy(p);
    free(A); free(B); free(X); free(F); free(W); free(info);
    return 0;
}

/* count matrices of m x n and nlam values of lambda each through one fused damped call, beside nlam stacked plain solves */
static int batched_damped_main(int m, int n, int count, int nlam)
{
    if (n < 1 || n >= QR_BATCHED_MAX_N || m < n || count < 1 || nlam < 1) {
        fprintf(stderr, "--batched count --damped nlam needs count >= 1, nlam >= 1 and 1 <= n < %d, n <= m\n", QR_BATCHED_MAX_N);
        return 1;
    }
    printf("Exact problem size: %d matrices of %dx%d, %d lambdas each\n", count, m, n, nlam);
    const int ms = m + n;
    const size_t mn = (size_t) m * n, cnt = mn * count, sn = (size_t) ms * n, nx = (size_t) n * nlam;
    double *A = malloc(sizeof(double) * cnt), *B = malloc(sizeof(double) * (size_t) m * count), *X = malloc(sizeof(double) * nx * count);
    double *S = malloc(sizeof(double) * sn * count), *C = malloc(sizeof(double) * (size_t) ms * count), *lam = malloc(sizeof(double) * (size_t) nlam);
    int* info = malloc(sizeof(int) * (size_t) count * nlam);
    if (!A || !B || !X || !S || !C || !lam || !info) { fprintf(stderr, "out of memory\n"); return 1; }
    srand(12);
    for (size_t i = 0; i < cnt; i++) A[i] = (double) rand() / RAND_MAX - 0.5;
    for (size_t i = 0; i < (size_t) m * count; i++) B[i] = (double) rand() / RAND_MAX - 0.5;
    for (int k = 0; k < nlam; k++) lam[k] = 0.05 * sqrt((double) m) * (k + 1);       /* one list for every member: stridelam = 0 */
    qr_plan* p = NULL;
    double *dA = NULL, *dB = NULL, *dtau = NULL, *dlam = NULL, *dX = NULL, *dS = NULL, *dC = NULL;
    int *dinfo = NULL, *dginfo = NULL;
    if (qr_plan_create(&p, m, n, 0, 0) || qr_device_malloc((void**) &dA, sizeof(double) * cnt) ||
        qr_device_malloc((void**) &dB, sizeof(double) * (size_t) m * count) || qr_device_malloc((void**) &dtau, sizeof(double) * (size_t) n * count) ||
        qr_device_malloc((void**) &dlam, sizeof(double) * (size_t) nlam) || qr_device_malloc((void**) &dX, sizeof(double) * nx * count) ||
        qr_device_malloc((void**) &dS, sizeof(double) * sn * count) || qr_device_malloc((void**) &dC, sizeof(double) * (size_t) ms * count) ||
        qr_device_malloc((void**) &dinfo, sizeof(int) * (size_t) count * nlam) || qr_device_malloc((void**) &dginfo, sizeof(int) * (size_t) count) ||
        qr_copy_to_device(dlam, lam, sizeof(double) * (size_t) nlam)) {
        fprintf(stderr, "device setup failed\n");
        return 1;
    }
    double el = 0.0;
    for (int t = -1; t < TRIALS; t++) {
        if (qr_copy_to_device(dA, A, sizeof(double) * cnt) || qr_copy_to_device(dB, B, sizeof(double) * (size_t) m * count)) {
            fprintf(stderr, "copy failed\n");
            return 1;
        }
        const double t0 = now();
        int rc = qr_gels_damped_batched_dev(p, dA, m, n, m, (long long) mn, dtau, n, dB, 1, m, m, NULL, 0, dlam, nlam, 0, dX, n, (long long) nx, NULL,
                                            NULL, dinfo, count);
        if (!rc) rc = qr_plan_sync(p);
        if (rc) {
            fprintf(stderr, "qr_gels_damped_batched_dev failed: %s%s\n", qr_strerror(rc), rc == QR_E_ARG ? " (the shape does not fit: see qr_batched_max_rows)" : "");
            return 1;
        }
        if (t >= 0) el += now() - t0;
    }
    if (qr_copy_to_host(X, dX, sizeof(double) * nx * count) || qr_copy_to_host(info, dinfo, sizeof(int) * (size_t) count * nlam)) {
        fprintf(stderr, "copy back failed\n");
        return 1;
    }
    int singular = 0, compared = 1;
    double worst = 0.0, els = 0.0;
    for (int k = 0; k < nlam && compared; k++) {     /* the route without the damped call: the stacked system, factored again per lambda */
        memset(S, 0, sizeof(double) * sn * count);
        memset(C, 0, sizeof(double) * (size_t) ms * count);
        for (int q = 0; q < count; q++) {
            for (int c = 0; c < n; c++) {
                memcpy(S + q * sn + (size_t) c * ms, A + q * mn + (size_t) c * m, sizeof(double) * (size_t) m);
                S[q * sn + (size_t) c * ms + m + c] = lam[k];
            }
            memcpy(C + (size_t) q * ms, B + (size_t) q * m, sizeof(double) * (size_t) m);
        }
        if (qr_copy_to_device(dS, S, sizeof(double) * sn * count) || qr_copy_to_device(dC, C, sizeof(double) * (size_t) ms * count)) {
            fprintf(stderr, "copy failed\n");
            return 1;
        }
        const double t0 = now();
        int rc = qr_gels_batched_dev(p, dS, ms, n, ms, (long long) sn, dtau, n, dC, 1, ms, ms, dginfo, count);
        if (!rc) rc = qr_plan_sync(p);
        if (rc == QR_E_ARG) { compared = 0; break; }  /* (m + n rows do not fit: nothing to compare against) */
        if (rc || qr_copy_to_host(C, dC, sizeof(double) * (size_t) ms * count)) { fprintf(stderr, "qr_gels_batched_dev failed\n"); return 1; }
        els += now() - t0;
        for (int q = 0; q < count; q++) {
            if (info[(size_t) q * nlam + k]) { singular++; continue; }
            const double *x = X + q * nx + (size_t) k * n, *xs = C + (size_t) q * ms;
            double nd = 0.0, ns = 0.0;
            for (int j = 0; j < n; j++) { nd += (x[j] - xs[j]) * (x[j] - xs[j]); ns += xs[j] * xs[j]; }
            if (ns > 0.0 && sqrt(nd / ns) > worst) worst = sqrt(nd / ns);
        }
    }
    printf(" MMQR ran damped solves of %d %dx%d systems for %d lambdas in %f s (avg over %d)   [batch resident in HBM, one right-hand side each]\n",
           count, m, n, nlam, el / TRIALS, TRIALS);
    if (compared)
        printf(" singular = %d   worst ||x - x_stacked|| / ||x_stacked|| = %.2e   (%d stacked qr_gels_batched_dev solves: %f s, with the copy back)\n",
               singular, worst, nlam, els);
    else
        printf(" the stacked (m + n) x n systems do not fit qr_gels_batched_dev: no comparison\n");
    qr_device_free(dA); qr_device_free(dB); qr_device_free(dtau); qr_device_free(dlam); qr_device_free(dX); qr_device_free(dS); qr_device_free(dC);
    qr_device_free(dinfo); qr_device_free(dginfo);
    qr_plan_destroy(p);
    free(A); free(B); free(X); free(S); free(C); free(lam); free(info);
    return 0;
}

/* count matrices of m x n through one trust-region call with Delta = frac x the Gauss-Newton |x| of each member */
static int batched_trust_main(int m, int n, int count, double frac)
{
    if (n < 1 || n >= QR_BATCHED_MAX_N || m < n || count < 1 || !(frac > 0.0)) {
        fprintf(stderr, "--batched count --trust frac needs count >= 1, frac > 0 and 1 <= n < %d, n <= m\n", QR_BATCHED_MAX_N);
        return 1;
    }
    printf("Exact problem size: %d matrices of %dx%d, Delta = %g x the Gauss-Newton step\n", count, m, n, frac);
    const size_t mn = (size_t) m * n, cnt = mn * count, nc = (size_t) count;
    double *A = malloc(sizeof(double) * cnt), *B = malloc(sizeof(double) * (size_t) m * count);
    double *delta = malloc(sizeof(double) * nc), *xn = malloc(sizeof(double) * nc);
    int *info = malloc(sizeof(int) * nc), *iter = malloc(sizeof(int) * nc);
    if (!A || !B || !delta || !xn || !info || !iter) { fprintf(stderr, "out of memory\n"); return 1; }
    srand(12);
    for (size_t i = 0; i < cnt; i++) A[i] = (double) rand() / RAND_MAX - 0.5;
    for (size_t i = 0; i < (size_t) m * count; i++) B[i] = (double) rand() / RAND_MAX - 0.5;
    const double zero = 0.0;
    qr_plan* p = NULL;
    double *dA = NULL, *dB = NULL, *dtau = NULL, *dX = NULL, *dv = NULL;
    int* di = NULL;
    if (qr_plan_create(&p, m, n, 0, 0) || qr_device_malloc((void**) &dA, sizeof(double) * cnt) ||
        qr_device_malloc((void**) &dB, sizeof(double) * (size_t) m * count) || qr_device_malloc((void**) &dtau, sizeof(double) * (size_t) n * count) ||
        qr_device_malloc((void**) &dX, sizeof(double) * (size_t) n * count) || qr_device_malloc((void**) &dv, sizeof(double) * (3 * nc + 1)) ||
        qr_device_malloc((void**) &di, sizeof(int) * 2 * nc) || qr_copy_to_device(dv + 3 * nc, &zero, sizeof(double))) {
        fprintf(stderr, "device setup failed\n");
        return 1;
    }
    double *ddelta = dv, *dlam = dv + nc, *dxn = dv + 2 * nc;
    double el = 0.0;
    for (int t = -2; t < TRIALS; t++) {               /* t == -2: the Gauss-Newton |x| of every member (lambda = 0), which sets the radii */
        if (qr_copy_to_device(dA, A, sizeof(double) * cnt) || qr_copy_to_device(dB, B, sizeof(double) * (size_t) m * count)) {
            fprintf(stderr, "copy failed\n");
            return 1;
        }
        const double t0 = now();
        int rc = t == -2 ? qr_gels_damped_batched_dev(p, dA, m, n, m, (long long) mn, dtau, n, dB, 1, m, m, NULL, 0, dv + 3 * nc, 1, 0, dX, n, n, dxn,
                                                      NULL, di, count)
                         : qr_gels_trust_batched_dev(p, dA, m, n, m, (long long) mn, dtau, n, dB, m, m, NULL, 0, ddelta, 1, NULL, 0, 0.1, 10, dX, n,
                                                     n, dlam, dxn, NULL, di + nc, NULL, di, count);
        if (!rc) rc = qr_plan_sync(p);
        if (rc) {
            fprintf(stderr, "the batched call failed: %s%s\n", qr_strerror(rc), rc == QR_E_ARG ? " (the shape does not fit: see qr_batched_max_rows)" : "");
            return 1;
        }
        if (t >= 0) el += now() - t0;
        if (t == -2) {
            if (qr_copy_to_host(xn, dxn, sizeof(double) * nc)) { fprintf(stderr, "copy back failed\n"); return 1; }
            for (size_t q = 0; q < nc; q++) delta[q] = frac * xn[q];
            if (qr_copy_to_device(ddelta, delta, sizeof(double) * nc)) { fprintf(stderr, "copy failed\n"); return 1; }
        }
    }
    if (qr_copy_to_host(xn, dxn, sizeof(double) * nc) || qr_copy_to_host(info, di, sizeof(int) * nc) || qr_copy_to_host(iter, di + nc, sizeof(int) * nc)) {
        fprintf(stderr, "copy back failed\n");
        return 1;
    }
    int failed = 0, most = 0;
    double worst = 0.0;
    for (size_t q = 0; q < nc; q++) {
        if (info[q]) { failed++; continue; }
        if (iter[q] > most) most = iter[q];
        const double e = fabs(xn[q] - delta[q]) / delta[q];
        if (iter[q] > 0 && e > worst) worst = e;    /* (a member whose Gauss-Newton step lies inside the radius keeps it) */
    }
    printf(" MMQR ran trust-region steps of %d %dx%d systems in %f s (avg over %d)   [batch resident in HBM, rtol 0.1, maxit 10]\n", count, m, n,
           el / TRIALS, TRIALS);
    printf(" failed = %d   worst | |x| - Delta | / Delta = %.2e   most iterations = %d\n", failed, worst, most);
    qr_device_free(dA); qr_device_free(dB); qr_device_free(dtau); qr_device_free(dX); qr_device_free(dv); qr_device_free(di);
    qr_plan_destroy(p);
    free(A); free(B); free(delta); free(xn); free(info); free(iter);
    return 0;
}

/* the model of --lm on host buffers: y = a exp(-b t) + c on m points of [0, 4] */
typedef struct lm_model {
    int m;
    const double* y;              /* count x m: the planted curves */
} lm_model;

static int lm_expdecay(void* user, int what, const double* X, int batch, double* F, double* J)
{
    const lm_model* M = (const lm_model*) user;
    const int m = M->m;
    for (int q = 0; q < batch; q++) {
        const double a = X[3 * (size_t) q], b = X[3 * (size_t) q + 1], c = X[3 * (size_t) q + 2];
        for (int i = 0; i < m; i++) {
            const double t = m > 1 ? 4.0 * i / (m - 1) : 0.0, e = exp(-b * t);
            if (what == 2) {
                double* Jq = J + (size_t) q * m * 3;
                Jq[i] = e; Jq[m + i] = -a * t * e; Jq[2 * m + i] = 1.0;
            } else {
                F[(size_t) q * m + i] = a * e + c - M->y[(size_t) q * m + i];
            }
        }
    }
    return 0;
}

/* count exponential-decay fits of m points (n = 3) through the host twin of the batched Levenberg-Marquardt solver; box: through the
 * bounded twin with 0 <= a, 0 <= b <= 0.8 planted b, 0 <= c, the start of b at half its bound */
static int batched_lm_main(int m, int n, int count, int box)
{
    if (n != 3 || m < 3 || m > qr_batched_max_rows(4) || count < 1) {
        fprintf(stderr, "--batched count --lm fits a exp(-b t) + c: needs n == 3, 3 <= m <= %d and count >= 1\n", qr_batched_max_rows(4));
        return 1;
    }
    printf("Exact problem size: %d exponential-decay fits of %d points, start = planted x (1 +- 0.2)\n", count, m);
    const size_t nc = (size_t) count;
    double *xs = malloc(sizeof(double) * 3 * nc), *X = malloc(sizeof(double) * 3 * nc), *y = malloc(sizeof(double) * nc * (size_t) m);
    double* fnorm = malloc(sizeof(double) * nc);
    int *nfev = malloc(sizeof(int) * nc), *njev = malloc(sizeof(int) * nc), *status = malloc(sizeof(int) * nc), *info = malloc(sizeof(int) * nc);
    if (!xs || !X || !y || !fnorm || !nfev || !njev || !status || !info) { fprintf(stderr, "out of memory\n"); return 1; }
    srand(12);
    for (size_t q = 0; q < nc; q++) {
        xs[3 * q] = 1.0 + (double) rand() / RAND_MAX;
        xs[3 * q + 1] = 0.5 + (double) rand() / RAND_MAX;
        xs[3 * q + 2] = 0.25 + 0.5 * rand() / RAND_MAX;
        for (int i = 0; i < m; i++) y[q * m + i] = xs[3 * q] * exp(-xs[3 * q + 1] * (m > 1 ? 4.0 * i / (m - 1) : 0.0)) + xs[3 * q + 2];
    }
    lm_model M = {m, y};
    double *lo = NULL, *hi = NULL;
    if (box) {
        lo = calloc(3 * nc, sizeof(double));
        hi = malloc(sizeof(double) * 3 * nc);
        if (!lo || !hi) { fprintf(stderr, "out of memory\n"); return 1; }
        for (size_t q = 0; q < nc; q++) { hi[3 * q] = hi[3 * q + 2] = INFINITY; hi[3 * q + 1] = 0.8 * xs[3 * q + 1]; }
    }
    double el = 0.0;
    for (int t = -1; t < TRIALS; t++) {
        srand(13);
        for (size_t i = 0; i < 3 * nc; i++) X[i] = xs[i] * (rand() & 1 ? 1.2 : 0.8);
        if (box)
            for (size_t q = 0; q < nc; q++) X[3 * q + 1] = 0.5 * hi[3 * q + 1];
        const double t0 = now();
        const int rc = box ? qr_lstsq_lm_bounded_batched(lm_expdecay, &M, m, 3, count, X, lo, hi, NULL, NULL, fnorm, nfev, njev, status, info)
                           : qr_lstsq_lm_batched(lm_expdecay, &M, m, 3, count, X, NULL, NULL, fnorm, nfev, njev, status, info);
        if (rc && rc != QR_E_SINGULAR) { fprintf(stderr, "%s failed: %s\n", box ? "qr_lstsq_lm_bounded_batched" : "qr_lstsq_lm_batched", qr_strerror(rc)); return 1; }
        if (t >= 0) el += now() - t0;
    }
    if (box) {                    /* the planted x is outside the box: what counts is the box and the bound the fits end on */
        size_t onb = 0, out = 0;
        for (size_t q = 0; q < nc; q++) {
            onb += X[3 * q + 1] == hi[3 * q + 1];
            for (int j = 0; j < 3; j++) out += !(X[3 * q + j] >= lo[3 * q + j] && X[3 * q + j] <= hi[3 * q + j]);
        }
        printf(" box: 0 <= a, 0 <= b <= 0.8 planted b, 0 <= c: %zu of %d fits end with b on its bound, %zu entries outside the box\n", onb, count, out);
        free(lo); free(hi);
    }
    int hist[10] = {0}, most = 0, failed = 0;
    double worst = 0.0, mean = 0.0;
    for (size_t q = 0; q < nc; q++) {
        if (info[q]) failed++;
        hist[status[q] >= 0 && status[q] <= 8 ? status[q] : 9]++;
        mean += nfev[q];
        if (nfev[q] > most) most = nfev[q];
        double e = 0.0;
        for (int j = 0; j < 3; j++) e += (X[3 * q + j] - xs[3 * q + j]) * (X[3 * q + j] - xs[3 * q + j]);
        if (sqrt(e) > worst) worst = sqrt(e);
    }
    printf(" MMQR ran %d Levenberg-Marquardt fits of %d points in %f s (avg over %d)   [host twin: the model runs on the host between the "
           "device calls]\n", count, m, el / TRIALS, TRIALS);
    printf(" worst |x - planted| = %.2e   nfev mean %.2f max %d   info != 0: %d\n status:", worst, mean / count, most, failed);
    for (int s = 0; s < 10; s++)
        if (hist[s]) printf(s < 9 ? "  %d: %d" : "  other: %d", s < 9 ? s : hist[s], hist[s]);
    printf("\n");
    free(xs); free(X); free(y); free(fnorm); free(nfev); free(njev); free(status); free(info);
    return 0;
}

/* count problems min |A x - b| subject to C x = d (A m x n, C p x n) through one qr_gglse_batched_dev call */
static int batched_lse_main(int m, int n, int count, int p)
{
    if (count < 1 || p < 1 || qr_gglse_batched_max_rows(n, p, 1) < 1 || m < 1 || m < n - p || m > qr_gglse_batched_max_rows(n, p, 1)) {
        fprintf(stderr, "--batched count --lse p needs count >= 1, 1 <= p <= n < %d, m + p >= n and 1 <= m <= qr_gglse_batched_max_rows(n, p, 1)\n",
                QR_BATCHED_MAX_N);
        return 1;
    }
    printf("Exact problem size: %d problems of %dx%d with %d constraints\n", count, m, n, p);
    const size_t nc = (size_t) count, mn = (size_t) m * n, pn = (size_t) p * n;
    const size_t tot = nc * (mn + pn + (size_t) m + (size_t) p), outs = nc * ((size_t) n + (size_t) p + 1);
    double *H = malloc(sizeof(double) * tot), *O = malloc(sizeof(double) * outs);
    int* info = malloc(sizeof(int) * nc);
    if (!H || !O || !info) { fprintf(stderr, "out of memory\n"); return 1; }
    srand(12);
    for (size_t i = 0; i < tot; i++) H[i] = (double) rand() / RAND_MAX - 0.5;
    const double *A = H, *C = A + nc * mn, *B = C + nc * pn, *D = B + nc * m;
    qr_plan* plan = NULL;
    double *dH = NULL, *dO = NULL;
    int* di = NULL;
    if (qr_plan_create(&plan, m > n ? m : n, n, 0, 0) || qr_device_malloc((void**) &dH, sizeof(double) * tot) ||
        qr_device_malloc((void**) &dO, sizeof(double) * outs) || qr_device_malloc((void**) &di, sizeof(int) * nc) ||
        qr_copy_to_device(dH, H, sizeof(double) * tot)) {
        fprintf(stderr, "device setup failed\n");
        return 1;
    }
    const double *dA = dH, *dC = dA + nc * mn, *dB = dC + nc * pn, *dD = dB + nc * m;
    double *dX = dO, *dL = dX + nc * n, *dres = dL + nc * p;
    double el = 0.0;
    for (int t = -1; t < TRIALS; t++) {               /* (the inputs are read only: no copy between the trials) */
        const double t0 = now();
        int rc = qr_gglse_batched_dev(plan, dA, m, n, m, (long long) mn, dC, p, p, (long long) pn, dB, m, m, dD, p, p, 1, dX, n, n, dL, p, p, dres, 1, di,
                                      count);
        if (!rc) rc = qr_plan_sync(plan);
        if (rc) { fprintf(stderr, "the batched call failed: %s\n", qr_strerror(rc)); return 1; }
        if (t >= 0) el += now() - t0;
    }
    if (qr_copy_to_host(O, dO, sizeof(double) * outs) || qr_copy_to_host(info, di, sizeof(int) * nc)) { fprintf(stderr, "copy back failed\n"); return 1; }
    const double *X = O, *L = X + nc * n;
    int failed = 0;
    double wc = 0.0, wk = 0.0;
    double* r = malloc(sizeof(double) * (size_t) m);
    if (!r) { fprintf(stderr, "out of memory\n"); return 1; }
    for (size_t q = 0; q < nc; q++) {
        if (info[q]) { failed++; continue; }
        const double *Aq = A + q * mn, *Cq = C + q * pn, *bq = B + q * m, *dq = D + q * p, *x = X + q * n, *l = L + q * p;
        double nA = 0.0, nC = 0.0, nx = 0.0, nb = 0.0, nd = 0.0, nl = 0.0, ec = 0.0, ek = 0.0;
        for (size_t i = 0; i < mn; i++) nA += Aq[i] * Aq[i];
        for (size_t i = 0; i < pn; i++) nC += Cq[i] * Cq[i];
        for (int i = 0; i < n; i++) nx += x[i] * x[i];
        for (int i = 0; i < m; i++) nb += bq[i] * bq[i];
        for (int i = 0; i < p; i++) { nd += dq[i] * dq[i]; nl += l[i] * l[i]; }
        for (int i = 0; i < p; i++) {
            double s = -dq[i];
            for (int c = 0; c < n; c++) s += Cq[(size_t) c * p + i] * x[c];
            ec += s * s;
        }
        for (int i = 0; i < m; i++) {
            double s = -bq[i];
            for (int c = 0; c < n; c++) s += Aq[(size_t) c * m + i] * x[c];
            r[i] = s;
        }
        for (int c = 0; c < n; c++) {
            double s = 0.0;
            for (int i = 0; i < m; i++) s += Aq[(size_t) c * m + i] * r[i];
            for (int i = 0; i < p; i++) s += Cq[(size_t) c * p + i] * l[i];
            ek += s * s;
        }
        nA = sqrt(nA); nC = sqrt(nC);
        const double c1 = sqrt(ec) / (nC * sqrt(nx) + sqrt(nd)), k1 = sqrt(ek) / (nA * (nA * sqrt(nx) + sqrt(nb)) + nC * sqrt(nl));
        if (c1 > wc) wc = c1;
        if (k1 > wk) wk = k1;
    }
    printf(" MMQR solved %d constrained %dx%d systems (p = %d) in %f s (avg over %d)   [batch resident in HBM]\n", count, m, n, p, el / TRIALS, TRIALS);
    printf(" worst ||C x - d|| / (||C|| ||x|| + ||d||) = %.2e   worst KKT residual = %.2e   non-zero info words = %d\n", wc, wk, failed);
    qr_device_free(dH); qr_device_free(dO); qr_device_free(di);
    qr_plan_destroy(plan);
    free(H); free(O); free(info); free(r);
    return 0;
}

/* count planted problems min |A x - b| subject to lo <= x <= hi through one qr_bvls_batched_dev call */
static int batched_bvls_main(int m, int n, int count)
{
    if (count < 1 || qr_bvls_batched_max_rows(n) < 1 || m < n || m > qr_bvls_batched_max_rows(n)) {
        fprintf(stderr, "--batched count --bvls needs count >= 1, 1 <= n < %d and n <= m <= qr_bvls_batched_max_rows(n)\n", QR_BATCHED_MAX_N);
        return 1;
    }
    printf("Exact problem size: %d planted bound-constrained problems of %dx%d\n", count, m, n);
    const size_t nc = (size_t) count, mn = (size_t) m * n;
    const size_t tot = nc * (mn + (size_t) m + 2 * (size_t) n), outs = nc * (2 * (size_t) n + 1);
    double *H = malloc(sizeof(double) * tot), *O = malloc(sizeof(double) * outs), *Qf = malloc(sizeof(double) * mn), *r = malloc(sizeof(double) * (size_t) m);
    int *planted = malloc(sizeof(int) * nc * n), *IO = malloc(sizeof(int) * nc * ((size_t) n + 2));
    if (!H || !O || !Qf || !r || !planted || !IO) { fprintf(stderr, "out of memory\n"); return 1; }
    srand(12);
    double *A = H, *B = A + nc * mn, *LO = B + nc * m, *HI = LO + nc * n;
    for (size_t q = 0; q < nc; q++) {
        double *Aq = A + q * mn, *bq = B + q * m, *lo = LO + q * n, *hi = HI + q * n;
        int* pl = planted + q * n;
        for (size_t i = 0; i < mn; i++) Aq[i] = (double) rand() / RAND_MAX - 0.5;
        for (int i = 0; i < m; i++) r[i] = (double) rand() / RAND_MAX - 0.5;
        int nf = 0;
        for (int j = 0; j < n; j++) {
            lo[j] = -0.5 - (double) rand() / RAND_MAX;
            hi[j] = 0.5 + (double) rand() / RAND_MAX;
            pl[j] = rand() & 1;                       /* 1: active; the side is decided by the sign of a_j^T r below */
            if (pl[j]) continue;
            /* a free column: orthonormalised against the earlier free ones (twice), then r made orthogonal to it */
            double* qc = Qf + (size_t) nf * m;
            memcpy(qc, Aq + (size_t) j * m, sizeof(double) * (size_t) m);
            for (int pass = 0; pass < 2; pass++)
                for (int k = 0; k < nf; k++) {
                    double d = 0.0;
                    for (int i = 0; i < m; i++) d += Qf[(size_t) k * m + i] * qc[i];
                    for (int i = 0; i < m; i++) qc[i] -= d * Qf[(size_t) k * m + i];
                }
            double nq = 0.0;
            for (int i = 0; i < m; i++) nq += qc[i] * qc[i];
            nq = sqrt(nq);
            for (int i = 0; i < m; i++) qc[i] /= nq;
            nf++;
        }
        for (int pass = 0; pass < 2; pass++)
            for (int k = 0; k < nf; k++) {
                double d = 0.0;
                for (int i = 0; i < m; i++) d += Qf[(size_t) k * m + i] * r[i];
                for (int i = 0; i < m; i++) r[i] -= d * Qf[(size_t) k * m + i];
            }
        memcpy(bq, r, sizeof(double) * (size_t) m);
        for (int j = 0; j < n; j++) {
            double xs = 0.8 * ((double) rand() / RAND_MAX - 0.5);
            if (pl[j]) {
                double g = 0.0;
                for (int i = 0; i < m; i++) g += Aq[(size_t) j * m + i] * r[i];
                pl[j] = g < 0.0 ? -1 : 1;
                xs = g < 0.0 ? lo[j] : hi[j];
            }
            for (int i = 0; i < m; i++) bq[i] += Aq[(size_t) j * m + i] * xs;
        }
    }
    qr_plan* plan = NULL;
    double *dH = NULL, *dO = NULL;
    int* dI = NULL;
    if (qr_plan_create(&plan, m, n, 0, 0) || qr_device_malloc((void**) &dH, sizeof(double) * tot) ||
        qr_device_malloc((void**) &dO, sizeof(double) * outs) || qr_device_malloc((void**) &dI, sizeof(int) * nc * ((size_t) n + 2)) ||
        qr_copy_to_device(dH, H, sizeof(double) * tot)) {
        fprintf(stderr, "device setup failed\n");
        return 1;
    }
    const double *dA = dH, *dB = dA + nc * mn, *dlo = dB + nc * m, *dhi = dlo + nc * n;
    double *dX = dO, *dW = dX + nc * n, *dres = dW + nc * n;
    int *dstate = dI, *diter = dstate + nc * n, *dinfo = diter + nc;
    double el = 0.0;
    for (int t = -1; t < TRIALS; t++) {               /* (the inputs are read only: no copy between the trials) */
        const double t0 = now();
        int rc = qr_bvls_batched_dev(plan, dA, m, n, m, (long long) mn, dB, m, dlo, dhi, n, 0, dX, n, dW, n, dstate, n, dres, diter, dinfo, count);
        if (!rc) rc = qr_plan_sync(plan);
        if (rc) { fprintf(stderr, "the batched call failed: %s\n", qr_strerror(rc)); return 1; }
        if (t >= 0) el += now() - t0;
    }
    if (qr_copy_to_host(O, dO, sizeof(double) * outs) || qr_copy_to_host(IO, dI, sizeof(int) * nc * ((size_t) n + 2))) { fprintf(stderr, "copy back failed\n"); return 1; }
    const double* X = O;
    const int *state = IO, *iter = state + nc * n, *info = iter + nc;
    int failed = 0, mismatched = 0, most = 0;
    double worst = 0.0, iters = 0.0;
    for (size_t q = 0; q < nc; q++) {
        if (info[q]) { failed++; continue; }
        const double *Aq = A + q * mn, *bq = B + q * m, *x = X + q * n;
        double nA = 0.0, nx = 0.0, nb = 0.0;
        for (size_t i = 0; i < mn; i++) nA += Aq[i] * Aq[i];
        for (int i = 0; i < n; i++) nx += x[i] * x[i];
        for (int i = 0; i < m; i++) nb += bq[i] * bq[i];
        for (int i = 0; i < m; i++) {
            double s = bq[i];
            for (int c = 0; c < n; c++) s -= Aq[(size_t) c * m + i] * x[c];
            r[i] = s;
        }
        const double nrm = sqrt(nA) * sqrt(nx) + sqrt(nb);
        for (int c = 0; c < n; c++) {
            if (state[q * n + c] != planted[q * n + c]) mismatched++;
            if (state[q * n + c] != 0) continue;
            double g = 0.0, na = 0.0;
            for (int i = 0; i < m; i++) { g += Aq[(size_t) c * m + i] * r[i]; na += Aq[(size_t) c * m + i] * Aq[(size_t) c * m + i]; }
            const double s1 = fabs(g) / (sqrt(na) * nrm);
            if (s1 > worst) worst = s1;
        }
        iters += iter[q];
        if (iter[q] > most) most = iter[q];
    }
    printf(" MMQR solved %d bound-constrained %dx%d systems in %f s (avg over %d)   [batch resident in HBM]\n", count, m, n, el / TRIALS, TRIALS);
    printf(" worst free stationarity = %.2e   state mismatches = %d   non-zero info words = %d   eliminations: mean %.2f, most %d\n", worst, mismatched,
           failed, failed < count ? iters / (count - failed) : 0.0, most);
    qr_device_free(dH); qr_device_free(dO); qr_device_free(dI);
    qr_plan_destroy(plan);
    free(H); free(O); free(Qf); free(r); free(planted); free(IO);
    return 0;
}

/* count planted problems min |A x - b| subject to G(0:neq) x = h(0:neq), G(neq:mg) x >= h(neq:mg) through one qr_lsei_batched_dev call */
static int batched_lsei_main(int m, int n, int count, int mg, int neq)
{
    if (count < 1 || qr_lsei_batched_max_rows(n, mg) < 1 || neq < 0 || neq > n || neq > mg || m < n || m > qr_lsei_batched_max_rows(n, mg)) {
        fprintf(stderr, "--batched count --lsei mg [neq] needs count >= 1, 1 <= n < %d, 1 <= mg <= 64, 0 <= neq <= min(n, mg) and "
                        "n <= m <= qr_lsei_batched_max_rows(n, mg)\n", QR_BATCHED_MAX_N);
        return 1;
    }
    int na = (n < mg - neq ? n : mg - neq) / 2;
    if (na > n - neq) na = n - neq;
    printf("Exact problem size: %d planted problems of %dx%d with %d constraint rows (%d equalities, %d inequalities active)\n", count, m, n, mg, neq, na);
    const size_t nc = (size_t) count, mn = (size_t) m * n, gn = (size_t) mg * n;
    const size_t tot = nc * (mn + (size_t) m + gn + (size_t) mg), outs = nc * ((size_t) n + 2 * (size_t) mg + 1);
    double *Hh = malloc(sizeof(double) * tot), *O = malloc(sizeof(double) * outs), *N = malloc(sizeof(double) * (size_t) n * n);
    double *w = malloc(sizeof(double) * (size_t) (n + m + mg)), *r = malloc(sizeof(double) * (size_t) m);
    int *planted = malloc(sizeof(int) * nc * mg), *IO = malloc(sizeof(int) * nc * ((size_t) mg + 2));
    if (!Hh || !O || !N || !w || !r || !planted || !IO) { fprintf(stderr, "out of memory\n"); return 1; }
    srand(12);
    double *A = Hh, *B = A + nc * mn, *G = B + nc * m, *HH = G + nc * gn;
    for (size_t q = 0; q < nc; q++) {
        double *Aq = A + q * mn, *bq = B + q * m, *Gq = G + q * gn, *hq = HH + q * mg;
        double *z = w, *xs = w + n, *mus = w + n + m;           /* (xs: n <= m entries) */
        int* pl = planted + q * mg;
        for (size_t i = 0; i < mn; i++) Aq[i] = (double) rand() / RAND_MAX - 0.5;
        for (size_t i = 0; i < gn; i++) Gq[i] = (double) rand() / RAND_MAX - 0.5;
        for (int j = 0; j < n; j++) xs[j] = 2.0 * ((double) rand() / RAND_MAX - 0.5);
        for (int i = 0; i < mg; i++) { pl[i] = i < neq; mus[i] = 0.0; }
        for (int c = 0; c < na; ) {                            /* na distinct inequality rows */
            const int i = neq + rand() % (mg - neq);
            if (!pl[i]) { pl[i] = 1; c++; }
        }
        for (int i = 0; i < mg; i++) {
            const double u = 0.5 + (double) rand() / RAND_MAX;
            if (pl[i]) mus[i] = (i < neq && (rand() & 1)) ? -u : u;
            double s = 0.0;
            for (int j = 0; j < n; j++) s += Gq[(size_t) j * mg + i] * xs[j];
            hq[i] = pl[i] ? s : s - u;
        }
        /* (A^T A) z = G^T mu* by Cholesky; b = A (x* - z): A^T (A x* - b) = G^T mu* */
        for (int a = 0; a < n; a++)
            for (int c = a; c < n; c++) {
                double s = 0.0;
                for (int i = 0; i < m; i++) s += Aq[(size_t) a * m + i] * Aq[(size_t) c * m + i];
                N[(size_t) c * n + a] = N[(size_t) a * n + c] = s;
            }
        for (int j = 0; j < n; j++) {
            double s = 0.0;
            for (int i = 0; i < mg; i++) s += Gq[(size_t) j * mg + i] * mus[i];
            z[j] = s;
        }
        for (int j = 0; j < n; j++) {                          /* N = L L^T, L in the lower triangle (N[c * n + r], r >= c) */
            double d = N[(size_t) j * n + j];
            for (int k = 0; k < j; k++) d -= N[(size_t) k * n + j] * N[(size_t) k * n + j];
            d = sqrt(d);
            N[(size_t) j * n + j] = d;
            for (int i = j + 1; i < n; i++) {
                double s = N[(size_t) j * n + i];
                for (int k = 0; k < j; k++) s -= N[(size_t) k * n + i] * N[(size_t) k * n + j];
                N[(size_t) j * n + i] = s / d;
            }
        }
        for (int i = 0; i < n; i++) {
            double s = z[i];
            for (int k = 0; k < i; k++) s -= N[(size_t) k * n + i] * z[k];
            z[i] = s / N[(size_t) i * n + i];
        }
        for (int i = n - 1; i >= 0; i--) {
            double s = z[i];
            for (int k = i + 1; k < n; k++) s -= N[(size_t) i * n + k] * z[k];
            z[i] = s / N[(size_t) i * n + i];
        }
        for (int i = 0; i < m; i++) {
            double s = 0.0;
            for (int j = 0; j < n; j++) s += Aq[(size_t) j * m + i] * (xs[j] - z[j]);
            bq[i] = s;
        }
    }
    qr_plan* plan = NULL;
    double *dH = NULL, *dO = NULL;
    int* dI = NULL;
    if (qr_plan_create(&plan, m, n, 0, 0) || qr_device_malloc((void**) &dH, sizeof(double) * tot) ||
        qr_device_malloc((void**) &dO, sizeof(double) * outs) || qr_device_malloc((void**) &dI, sizeof(int) * nc * ((size_t) mg + 2)) ||
        qr_copy_to_device(dH, Hh, sizeof(double) * tot)) {
        fprintf(stderr, "device setup failed\n");
        return 1;
    }
    const double *dA = dH, *dB = dA + nc * mn, *dG = dB + nc * m, *dHH = dG + nc * gn;
    double *dX = dO, *dMU = dX + nc * n, *dS = dMU + nc * mg, *dres = dS + nc * mg;
    int *dstate = dI, *diter = dstate + nc * mg, *dinfo = diter + nc;
    double el = 0.0;
    for (int t = -1; t < TRIALS; t++) {               /* (the inputs are read only: no copy between the trials) */
        const double t0 = now();
        int rc = qr_lsei_batched_dev(plan, dA, m, n, m, (long long) mn, dB, m, dG, mg, neq, mg, (long long) gn, dHH, mg, 0, 0.0, dX, n, dMU, mg, dS,
                                     mg, dstate, mg, dres, diter, dinfo, count);
        if (!rc) rc = qr_plan_sync(plan);
        if (rc) { fprintf(stderr, "the batched call failed: %s\n", qr_strerror(rc)); return 1; }
        if (t >= 0) el += now() - t0;
    }
    if (qr_copy_to_host(O, dO, sizeof(double) * outs) || qr_copy_to_host(IO, dI, sizeof(int) * nc * ((size_t) mg + 2))) { fprintf(stderr, "copy back failed\n"); return 1; }
    const double *X = O, *MU = X + nc * n;
    const int *state = IO, *iter = state + nc * mg, *info = iter + nc;
    int failed = 0, mismatched = 0, most = 0;
    double worstc = 0.0, worstk = 0.0, iters = 0.0;
    for (size_t q = 0; q < nc; q++) {
        if (info[q]) { failed++; continue; }
        const double *Aq = A + q * mn, *bq = B + q * m, *Gq = G + q * gn, *hq = HH + q * mg, *x = X + q * n, *mu = MU + q * mg;
        double nA = 0.0, nx = 0.0, nb = 0.0;
        for (size_t i = 0; i < mn; i++) nA += Aq[i] * Aq[i];
        for (int i = 0; i < n; i++) nx += x[i] * x[i];
        for (int i = 0; i < m; i++) nb += bq[i] * bq[i];
        for (int i = 0; i < m; i++) {
            double s = -bq[i];
            for (int c = 0; c < n; c++) s += Aq[(size_t) c * m + i] * x[c];
            r[i] = s;
        }
        const double nrm = sqrt(nA) * sqrt(nx) + sqrt(nb);
        for (int i = 0; i < mg; i++) {
            if (state[q * mg + i] != planted[q * mg + i]) mismatched++;
            double s = -hq[i], sc = fabs(hq[i]);
            for (int c = 0; c < n; c++) { s += Gq[(size_t) c * mg + i] * x[c]; sc += fabs(Gq[(size_t) c * mg + i] * x[c]); }
            const double v = state[q * mg + i] ? fabs(s) : (s < 0.0 ? -s : 0.0);
            if (sc > 0.0 && v / sc > worstc) worstc = v / sc;
        }
        for (int c = 0; c < n; c++) {
            double g = 0.0, na2 = 0.0, gm = 0.0;
            for (int i = 0; i < m; i++) { g += Aq[(size_t) c * m + i] * r[i]; na2 += Aq[(size_t) c * m + i] * Aq[(size_t) c * m + i]; }
            for (int i = 0; i < mg; i++) { g -= Gq[(size_t) c * mg + i] * mu[i]; gm += fabs(Gq[(size_t) c * mg + i] * mu[i]); }
            const double k1 = fabs(g) / (sqrt(na2) * nrm + gm);
            if (k1 > worstk) worstk = k1;
        }
        iters += iter[q];
        if (iter[q] > most) most = iter[q];
    }
    printf(" MMQR solved %d inequality-constrained %dx%d systems with %d rows of G in %f s (avg over %d)   [batch resident in HBM]\n", count, m, n, mg,
           el / TRIALS, TRIALS);
    printf(" worst constraint violation = %.2e   worst KKT residual = %.2e   state mismatches = %d   candidates: mean %.2f, most %d   non-zero info words = %d\n",
           worstc, worstk, mismatched, failed < count ? iters / (count - failed) : 0.0, most, failed);
    qr_device_free(dH); qr_device_free(dO); qr_device_free(dI);
    qr_plan_destroy(plan);
    free(Hh); free(O); free(N); free(w); free(r); free(planted); free(IO);
    return 0;
}

/* count planted problems with a fraction frac of outlier rows through one qr_irls_batched_dev call (Huber), beside qr_gels_batched_dev */
static int batched_robust_main(int m, int n, int count, double frac)
{
    if (count < 1 || qr_irls_batched_max_rows(n) < 1 || m < n || m > qr_irls_batched_max_rows(n) || !(frac >= 0.0 && frac < 0.5)) {
        fprintf(stderr, "--batched count --robust frac needs count >= 1, 1 <= n < %d, n <= m <= qr_irls_batched_max_rows(n) and 0 <= frac < 0.5\n",
                QR_BATCHED_MAX_N);
        return 1;
    }
    const int nout = (int) (frac * m);
    printf("Exact problem size: %d planted %dx%d problems with %d outlier rows each\n", count, m, n, nout);
    const size_t nc = (size_t) count, mn = (size_t) m * n;
    const size_t tot = nc * (mn + (size_t) m), outs = nc * (size_t) n;
    double *H = malloc(sizeof(double) * tot), *XS = malloc(sizeof(double) * outs), *X = malloc(sizeof(double) * outs), *XG = malloc(sizeof(double) * nc * m);
    int* IO = malloc(sizeof(int) * nc * 3);
    if (!H || !XS || !X || !XG || !IO) { fprintf(stderr, "out of memory\n"); return 1; }
    srand(12);
    double *A = H, *B = A + nc * mn;
    for (size_t q = 0; q < nc; q++) {
        double *Aq = A + q * mn, *bq = B + q * m, *xs = XS + q * n;
        for (size_t i = 0; i < mn; i++) Aq[i] = (double) rand() / RAND_MAX - 0.5;
        for (int j = 0; j < n; j++) xs[j] = 2.0 * ((double) rand() / RAND_MAX - 0.5);
        for (int i = 0; i < m; i++) {
            /* noise: the sum of twelve uniforms, variance 1, times 0.01 */
            double g = -6.0;
            for (int k = 0; k < 12; k++) g += (double) rand() / RAND_MAX;
            double s = 0.01 * g;
            for (int j = 0; j < n; j++) s += Aq[(size_t) j * m + i] * xs[j];
            bq[i] = s;
        }
        for (int k = 0; k < nout; k++) {              /* every (m / nout)-th row, from a random offset */
            const int i = (int) (((size_t) k * m) / nout + (size_t) (rand() % (m / nout))) % m;
            const double sh = 0.1 + 0.4 * (double) rand() / RAND_MAX;
            bq[i] += (rand() & 1) ? sh : -sh;
        }
    }
    qr_plan* plan = NULL;
    double *dH = NULL, *dG = NULL, *dX = NULL, *dtau = NULL;
    int* dI = NULL;
    if (qr_plan_create(&plan, m, n, 0, 0) || qr_device_malloc((void**) &dH, sizeof(double) * tot) || qr_device_malloc((void**) &dG, sizeof(double) * tot) ||
        qr_device_malloc((void**) &dX, sizeof(double) * outs) || qr_device_malloc((void**) &dtau, sizeof(double) * outs) ||
        qr_device_malloc((void**) &dI, sizeof(int) * nc * 3) || qr_copy_to_device(dH, H, sizeof(double) * tot) ||
        qr_copy_to_device(dG, H, sizeof(double) * tot)) {
        fprintf(stderr, "device setup failed\n");
        return 1;
    }
    const double *dA = dH, *dB = dA + nc * mn;
    int *diter = dI, *dstatus = diter + nc, *dinfo = dstatus + nc;
    double el = 0.0;
    for (int t = -1; t < TRIALS; t++) {               /* (the inputs are read only: no copy between the trials) */
        const double t0 = now();
        int rc = qr_irls_batched_dev(plan, QR_LOSS_HUBER, 0.0, dA, m, n, m, (long long) mn, dB, m, NULL, 0, NULL, NULL, 0, 1e-8, 0, dX, n, NULL, 0,
                                     NULL, NULL, diter, dstatus, dinfo, count);
        if (!rc) rc = qr_plan_sync(plan);
        if (rc) { fprintf(stderr, "the batched call failed: %s\n", qr_strerror(rc)); return 1; }
        if (t >= 0) el += now() - t0;
    }
    if (qr_copy_to_host(X, dX, sizeof(double) * outs) || qr_copy_to_host(IO, dI, sizeof(int) * nc * 3)) { fprintf(stderr, "copy back failed\n"); return 1; }
    /* the squared loss on copies of the same members (qr_gels_batched_dev factors in place) */
    {
        int rc = qr_gels_batched_dev(plan, dG, m, n, m, (long long) mn, dtau, n, dG + nc * mn, 1, m, m, dinfo, count);
        if (!rc) rc = qr_plan_sync(plan);
        if (rc || qr_copy_to_host(XG, dG + nc * mn, sizeof(double) * nc * m)) { fprintf(stderr, "the least-squares call failed\n"); return 1; }
    }
    const int *iter = IO, *info = IO + 2 * nc;
    int failed = 0, most = 0;
    double worst = 0.0, worst_ls = 0.0, iters = 0.0;
    for (size_t q = 0; q < nc; q++) {
        if (info[q]) { failed++; continue; }
        const double *xs = XS + q * n, *x = X + q * n, *xg = XG + q * m;
        double d = 0.0, dg = 0.0, nx = 0.0;
        for (int j = 0; j < n; j++) { d += (x[j] - xs[j]) * (x[j] - xs[j]); dg += (xg[j] - xs[j]) * (xg[j] - xs[j]); nx += xs[j] * xs[j]; }
        if (sqrt(d / nx) > worst) worst = sqrt(d / nx);
        if (sqrt(dg / nx) > worst_ls) worst_ls = sqrt(dg / nx);
        iters += iter[q];
        if (iter[q] > most) most = iter[q];
    }
    printf(" MMQR solved %d robust (Huber) %dx%d systems in %f s (avg over %d)   [batch resident in HBM]\n", count, m, n, el / TRIALS, TRIALS);
    printf(" worst ||x - x*|| / ||x*|| = %.2e (qr_gels_batched_dev: %.2e)   solves: mean %.2f, most %d   non-zero info words = %d\n", worst, worst_ls,
           failed < count ? iters / (count - failed) : 0.0, most, failed);
    qr_device_free(dH); qr_device_free(dG); qr_device_free(dX); qr_device_free(dtau); qr_device_free(dI);
    qr_plan_destroy(plan);
    free(H); free(XS); free(X); free(XG); free(IO);
    return 0;
}

/* count seeded members through one qr_gels_stats_batched_dev call with every output */
static int batched_stats_main(int m, int n, int count)
{
    if (count < 1 || qr_stats_batched_max_rows(n) < 1 || m < n || m > qr_stats_batched_max_rows(n)) {
        fprintf(stderr, "--batched count --stats needs count >= 1, 1 <= n < %d and n <= m <= qr_stats_batched_max_rows(n)\n", QR_BATCHED_MAX_N);
        return 1;
    }
    printf("Exact problem size: %d seeded %dx%d fits with residuals, leverages, covariance and standard errors\n", count, m, n);
    const size_t nc = (size_t) count, mn = (size_t) m * n, nn = (size_t) n * n;
    const size_t ins = nc * (mn + (size_t) m), outs = nc * ((size_t) n + 2 * (size_t) m + 1 + nn + (size_t) n);
    double *H = malloc(sizeof(double) * ins), *O = malloc(sizeof(double) * outs);
    int* IO = malloc(sizeof(int) * nc * 2);
    if (!H || !O || !IO) { fprintf(stderr, "out of memory\n"); return 1; }
    srand(12);
    double *A = H, *B = A + nc * mn;
    for (size_t q = 0; q < nc; q++) {
        double *Aq = A + q * mn, *bq = B + q * m;
        for (size_t i = 0; i < mn; i++) Aq[i] = (double) rand() / RAND_MAX - 0.5;
        for (int i = 0; i < m; i++) bq[i] = 0.01 * ((double) rand() / RAND_MAX - 0.5);
        for (int j = 0; j < n; j++) {
            const double xs = 2.0 * ((double) rand() / RAND_MAX - 0.5);
            for (int i = 0; i < m; i++) bq[i] += Aq[(size_t) j * m + i] * xs;
        }
    }
    qr_plan* plan = NULL;
    double *dH = NULL, *dO = NULL;
    int* dI = NULL;
    if (qr_plan_create(&plan, m, n, 0, 0) || qr_device_malloc((void**) &dH, sizeof(double) * ins) || qr_device_malloc((void**) &dO, sizeof(double) * outs) ||
        qr_device_malloc((void**) &dI, sizeof(int) * nc * 2) || qr_copy_to_device(dH, H, sizeof(double) * ins)) {
        fprintf(stderr, "device setup failed\n");
        return 1;
    }
    const double *dA = dH, *dB = dA + nc * mn;
    double *dX = dO, *dE = dX + nc * n, *dLev = dE + nc * m, *dsig = dLev + nc * m, *dC = dsig + nc, *dse = dC + nc * nn;
    int *ddof = dI, *dinfo = dI + nc;
    double el = 0.0;
    for (int t = -1; t < TRIALS; t++) {               /* (the inputs are read only: no copy between the trials) */
        const double t0 = now();
        int rc = qr_gels_stats_batched_dev(plan, QR_COV_UNSCALED, dA, m, n, m, (long long) mn, dB, m, NULL, 0, dX, n, dE, m, dLev, m, dsig, ddof, dC,
                                           n, (long long) nn, dse, n, dinfo, count);
        if (!rc) rc = qr_plan_sync(plan);
        if (rc) { fprintf(stderr, "the batched call failed: %s\n", qr_strerror(rc)); return 1; }
        if (t >= 0) el += now() - t0;
    }
    if (qr_copy_to_host(O, dO, sizeof(double) * outs) || qr_copy_to_host(IO, dI, sizeof(int) * nc * 2)) { fprintf(stderr, "copy back failed\n"); return 1; }
    const double *Lev = O + nc * n + nc * m, *Cv = Lev + nc * m + nc;
    const int* info = IO + nc;
    int failed = 0;
    double worst_h = 0.0, worst_c = 0.0;
    double* G = malloc(sizeof(double) * nn);
    if (!G) { fprintf(stderr, "out of memory\n"); return 1; }
    for (size_t q = 0; q < nc; q++) {
        if (info[q]) { failed++; continue; }
        const double *Aq = A + q * mn, *Cq = Cv + q * nn, *hq = Lev + q * m;
        double sh = 0.0;
        for (int i = 0; i < m; i++) sh += hq[i];
        if (fabs(sh - n) > worst_h) worst_h = fabs(sh - n);
        for (int a = 0; a < n; a++)
            for (int c = 0; c < n; c++) {
                double s = 0.0;
                for (int i = 0; i < m; i++) s += Aq[(size_t) a * m + i] * Aq[(size_t) c * m + i];
                G[(size_t) c * n + a] = s;
            }
        double f = 0.0;
        for (int a = 0; a < n; a++)
            for (int c = 0; c < n; c++) {
                double s = a == c ? -1.0 : 0.0;
                for (int k = 0; k < n; k++) s += Cq[(size_t) k * n + a] * G[(size_t) c * n + k];
                f += s * s;
            }
        if (sqrt(f) > worst_c) worst_c = sqrt(f);
    }
    printf(" MMQR fitted %d %dx%d systems with statistics in %f s (avg over %d)   [batch resident in HBM]\n", count, m, n, el / TRIALS, TRIALS);
    printf(" worst |sum h - n| = %.2e   worst ||C A^T A - I|| = %.2e   non-zero info words = %d\n", worst_h, worst_c, failed);
    qr_device_free(dH); qr_device_free(dO); qr_device_free(dI);
    qr_plan_destroy(plan);
    free(G); free(H); free(O); free(IO);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 3) { puts("Usage: ./qr_device m n [--compare] [--pivot] | ./qr_device m n --minnorm   (m <= n) | ./qr_device m n --append [chunk_rows] | ./qr_device m n --svd | ./qr_device m n --slide window step | ./qr_device m n --batched count [--pivot [rank] | --svd | --slide window step | --minnorm | --damped nlam | --trust frac | --lse p | --bvls | --lsei mg [neq] | --robust frac | --stats | --lm [--box]]"); return 1; }
    int compare = 0, pivot = 0, minnorm = 0;
    for (int i = 3; i < argc; i++)
        if (strcmp(argv[i], "--append") == 0) return append_main(atoi(argv[1]), atoi(argv[2]), i + 1 < argc ? atoi(argv[i + 1]) : 4096);
    for (int i = 3; i < argc; i++)
        if (strcmp(argv[i], "--slide") == 0) {
            if (i + 2 >= argc) { fprintf(stderr, "--slide needs window and step\n"); return 1; }
            for (int k = 3; k + 1 < argc; k++)          /* with --batched count: the batched accumulator */
                if (strcmp(argv[k], "--batched") == 0)
                    return batched_slide_main(atoi(argv[1]), atoi(argv[2]), atoi(argv[k + 1]), atoi(argv[i + 1]), atoi(argv[i + 2]));
            return slide_main(atoi(argv[1]), atoi(argv[2]), atoi(argv[i + 1]), atoi(argv[i + 2]));
        }
    for (int i = 3; i < argc; i++)
        if (strcmp(argv[i], "--batched") == 0) {
            if (i + 1 >= argc) { fprintf(stderr, "--batched needs a count\n"); return 1; }
            for (int k = 3; k < argc; k++)
                if (strcmp(argv[k], "--pivot") == 0)
                    return batched_pivot_main(atoi(argv[1]), atoi(argv[2]), atoi(argv[i + 1]),
                                              k + 1 < argc && argv[k + 1][0] != '-' ? atoi(argv[k + 1]) : atoi(argv[2]));
            for (int k = 3; k < argc; k++)
                if (strcmp(argv[k], "--svd") == 0) return batched_svd_main(atoi(argv[1]), atoi(argv[2]), atoi(argv[i + 1]));
            for (int k = 3; k < argc; k++)
                if (strcmp(argv[k], "--minnorm") == 0) return batched_minnorm_main(atoi(argv[1]), atoi(argv[2]), atoi(argv[i + 1]));
            for (int k = 3; k < argc; k++)
                if (strcmp(argv[k], "--damped") == 0)
                    return batched_damped_main(atoi(argv[1]), atoi(argv[2]), atoi(argv[i + 1]), k + 1 < argc ? atoi(argv[k + 1]) : 1);
            for (int k = 3; k < argc; k++)
                if (strcmp(argv[k], "--trust") == 0)
                    return batched_trust_main(atoi(argv[1]), atoi(argv[2]), atoi(argv[i + 1]), k + 1 < argc ? atof(argv[k + 1]) : 0.5);
            for (int k = 3; k < argc; k++)
                if (strcmp(argv[k], "--robust") == 0)
                    return batched_robust_main(atoi(argv[1]), atoi(argv[2]), atoi(argv[i + 1]), k + 1 < argc ? atof(argv[k + 1]) : 0.2);
            for (int k = 3; k < argc; k++)
                if (strcmp(argv[k], "--stats") == 0) return batched_stats_main(atoi(argv[1]), atoi(argv[2]), atoi(argv[i + 1]));
            for (int k = 3; k < argc; k++)
                if (strcmp(argv[k], "--lsei") == 0)
                    return batched_lsei_main(atoi(argv[1]), atoi(argv[2]), atoi(argv[i + 1]), k + 1 < argc ? atoi(argv[k + 1]) : 1,
                                             k + 2 < argc ? atoi(argv[k + 2]) : 0);
            for (int k = 3; k < argc; k++)
                if (strcmp(argv[k], "--lm") == 0) {
                    int box = 0;
                    for (int b = 3; b < argc; b++) box |= strcmp(argv[b], "--box") == 0;
                    return batched_lm_main(atoi(argv[1]), atoi(argv[2]), atoi(argv[i + 1]), box);
                }
            for (int k = 3; k < argc; k++)
                if (strcmp(argv[k], "--bvls") == 0) return batched_bvls_main(atoi(argv[1]), atoi(argv[2]), atoi(argv[i + 1]));
            for (int k = 3; k < argc; k++)
                if (strcmp(argv[k], "--lse") == 0)
                    return batched_lse_main(atoi(argv[1]), atoi(argv[2]), atoi(argv[i + 1]), k + 1 < argc ? atoi(argv[k + 1]) : 1);
            return batched_main(atoi(argv[1]), atoi(argv[2]), atoi(argv[i + 1]));
        }
    for (int i = 3; i < argc; i++)
        if (strcmp(argv[i], "--svd") == 0) return svd_main(atoi(argv[1]), atoi(argv[2]));
    for (int i = 3; i < argc; i++) {
        if (strcmp(argv[i], "--compare") == 0) compare = 1;
        if (strcmp(argv[i], "--pivot") == 0) pivot = 1;
        if (strcmp(argv[i], "--minnorm") == 0) minnorm = 1;
    }
    const int m = atoi(argv[1]), n = atoi(argv[2]);
    if (minnorm) return minnorm_main(m, n);
    if (m < 1 || n < 1 || m < n) { fprintf(stderr, "need m >= n >= 1\n"); return 1; }
    printf("Exact problem size: %dx%d\n", m, n);
    char arch[64]; int cus = 0, khz = 0; size_t hbm = 0;
    if (qr_device_info(arch, sizeof arch, &cus, &khz, &hbm)) { fprintf(stderr, "no HIP device\n"); return 1; }
    printf("Testing mmqr on \"%s\" (%d CUs, %.1f GiB HBM)\n", arch, cus, hbm / 1073741824.0);

    const size_t cnt = (size_t) m * n;
    double* A = malloc(sizeof(double) * cnt);
    double* RV = malloc(sizeof(double) * cnt);
    srand(12);
    for (size_t i = 0; i < cnt; i++) RV[i] = A[i] = (double) rand() / RAND_MAX;      /* qr.cu:765-771 */

    double* tau = NULL;
    mmqr(RV, &tau, m, n);                       /* untimed: first call pays library/context initialisation */
    free(tau);
    double el = 0.0;
    for (int t = 0; t < TRIALS; t++) {
        memcpy(RV, A, sizeof(double) * cnt);    /* refresh, untimed like qr.cu:786-787 */
        const double t0 = now();
        if (mmqr_status(RV, &tau, m, n)) { fprintf(stderr, "mmqr failed\n"); return 1; }
        el += now() - t0;
        free(tau);
    }
    const double flops = 2.0 * m * (double) n * n - 2.0 * (double) n * n * n / 3.0;
    printf(" MMQR ran QR on %dx%d matrix in %f s (avg over %d)   [host pointers: alloc + H2D + QR + D2H, %.1f GFLOP/s fp64]\n",
           m, n, el / TRIALS, TRIALS, flops / (el / TRIALS) / 1e9);

    /* the same factorisation with the matrix already resident in HBM (plan API; what bench.py reports) */
    qr_plan* p = NULL;
    double *dA = NULL, *dtau = NULL;
    if (qr_plan_create(&p, m, n, 0, 0) || qr_device_malloc((void**) &dA, sizeof(double) * cnt) ||
        qr_device_malloc((void**) &dtau, sizeof(double) * n)) { fprintf(stderr, "device setup failed\n"); return 1; }
    el = 0.0;
    for (int t = -1; t < TRIALS; t++) {
        if (qr_copy_to_device(dA, A, sizeof(double) * cnt)) { fprintf(stderr, "copy failed\n"); return 1; }
        const double t0 = now();
        if (qr_geqrf_dev(p, dA, m, n, m, dtau) || qr_plan_sync(p)) { fprintf(stderr, "qr_geqrf_dev failed\n"); return 1; }
        if (t >= 0) el += now() - t0;
    }
    printf(" MMQR ran QR on %dx%d matrix in %f s (avg over %d)   [matrix resident in HBM, %.1f GFLOP/s fp64]\n",
           m, n, el / TRIALS, TRIALS, flops / (el / TRIALS) / 1e9);
    if (compare && vendor_line(A, dA, dtau, m, n, flops)) return 1;
    if (pivot && pivot_line(p, A, dA, dtau, m, n)) return 1;
    qr_device_free(dA); qr_device_free(dtau);
    qr_plan_destroy(p);
    free(A); free(RV);
    return 0;
}
