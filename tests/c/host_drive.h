/* host_drive.h -- TEST-ONLY helpers shared by the drivers of the C host layer over the stub device layer (host_sanitize.c: the
 * sanitizer run; host_order.c: one schedule configuration per process for the stream-order check; host_units.c: the per-interface units). */
#ifndef HOST_DRIVE_H
#define HOST_DRIVE_H
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/mi355x_qr.h"

long qrd_stub_launches(void);
long qrd_stub_stalls(void);
int qrd_stub_live_allocations(void);

/* ---- the drivers of the per-interface units (host_units.c): the stub's hooks, caller-side buffers, the call macros ---- */
int qrd_malloc(void** p, size_t bytes);
int qrd_free(void* p);
long qrd_stub_order_reports(void);
int qrd_stub_fail_take(void);
long qrd_stub_alloc_count(void);
int qrd_stub_alloc_site(long k, size_t* bytes, const char** func, const char** expr);
void qrd_stub_script(const char* entry, const double* v, int n);
void qrd_stub_set_diag(double d);
void qrd_stub_set_info(int v);
void qrd_stub_guard(const void* p, size_t bytes);

/* caller-side device buffers: straight from the stub (not counted as the library's), exactly the size asked, freed by dev_free_all */
static void* g_dev_buf[512] __attribute__((unused));
static int g_dev_nbuf __attribute__((unused));
static inline void* dev_bytes(size_t bytes)
{
    void* p = NULL;
    if (g_dev_nbuf == 512 || qrd_malloc(&p, bytes)) { fprintf(stderr, "driver: out of device buffers\n"); exit(1); }
    return g_dev_buf[g_dev_nbuf++] = p;
}
/* `batch` blocks rows x cols at leading dimension ld, stride doubles apart: the documented minimum, to the last element of the last block */
static inline double* dev_blocks(long rows, long cols, long ld, long batch, long stride)
{ return (double*) dev_bytes(sizeof(double) * (size_t) ((batch - 1) * stride + (cols - 1) * ld + rows)); }
static inline double* dev_block(long rows, long cols, long ld) { return dev_blocks(rows, cols, ld, 1, 0); }
static inline double* dev_vec(long n) { return dev_block(n, 1, n); }
static inline int* dev_ints(long n) { return (int*) dev_bytes(sizeof(int) * (size_t) n); }
static inline void dev_free_all(void) { while (g_dev_nbuf) qrd_free(g_dev_buf[--g_dev_nbuf]); }

/* CALL(x): x must return 0.  Under QRD_STUB_FAIL_MALLOC a call that returns QR_E_ALLOC after the injected failure fired is made once more,
 * on the same plan and handles, and must then complete.  CALLS(setup, x, want): `setup` runs before every attempt (scripted words), the
 * call must return `want`.  ARG(x): QR_E_ARG, and nothing was launched. */
static int g_fail_hits __attribute__((unused));
#define CALLS(setup, x, want) do { setup; int rc_ = (x); if (rc_ == QR_E_ALLOC && qrd_stub_fail_take()) { ++g_fail_hits; setup; rc_ = (x); } \
    if (rc_ != (want)) { fprintf(stderr, "%s:%d: %s -> %d (%s), expected %d\n", __FILE__, __LINE__, #x, rc_, qr_strerror(rc_), (int) (want)); exit(1); } } while (0)
#define CALLX(x, want) CALLS((void) 0, x, want)
#define CALL(x) CALLS((void) 0, x, 0)
#define ARG(x) do { const long l0_ = qrd_stub_launches(); const int rc_ = (x); if (rc_ != QR_E_ARG || qrd_stub_launches() != l0_) { \
    fprintf(stderr, "%s:%d: %s -> %d with %ld launches, expected QR_E_ARG and none\n", __FILE__, __LINE__, #x, rc_, qrd_stub_launches() - l0_); exit(1); } } while (0)

#define OK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s:%d: %s -> %d (%s)\n", __FILE__, __LINE__, #x, rc_, qr_strerror(rc_)); exit(1); } } while (0)

static inline void factor_once(int pm, int pn, int nb, int m, int n, int with_q, int profile)
{
    qr_plan* p = NULL;
    double *dA = NULL, *dtau = NULL, *dQ = NULL, *dR = NULL;
    OK(qr_plan_create(&p, pm, pn, nb, 0));
    OK(qr_device_malloc((void**) &dA, sizeof(double) * (size_t) m * n));
    OK(qr_device_malloc((void**) &dtau, sizeof(double) * n));
    if (profile) OK(qr_plan_set_profile(p, 1));
    OK(qr_geqrf_dev(p, dA, m, n, m, dtau));
    OK(qr_geqrf_dev(p, dA, m, n, m, dtau));
    if (profile) { qr_profile pr; OK(qr_plan_get_profile(p, &pr)); }
    if (with_q) {
        OK(qr_device_malloc((void**) &dQ, sizeof(double) * (size_t) m * n));
        OK(qr_device_malloc((void**) &dR, sizeof(double) * (size_t) n * n));
        OK(qr_extract_r_dev(p, dA, m, n, m, dR, n, n));
        OK(qr_applyq_dev(p, dA, m, n, m, dtau, dQ, n, m, 1));
        OK(qr_applyq_dev(p, dA, m, n, m, dtau, dQ, n, m, 0));
    }
    OK(qr_plan_sync(p));
    OK(qr_device_free(dA)); OK(qr_device_free(dtau)); OK(qr_device_free(dQ)); OK(qr_device_free(dR));
    OK(qr_plan_destroy(p));
}

/* one rank of a multi-rank TSQR over the stub's thread communicators: four steps, the joint fall-back decision before the third */
int qrd_comm_init_all(void** comms, int n, const int* devs);
int qrd_comm_destroy(void* comm);
typedef struct { void* comm; int rank, P, expect_fallback, bad; } tsqr_rank_arg;
static inline void* tsqr_rank(void* arg)
{
    tsqr_rank_arg* a = (tsqr_rank_arg*) arg;
    const int ml = 8192, n = 256;
    qr_tsqr_plan* t = NULL;
    double *dA = NULL, *dR = NULL, st[5];
    OK(qr_tsqr_plan_create_comm(&t, a->comm, a->P, a->rank, ml, n, 64));
    OK(qr_device_malloc((void**) &dA, sizeof(double) * (size_t) ml * n));
    OK(qr_device_malloc((void**) &dR, sizeof(double) * (size_t) n * n));
    if (!qr_tsqr_is_pipelined(t)) a->bad = 1;
    for (int it = 0; it < 4; ++it) OK(qr_tsqr_factor_dev(t, dA, ml, dR));
    OK(qr_tsqr_gather_stats(t, st));
    if ((int) st[4] != a->expect_fallback || qr_tsqr_is_pipelined(t) == a->expect_fallback) a->bad = 2;
    if (!a->expect_fallback && !(st[0] > 0.0 && st[1] > 0.0 && st[2] > st[0])) a->bad = 3;
    OK(qr_tsqr_plan_destroy(t));
    OK(qr_device_free(dA)); OK(qr_device_free(dR));
    return NULL;
}
static inline int tsqr_ranks_run(int expect_fallback)
{
    enum { P = 3 };
    void* comms[P];
    const int devs[P] = {0, 1, 2};
    pthread_t th[P];
    tsqr_rank_arg args[P];
    OK(qrd_comm_init_all(comms, P, devs));
    for (int r = 0; r < P; ++r) {
        args[r] = (tsqr_rank_arg){comms[r], r, P, expect_fallback, 0};
        pthread_create(&th[r], NULL, tsqr_rank, &args[r]);
    }
    int bad = 0;
    for (int r = 0; r < P; ++r) { pthread_join(th[r], NULL); if (args[r].bad) bad = args[r].bad; }
    for (int r = P - 1; r >= 0; --r) qrd_comm_destroy(comms[r]);
    return bad;
}

#endif
