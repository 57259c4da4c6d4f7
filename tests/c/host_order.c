/* host_order.c -- TEST-ONLY driver of the C host layer over the stub device layer for the STREAM-ORDER check (qrd_stub.c keeps a
 * happens-before model of streams and events; tests/test_schedule_order.py).  One schedule configuration per process -- the knobs are
 * read once per process -- named by argv[1]; `host_order list` prints the names, `host_order factor m n nb` factors one m x n matrix
 * twice under the caller's own environment (which branches does a GPU test's configuration take?).  The run is in count mode: it ends with
 *   ORDER <reports> <waits>            and one line per stream_wait_event of the run, in call order:
 *   WAIT <k> <site> <function>:<event expression>
 * (site: serial number of the call site in qr_host.c, see order_sites.h), so that the wait-removal sweep (QRD_STUB_SKIP_WAIT=k) can say
 * which wait it took out.  Shapes are the smallest at which the branch in question is taken: the stub computes nothing. */
#define _POSIX_C_SOURCE 200809L
#include "host_drive.h"

long qrd_stub_order_reports(void);
long qrd_stub_wait_count(void);
int qrd_stub_wait_site(long k, const char** func, const char** expr, int* site);

/* geqrf -> extract_r -> applyq -> geqrf of a second matrix on one plan, no sync in between */
static void chain_once(int m, int n, int nb)
{
    qr_plan* p = NULL;
    double *dA = NULL, *dB = NULL, *dtau = NULL, *dQ = NULL, *dR = NULL;
    OK(qr_plan_create(&p, m, n, nb, 0));
    OK(qr_device_malloc((void**) &dA, sizeof(double) * (size_t) m * n));
    OK(qr_device_malloc((void**) &dB, sizeof(double) * (size_t) m * n));
    OK(qr_device_malloc((void**) &dtau, sizeof(double) * 2 * n));
    OK(qr_device_malloc((void**) &dQ, sizeof(double) * (size_t) m * n));
    OK(qr_device_malloc((void**) &dR, sizeof(double) * (size_t) n * n));
    OK(qr_geqrf_dev(p, dA, m, n, m, dtau));
    OK(qr_extract_r_dev(p, dA, m, n, m, dR, n, n));
    OK(qr_applyq_dev(p, dA, m, n, m, dtau, dQ, n, m, 1));
    OK(qr_geqrf_dev(p, dB, m, n, m, dtau + n));
    OK(qr_plan_sync(p));
    OK(qr_device_free(dA)); OK(qr_device_free(dB)); OK(qr_device_free(dtau)); OK(qr_device_free(dQ)); OK(qr_device_free(dR));
    OK(qr_plan_destroy(p));
}

static void tsqr_external(void)
{
    const int ml = 8192, n = 128, P = 4;
    qr_tsqr_plan* t = NULL;
    double *dA = NULL, *dR = NULL, *dQ = NULL, *send = NULL, *recv = NULL;
    OK(qr_tsqr_plan_create_comm(&t, NULL, P, 1, ml, n, 0));
    OK(qr_device_malloc((void**) &dA, sizeof(double) * (size_t) ml * n));
    OK(qr_device_malloc((void**) &dQ, sizeof(double) * (size_t) ml * n));
    OK(qr_device_malloc((void**) &dR, sizeof(double) * (size_t) n * n));
    OK(qr_tsqr_exchange_buffers(t, &send, &recv));
    for (int it = 0; it < 3; ++it) {
        OK(qr_tsqr_local_dev(t, dA, ml));
        OK(qr_tsqr_stacked_dev(t, dR));
    }
    OK(qr_tsqr_formq_dev(t, dA, ml, dQ, ml));
    OK(qr_tsqr_formq_dev(t, dA, ml, dQ, ml));
    OK(qr_tsqr_sync(t));
    OK(qr_tsqr_plan_destroy(t));
    OK(qr_tsqr_plan_create(&t, NULL, 1, 0, ml, n, 0));
    OK(qr_tsqr_factor_dev(t, dA, ml, dR));
    OK(qr_tsqr_formq_dev(t, dA, ml, dQ, ml));
    OK(qr_tsqr_plan_destroy(t));
    OK(qr_device_free(dA)); OK(qr_device_free(dQ)); OK(qr_device_free(dR));
}

static void tsqr_virtual(void)
{
    enum { P = 3 };
    const int ml = 16384, n = 384;
    qr_tsqr_plan* tps[P];
    double *dA[P], *dR[P];
    for (int r = 0; r < P; ++r) {
        OK(qr_tsqr_plan_create_comm(&tps[r], NULL, P, r, ml, n, 128));
        OK(qr_device_malloc((void**) &dA[r], sizeof(double) * (size_t) ml * n));
        OK(qr_device_malloc((void**) &dR[r], sizeof(double) * (size_t) n * n));
    }
    OK(qr_tsqr_factor_virtual_dev(tps, P, dA, ml, dR));
    OK(qr_tsqr_factor_virtual_dev(tps, P, dA, ml, dR));
    OK(qr_tsqr_factor_selfgather_dev(tps[1], dA[1], ml, dR[1]));
    OK(qr_tsqr_factor_selfgather_dev(tps[1], dA[1], ml, dR[1]));
    OK(qr_tsqr_formq_dev(tps[1], dA[1], ml, dA[0], ml));
    OK(qr_tsqr_formq_dev(tps[1], dA[1], ml, dA[0], ml));
    for (int r = 0; r < P; ++r) { OK(qr_tsqr_plan_destroy(tps[r])); OK(qr_device_free(dA[r])); OK(qr_device_free(dR[r])); }
}

static void thin_mgpu(void)
{
    const int m = 16384, n = 256;
    double* A = (double*) calloc((size_t) m * n, sizeof(double));
    double* Q = (double*) calloc((size_t) m * n, sizeof(double));
    double* R = (double*) calloc((size_t) n * n, sizeof(double));
    OK(qr_thin_mgpu(A, 4096, 64, Q, R, 0, 4));
    OK(qr_thin_mgpu(A, 4093, 64, Q, R, 0, 3));
    OK(qr_thin_mgpu(A, m, n, Q, R, 64, 4));          /* n a multiple of the block size: the panel-pipelined exchange */
    OK(qr_thin(A, 4096, 64, Q, R, 32, 3));
    free(A); free(Q); free(R);
}

typedef struct { const char *name, *env; int kind, pm, pn, nb, m, n, with_q; } config;
enum { FACTOR, CHAIN, TSQR_EXT, TSQR_VIRT, TSQR_RANKS, TSQR_RANKS_SLOW, MGPU };
#define LA "MI355XQR_LOOKAHEAD=1 "
static const config g_cfg[] = {
    /* single stream, graph replay, the Householder leaf: one stream, no waits -- the NULL-stream and plan-creation operations are checked */
    {"single_stream", "MI355XQR_LOOKAHEAD=0", FACTOR, 1000, 333, 128, 1000, 333, 1},
    {"graph", "MI355XQR_LOOKAHEAD=0 MI355XQR_GRAPH=1", FACTOR, 2000, 500, 128, 2000, 500, 0},
    /* default knobs where lookahead_pays and the default split turn the partition on by themselves */
    {"default", "", FACTOR, 4096, 2048, 0, 4096, 2048, 1},
    {"default_square", "", FACTOR, 3072, 3072, 0, 3072, 3072, 0},
    /* look-ahead on shared CUs (no partition), padded plan (3000 is no multiple of 16), sub-size problem on a larger plan */
    {"shared_cus_padded", LA, FACTOR, 3000, 2100, 128, 3000, 2100, 1},
    {"subsize", LA, FACTOR, 16384, 2048, 256, 8192, 2048, 0},
    /* two-level panels: W_a, W_b, ev_half into factor_panel -- on shared CUs and on a partition */
    {"two_level", LA, FACTOR, 2304, 2304, 512, 2304, 2304, 0},
    {"two_level_wide_last", LA, FACTOR, 2560, 2560, 512, 2560, 2560, 0},          /* the last panel has a second half: W_a(last) is pending at the end */
    {"two_level_split", LA "MI355XQR_SPLIT=64 MI355XQR_BALANCE=14,44,0.05,0.05", FACTOR, 5120, 5120, 512, 5120, 5120, 0},
    /* phases: two masked phases, and an unmasked panel stream over the previous phase's update stream */
    {"split_two_phases", LA "MI355XQR_SPLIT=64:0.5,32", FACTOR, 4096, 2048, 256, 4096, 2048, 0},
    {"split_u_phase", LA "MI355XQR_SPLIT=64:0.5,U", FACTOR, 4096, 2048, 256, 4096, 2048, 0},
    /* where N(s) runs */
    {"next_panel", LA "MI355XQR_SPLIT=64 MI355XQR_NEXT=panel", FACTOR, 4096, 2048, 256, 4096, 2048, 0},
    {"next_update", LA "MI355XQR_SPLIT=64 MI355XQR_NEXT=update", FACTOR, 4096, 2048, 256, 4096, 2048, 0},
    {"next_auto", LA "MI355XQR_SPLIT=64 MI355XQR_NEXT=auto", FACTOR, 6144, 4096, 256, 6144, 4096, 0},
    /* the panel stream's share E(s), early N(s+1) and W1(s); without a share; without the early look-ahead update */
    {"balance_share", LA "MI355XQR_SPLIT=64 MI355XQR_BALANCE=14,44,0.05,0.05", FACTOR, 6144, 4096, 256, 6144, 4096, 0},
    {"balance_share_ragged", LA "MI355XQR_SPLIT=64 MI355XQR_BALANCE=14,44,0.05,0.05", FACTOR, 6144, 4096, 128, 6000, 3900, 0},
    {"balance_none", LA "MI355XQR_SPLIT=64 MI355XQR_BALANCE=0", FACTOR, 6144, 4096, 256, 6144, 4096, 0},
    {"early_next_off", LA "MI355XQR_SPLIT=64 MI355XQR_BALANCE=14,44,0.05,0.05 MI355XQR_EARLY_NEXT=0", FACTOR, 6144, 4096, 256, 6144, 4096, 0},
    /* W(s) in two slices: W1(s) for N(s+1), the rest behind it (more than QR_EARLY_W1 + 1024 wide columns) */
    {"early_next_sliced", LA "MI355XQR_SPLIT=64 MI355XQR_BALANCE=14,44,0.05,0.05", FACTOR, 8192, 8192, 256, 8192, 8192, 0},
    /* the profile's event brackets on both streams */
    {"profile", LA "MI355XQR_SPLIT=64 MI355XQR_BALANCE=14,44,0.05,0.05", FACTOR, 4096, 2048, 256, 4096, 2048, 0},
    /* ev_v and t_wait: V complete before T */
    {"split_t_off", LA "MI355XQR_SPLIT=64 MI355XQR_NEXT=update MI355XQR_SPLIT_T=0", FACTOR, 4096, 2048, 128, 4096, 2048, 0},
    {"split_t_on", LA "MI355XQR_SPLIT=64 MI355XQR_NEXT=update MI355XQR_SPLIT_T=1", FACTOR, 4096, 2048, 128, 4096, 2048, 0},
    {"split_t_on_256", LA "MI355XQR_SPLIT=64 MI355XQR_NEXT=update MI355XQR_SPLIT_T=1 MI355XQR_DEFER_T=0", FACTOR, 4096, 2048, 256, 4096, 2048, 0},
    /* the deferred Gram matrix and merge tree on the update stream, lookahead_update_no_t and both outcomes of its return value */
    {"defer_t_off", LA "MI355XQR_SPLIT=32 MI355XQR_DEFER_T=0", FACTOR, 4096, 2048, 256, 4096, 2048, 0},
    {"defer_t_trsm", LA "MI355XQR_SPLIT=32 MI355XQR_DEFER_T=1 MI355XQR_TRSM=1", FACTOR, 4096, 2048, 256, 4096, 2048, 0},
    {"defer_t_tree_first", LA "MI355XQR_SPLIT=32 MI355XQR_DEFER_T=1 MI355XQR_TRSM=0", FACTOR, 4096, 2048, 256, 4096, 2048, 0},
    {"defer_t_ragged", LA "MI355XQR_SPLIT=32 MI355XQR_DEFER_T=1 MI355XQR_TRSM=1", FACTOR, 4096, 2040, 256, 4096, 2040, 0},
    {"defer_t_share", LA "MI355XQR_SPLIT=64 MI355XQR_NEXT=update MI355XQR_BALANCE=14,44,0,0 MI355XQR_EARLY_NEXT=0 MI355XQR_DEFER_T=1", FACTOR, 4096, 2048, 256, 4096, 2048, 0},
    {"defer_t_next_panel", LA "MI355XQR_SPLIT=32 MI355XQR_DEFER_T=1 MI355XQR_NEXT=panel", FACTOR, 4096, 2048, 256, 4096, 2048, 0},
    /* the full-width panel on a look-ahead plan; the stub's guard refuses heights with bit 12 set and a retry with bit 7 set as well:
     * 5120 refused, retried, accepted; 4992 refused twice (leaf chain); 4864 ... */
    {"cqr_lookahead", LA "MI355XQR_CQR_MIN_ROWS=1024 MI355XQR_CQR_MIN_ROWS_LA=1024", FACTOR, 5120, 768, 128, 5120, 768, 1},
    {"cqr_lookahead_split", LA "MI355XQR_SPLIT=64 MI355XQR_CQR_MIN_ROWS=1024 MI355XQR_CQR_MIN_ROWS_LA=1024", FACTOR, 5120, 768, 128, 5120, 768, 0},
    /* across calls on one plan without a sync (factor_once issues two factorisations back to back as well) */
    {"chain", "", CHAIN, 0, 0, 0, 4096, 2048, 0},
    {"chain_split_u", LA "MI355XQR_SPLIT=64:0.5,U", CHAIN, 0, 0, 256, 4096, 2048, 0},
    /* the TSQR plan and the per-device threads */
    {"tsqr_external", "", TSQR_EXT, 0, 0, 0, 0, 0, 0},
    {"tsqr_virtual", "", TSQR_VIRT, 0, 0, 0, 0, 0, 0},
    {"tsqr_ranks", "", TSQR_RANKS, 0, 0, 0, 0, 0, 0},
    {"tsqr_ranks_fallback", "QRD_STUB_GATHER_MS=50", TSQR_RANKS_SLOW, 0, 0, 0, 0, 0, 0},
    {"thin_mgpu", "", MGPU, 0, 0, 0, 0, 0, 0},
};

int main(int argc, char** argv)
{
    const int ncfg = (int) (sizeof g_cfg / sizeof g_cfg[0]);
    if (argc < 2) { fprintf(stderr, "usage: host_order <configuration> | list | env <configuration> | factor m n nb\n"); return 2; }
    if (!strcmp(argv[1], "list")) { for (int i = 0; i < ncfg; ++i) printf("%s\n", g_cfg[i].name); return 0; }
    const config custom = {"factor", "", FACTOR, argc > 4 ? atoi(argv[2]) : 0, argc > 4 ? atoi(argv[3]) : 0, argc > 4 ? atoi(argv[4]) : 0,
                           argc > 4 ? atoi(argv[2]) : 0, argc > 4 ? atoi(argv[3]) : 0, 0};
    const char* name = !strcmp(argv[1], "env") && argc > 2 ? argv[2] : argv[1];
    const config* c = NULL;
    for (int i = 0; i < ncfg; ++i) if (!strcmp(name, g_cfg[i].name)) c = &g_cfg[i];
    if (!strcmp(name, "factor") && argc > 4) c = &custom;
    if (!c) { fprintf(stderr, "host_order: no configuration '%s'\n", name); return 2; }
    if (name != argv[1]) { printf("%s\n", c->env); return 0; }
    {
        char env[512];
        snprintf(env, sizeof env, "%s", c->env);
        char* save = NULL;
        for (char* tok = strtok_r(env, " ", &save); tok; tok = strtok_r(NULL, " ", &save)) {
            char* eq = strchr(tok, '=');
            *eq = 0;
            setenv(tok, eq + 1, 1);
        }
    }
    setenv("QRD_STUB_ORDER", "count", 0);
    switch (c->kind) {
    case FACTOR: factor_once(c->pm, c->pn, c->nb, c->m, c->n, c->with_q, !strcmp(c->name, "profile")); break;
    case CHAIN: chain_once(c->m, c->n, c->nb); break;
    case TSQR_EXT: tsqr_external(); break;
    case TSQR_VIRT: tsqr_virtual(); break;
    case TSQR_RANKS: if (tsqr_ranks_run(0)) return 10; break;
    case TSQR_RANKS_SLOW: if (tsqr_ranks_run(1)) return 11; break;
    case MGPU: thin_mgpu(); break;
    }
    if (qrd_stub_live_allocations() != 0) { fprintf(stderr, "device-memory leak: %d allocations still live\n", qrd_stub_live_allocations()); return 6; }
    const long nw = qrd_stub_wait_count();
    printf("ORDER %ld %ld\n", qrd_stub_order_reports(), nw);
    for (long k = 1; k <= nw; ++k) {
        const char *f = NULL, *e = NULL;
        int site = -1;
        if (qrd_stub_wait_site(k, &f, &e, &site)) break;
        printf("WAIT %ld %d %s:%s\n", k, site, f ? f : "?", e ? e : "?");
    }
    return 0;
}
