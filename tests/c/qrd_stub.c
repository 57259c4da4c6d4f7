/* qrd_stub.c -- TEST-ONLY stand-in for the HIP launch layer (cuda-qr_amd/csrc/qr_device.h), so that the C host layer
 * (qr_host.c: schedule, plan cache, TSQR plan, per-device threads) can run under AddressSanitizer / UBSan / ThreadSanitizer on a
 * box without a GPU (SURVEY section 5 "race detection / sanitizers"; GPU sanitizers are not available on the pool).
 *
 * It computes NOTHING: "device memory" is host calloc, copies are memcpy, every kernel launch only CHECKS the operand blocks it was
 * given and returns.  Two checks, both always on:
 *   BOUNDS  every operand block lies inside one live allocation (an out-of-range workspace index in the schedule aborts here);
 *   ORDER   a happens-before model of streams and events (DESIGN "Stream-order model of the stub").  Every stream and every host
 *           thread has a vector clock over the streams.  A device operation issued by host thread H on stream S joins H's clock into
 *           S's, ticks S and stamps its operand blocks -- tagged read / write / read-write after the contract of qr_device.h -- with
 *           (S, tick) in the access log of their allocation.  event_record copies S's clock into the event, stream_wait_event joins the
 *           event's clock AS OF THE CALL into the stream (an event never recorded orders nothing), stream_sync / event_sync join into
 *           the calling host thread, device_sync and qrd_free join every stream of the thread's device, the all-gather joins the
 *           participating ranks' streams at its barrier.  Two accesses conflict when their element sets intersect (exactly, for
 *           column-major blocks of any two leading dimensions), at least one writes, and the earlier one (Sa, ta) is not ordered
 *           before the later operation b: clock_b[Sa] < ta.  A conflict aborts like a bounds error; QRD_STUB_ORDER=count prints
 *           the first 20, goes on and counts (qrd_stub_order_reports).
 *           The NULL stream is a stream of its own (index 0): the plan's streams are non-blocking, so it orders nothing against them;
 *           the operations the host layer issues on it are counted (qrd_stub_null_stream_ops).
 *           The host-polled hand-off word of the full-width panel (cq_hword / hflag) is NOT modelled as a join: the host layer uses
 *           what it reads there only to choose what to queue next ON THE SAME STREAM (retry, leaf chain), never to order two streams.
 *           Log entries ordered before every live stream are pruned (the NULL stream is not counted there: its only users are the
 *           blocking copies, which end in a host sync); tile-padding over-reads of the real loaders are not modelled.
 *           Test hooks: QRD_STUB_SKIP_WAIT=k lets the k-th stream_wait_event of the process return without joining; qrd_stub_wait_at
 *           is stream_wait_event with the caller's site (the `order` build of the Makefile routes qr_host.c's calls through it).
 *           QRD_STUB_FAIL_MALLOC=k / QRD_STUB_SHRINK_MALLOC=k: see qrd_stub_malloc_at; qrd_stub_guard: a block no launch may write.
 * The launches of the per-interface host units (qr_solve.c ... qr_batched_lm.c) and the scripted device words that drive their host
 * loops are in qrd_stub_units.c, included at the end of this file.
 * It is never linked into libmi355xqr.so and nothing under cuda-qr_amd/ refers to it. */
#define _POSIX_C_SOURCE 200809L
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../cuda-qr_amd/csrc/qr_device.h"

static long g_stub_stalls = 0;      /* injected stalls of the one-launch panel (QRD_STUB_STALL_ONCE) */

/* ---- the order model's state: all of it under g_mu, but the host thread's own clock ---- */
#define MAXS 256                    /* stream slots; slot 0 is the NULL stream.  A destroyed stream's slot is used again, its tick goes on */
typedef struct vclock { uint32_t c[MAXS]; } vclock;
typedef struct stub_slot { int live, cus, dev; uint32_t tick; vclock clk; } stub_slot;
static stub_slot g_slot[MAXS] = {{1, 256, 0, 0, {{0}}}};
static int g_hi = 1;                /* slots [0, g_hi) have been in use */
static __thread vclock t_host;      /* what this host thread has synchronised with */
enum { ACC_R = 1, ACC_W = 2, ACC_RW = 3 };
typedef struct acc {
    size_t off, run, stride;        /* bytes: `ncols` runs of `run` bytes, `stride` apart, from `off` into the allocation */
    long ncols;
    uint32_t slot, tick;
    int mode;
    const char *op, *what;
} acc;
static __thread struct { uint32_t slot, tick; const char* name; vclock clk; } t_op;      /* the device operation being issued */
static int g_order_mode = -1;       /* 0 abort, 1 count */
static long g_order_reports, g_null_ops;

#define MAXA 4096
static struct { char* p; size_t n; acc* log; int nlog, cap, prune_at; } g_alloc[MAXA];
static int g_nalloc;
static pthread_mutex_t g_mu = PTHREAD_MUTEX_INITIALIZER;
static __thread int t_dev = 0;
static long g_launches;

static void die(const char* what, const void* p, size_t bytes)
{
    fprintf(stderr, "qrd_stub: %s: block %p + %zu bytes is not inside a live device allocation\n", what, p, bytes);
    abort();
}

static void vc_join(vclock* d, const vclock* s) { for (int i = 0; i < g_hi; ++i) if (s->c[i] > d->c[i]) d->c[i] = s->c[i]; }

typedef struct stub_stream { int cus, slot; } stub_stream;
static int slot_of(void* s) { return s ? ((stub_stream*) s)->slot : 0; }

/* a device operation starts: host clock into the stream's, tick, remember (stream, tick, clock) for the operand stamps */
static void op_begin(void* s, const char* name)
{
    const int k = slot_of(s);
    pthread_mutex_lock(&g_mu);
    if (!s) ++g_null_ops;
    vc_join(&g_slot[k].clk, &t_host);
    g_slot[k].clk.c[k] = ++g_slot[k].tick;
    t_op.slot = (uint32_t) k; t_op.tick = g_slot[k].tick; t_op.name = name;
    memcpy(t_op.clk.c, g_slot[k].clk.c, sizeof(uint32_t) * (size_t) g_hi);
    pthread_mutex_unlock(&g_mu);
}

/* exact intersection of two strided blocks of one allocation: 0 when disjoint, else the first shared byte and how many are shared */
static int acc_overlap(const acc* a, const acc* b, size_t* first, size_t* total)
{
    const size_t aend = a->off + a->stride * (size_t) (a->ncols - 1) + a->run, bend = b->off + b->stride * (size_t) (b->ncols - 1) + b->run;
    if (aend <= b->off || bend <= a->off) return 0;
    const acc *x = a, *y = b;           /* walk the columns of the block that has fewer */
    if (x->ncols > y->ncols) { x = b; y = a; }
    size_t f = (size_t) -1, tot = 0;
    for (long i = 0; i < x->ncols; ++i) {
        const size_t lo = x->off + x->stride * (size_t) i, hi = lo + x->run;
        if (hi <= y->off) continue;
        long j0 = lo < y->off + y->run ? 0 : (long) ((lo - y->off - y->run) / y->stride) + 1;
        long j1 = (long) ((hi - 1 - y->off) / y->stride);
        if (j1 > y->ncols - 1) j1 = y->ncols - 1;
        for (long j = j0; j <= j1; ++j) {
            const size_t ylo = y->off + y->stride * (size_t) j, yhi = ylo + y->run;
            const size_t l = lo > ylo ? lo : ylo, h = hi < yhi ? hi : yhi;
            if (l < h) { tot += h - l; if (l < f) f = l; }
        }
    }
    if (!tot) return 0;
    *first = f; *total = tot;
    return 1;
}

static const char* mode_name(int m) { return m == ACC_R ? "read" : (m == ACC_W ? "write" : "read-write"); }

static void order_report(int ai, const acc* old, const acc* now, size_t first, size_t total)
{
    if (g_order_mode < 0) { const char* e = getenv("QRD_STUB_ORDER"); g_order_mode = e && !strcmp(e, "count"); }
    ++g_order_reports;
    if (!g_order_mode || g_order_reports <= 20)
        fprintf(stderr, "qrd_stub: ORDER: %s [%s, %s] on stream %u (%d CUs) is not ordered after %s [%s, %s] on stream %u (%d CUs): "
                        "they share %zu bytes from offset %zu of allocation %p (%zu bytes)\n",
                now->op, now->what, mode_name(now->mode), now->slot, g_slot[now->slot].cus, old->op, old->what, mode_name(old->mode), old->slot,
                g_slot[old->slot].cus, total, first, (void*) g_alloc[ai].p, g_alloc[ai].n);
    if (!g_order_mode) abort();
}

/* drop the entries of allocation ai that are ordered before every live stream (not counting the NULL stream) */
static void log_prune(int ai)
{
    int n = 0;
    for (int i = 0; i < g_alloc[ai].nlog; ++i) {
        const acc* a = &g_alloc[ai].log[i];
        int keep = 0;
        for (int k = 1; k < g_hi && !keep; ++k) if (g_slot[k].live && g_slot[k].clk.c[a->slot] < a->tick) keep = 1;
        if (keep) g_alloc[ai].log[n++] = *a;
    }
    g_alloc[ai].nlog = n;
    g_alloc[ai].prune_at = 2 * n + 64;
}

/* stamp one operand block of the current operation (g_mu held): report what it conflicts with, then log it */
static void order_access(int ai, const char* what, size_t off, size_t run, size_t stride, long ncols, int mode)
{
    acc now = {off, run, stride, ncols, t_op.slot, t_op.tick, mode, t_op.name ? t_op.name : "?", what};
    acc* same = NULL;
    for (int i = 0; i < g_alloc[ai].nlog; ++i) {
        acc* a = &g_alloc[ai].log[i];
        if (a->slot == now.slot) {      /* same stream: ordered.  The same block in the same mode: the later stamp stands for both */
            if (!same && a->off == off && a->run == run && a->stride == stride && a->ncols == ncols && a->mode == mode) same = a;
            continue;
        }
        if (!((a->mode | mode) & ACC_W)) continue;
        if (t_op.clk.c[a->slot] >= a->tick) continue;
        size_t first = 0, total = 0;
        if (acc_overlap(a, &now, &first, &total)) order_report(ai, a, &now, first, total);
    }
    if (same) { same->tick = now.tick; same->op = now.op; same->what = now.what; return; }
    if (g_alloc[ai].nlog >= g_alloc[ai].prune_at) log_prune(ai);
    if (g_alloc[ai].nlog == g_alloc[ai].cap) {
        const int cap = g_alloc[ai].cap ? 2 * g_alloc[ai].cap : 32;
        acc* l = (acc*) realloc(g_alloc[ai].log, sizeof(acc) * (size_t) cap);
        if (!l) { fprintf(stderr, "qrd_stub: out of memory for the access log\n"); abort(); }
        g_alloc[ai].log = l; g_alloc[ai].cap = cap;
    }
    g_alloc[ai].log[g_alloc[ai].nlog++] = now;
}

/* `ncols` runs of `run` bytes, `stride` bytes apart, at p: inside ONE live allocation?  Then stamp them for the order model */
static const char* g_guard_p;      /* qrd_stub_guard: a block no launch may write while it is set (a rollback must leave it alone) */
static size_t g_guard_n;
void qrd_stub_guard(const void* p, size_t bytes) { g_guard_p = (const char*) p; g_guard_n = p ? bytes : 0; }
static void chk_bytes(const char* what, const void* p, size_t run, size_t stride, long ncols, int mode)
{
    const size_t bytes = stride * (size_t) (ncols - 1) + run;      /* (allocations are whole multiples of 8 bytes: no rounding is needed, and a block of ints may start between two) */
    const char* c = (const char*) p;
    int ok = 0;
    if (g_guard_n && (mode & ACC_W) && c < g_guard_p + g_guard_n && g_guard_p < c + bytes) {
        fprintf(stderr, "qrd_stub: %s: writes %p + %zu bytes, inside the guarded block %p + %zu\n", what, p, bytes, (const void*) g_guard_p, g_guard_n);
        abort();
    }
    pthread_mutex_lock(&g_mu);
    for (int i = 0; i < g_nalloc && !ok; ++i)
        if (c >= g_alloc[i].p && c + bytes <= g_alloc[i].p + g_alloc[i].n) {
            ok = 1;
            order_access(i, what, (size_t) (c - g_alloc[i].p), run, stride, ncols, mode);
        }
    ++g_launches;
    pthread_mutex_unlock(&g_mu);
    if (!ok) die(what, p, bytes);
}
/* column-major block rows x cols (doubles) with leading dimension ld at p */
static void chk(const char* what, const void* p, long ld, long rows, long cols, int mode)
{
    if (rows <= 0 || cols <= 0) return;
    if (!p) die(what, p, 0);
    if (ld < rows) { fprintf(stderr, "qrd_stub: %s: ld %ld < rows %ld\n", what, ld, rows); abort(); }
    chk_bytes(what, p, sizeof(double) * (size_t) rows, sizeof(double) * (size_t) ld, cols, mode);
}
static void chkb(const char* what, const void* p, size_t bytes, int mode)
{
    if (!bytes) return;
    if (!p) die(what, p, 0);
    chk_bytes(what, p, bytes, bytes, 1, mode);
}
#define RD ACC_R
#define WR ACC_W
#define RW ACC_RW
#define BETA(be) ((be) == 0.0 ? WR : RW)

long qrd_stub_launches(void) { return g_launches; }
int qrd_stub_live_allocations(void) { return g_nalloc; }
long qrd_stub_order_reports(void) { pthread_mutex_lock(&g_mu); const long r = g_order_reports; pthread_mutex_unlock(&g_mu); return r; }
long qrd_stub_null_stream_ops(void) { pthread_mutex_lock(&g_mu); const long r = g_null_ops; pthread_mutex_unlock(&g_mu); return r; }

void qrd_range_push(const char* name) { (void) name; }
void qrd_range_pop(void) { }
int qrd_init(void) { return 0; }
int qrd_gemm2_init(void) { return 0; }
int qrd_panel_tsqr_init(void) { return 0; }
int qrd_leaf_fused_init(void) { return 0; }
int qrd_panel_fused_init(void) { return 0; }

/* The LIBRARY's allocations of the process, in call order (tests/c/units_sites.h routes the qrd_malloc calls of the host units through
 * qrd_stub_malloc_at with their site: the calling function and the text of the pointer expression).  A call without a site, or from
 * qr_device_malloc, is the caller's own buffer and is not counted.  QRD_STUB_FAIL_MALLOC=k: the k-th counted allocation fails, once, with
 * QR_E_ALLOC's value (-102; the real layer hands hipErrorOutOfMemory up the same way) -- qrd_stub_fail_take tells the driver that it did;
 * QRD_STUB_SHRINK_MALLOC=k: the k-th one is 8 bytes shorter than asked (tests/test_units_stub.py: every workspace is checked and tight). */
#define MAXSITE 4096
static struct { size_t bytes; const char *func, *expr; } g_site[MAXSITE];
static long g_nsite, g_fail_at = -1, g_shrink_at = -1;
static int g_fail_fired;
int qrd_stub_malloc_at(void** p, size_t bytes, const char* func, const char* expr)
{
    if (!p) return 1;
    size_t n = (bytes + 7) & ~(size_t) 7;
    if (!n) n = 8;
    const int counted = func && strcmp(func, "qr_device_malloc") != 0;
    pthread_mutex_lock(&g_mu);
    if (g_fail_at < 0) {
        const char *f = getenv("QRD_STUB_FAIL_MALLOC"), *s = getenv("QRD_STUB_SHRINK_MALLOC");
        g_fail_at = f ? atol(f) : 0; g_shrink_at = s ? atol(s) : 0;
    }
    long k = 0;
    if (counted) {
        if (g_nsite < MAXSITE) { g_site[g_nsite].bytes = bytes; g_site[g_nsite].func = func; g_site[g_nsite].expr = expr; }
        k = ++g_nsite;
    }
    if (k && k == g_fail_at) { g_fail_fired = 1; pthread_mutex_unlock(&g_mu); *p = NULL; return -102; }
    const size_t keep = (k && k == g_shrink_at) ? n - 8 : n;      /* what the bounds check believes; the host block keeps its size */
    pthread_mutex_unlock(&g_mu);
    char* q = (char*) calloc(1, n);
    if (!q) return 2;
    pthread_mutex_lock(&g_mu);
    if (g_nalloc == MAXA) { pthread_mutex_unlock(&g_mu); free(q); return 2; }
    memset(&g_alloc[g_nalloc], 0, sizeof g_alloc[0]);
    g_alloc[g_nalloc].p = q; g_alloc[g_nalloc].n = keep; g_alloc[g_nalloc].prune_at = 64; ++g_nalloc;
    pthread_mutex_unlock(&g_mu);
    *p = q;
    return 0;
}
int qrd_malloc(void** p, size_t bytes) { return qrd_stub_malloc_at(p, bytes, NULL, NULL); }
int qrd_stub_fail_take(void) { pthread_mutex_lock(&g_mu); const int f = g_fail_fired; g_fail_fired = 0; pthread_mutex_unlock(&g_mu); return f; }
long qrd_stub_alloc_count(void) { pthread_mutex_lock(&g_mu); const long n = g_nsite; pthread_mutex_unlock(&g_mu); return n; }
int qrd_stub_alloc_site(long k, size_t* bytes, const char** func, const char** expr)
{
    if (k < 1 || k > g_nsite || k > MAXSITE) return 1;
    *bytes = g_site[k - 1].bytes; *func = g_site[k - 1].func; *expr = g_site[k - 1].expr;
    return 0;
}
/* every stream of the calling thread's device (the NULL stream too) joins the host thread: hipDeviceSynchronize, and hipFree */
static void join_device_locked(void)
{
    for (int k = 0; k < g_hi; ++k) if (k == 0 || g_slot[k].dev == t_dev) vc_join(&t_host, &g_slot[k].clk);
}
int qrd_free(void* p)
{
    if (!p) return 0;
    pthread_mutex_lock(&g_mu);
    int found = 0;
    for (int i = 0; i < g_nalloc; ++i)
        if (g_alloc[i].p == (char*) p) { free(g_alloc[i].log); g_alloc[i] = g_alloc[--g_nalloc]; found = 1; break; }
    join_device_locked();
    pthread_mutex_unlock(&g_mu);
    if (!found) { fprintf(stderr, "qrd_stub: qrd_free of %p, which is not a live allocation (double free?)\n", p); abort(); }
    free(p);
    return 0;
}
int qrd_memset(void* s, void* p, int v, size_t bytes) { op_begin(s, "memset"); chkb("memset", p, bytes, WR); memset(p, v, bytes); return 0; }
int qrd_h2d(void* s, void* d, const void* h, size_t bytes) { op_begin(s, "h2d"); chkb("h2d", d, bytes, WR); memcpy(d, h, bytes); return 0; }
int qrd_d2h(void* s, void* h, const void* d, size_t bytes) { op_begin(s, "d2h"); chkb("d2h", d, bytes, RD); memcpy(h, d, bytes); return 0; }
int qrd_d2d(void* s, void* dst, const void* src, size_t bytes)
{ op_begin(s, "d2d"); chkb("d2d dst", dst, bytes, WR); chkb("d2d src", src, bytes, RD); memmove(dst, src, bytes); return 0; }
int qrd_h2d_2d(void* s, void* d, size_t dp, const void* h, size_t hp, size_t w, size_t hgt)
{
    op_begin(s, "h2d_2d");
    if (w && hgt) { if (dp < w) die("h2d_2d pitch", d, w); chk_bytes("h2d_2d", d, w, dp, (long) hgt, WR); }
    for (size_t r = 0; r < hgt; ++r) memcpy((char*) d + r * dp, (const char*) h + r * hp, w);
    return 0;
}
int qrd_d2h_2d(void* s, void* h, size_t hp, const void* d, size_t dp, size_t w, size_t hgt)
{
    op_begin(s, "d2h_2d");
    if (w && hgt) { if (dp < w) die("d2h_2d pitch", d, w); chk_bytes("d2h_2d", d, w, dp, (long) hgt, RD); }
    for (size_t r = 0; r < hgt; ++r) memcpy((char*) h + r * hp, (const char*) d + r * dp, w);
    return 0;
}

static int stream_new(void** s, int cus)
{
    stub_stream* x = calloc(1, sizeof *x);
    if (!x) return 2;
    pthread_mutex_lock(&g_mu);
    int k = 1;
    while (k < MAXS && g_slot[k].live) ++k;
    if (k == MAXS) { fprintf(stderr, "qrd_stub: more than %d live streams\n", MAXS - 1); abort(); }
    if (k >= g_hi) g_hi = k + 1;
    g_slot[k].live = 1; g_slot[k].cus = cus; g_slot[k].dev = t_dev;
    memset(&g_slot[k].clk, 0, sizeof g_slot[k].clk);
    g_slot[k].clk.c[k] = g_slot[k].tick;          /* (a slot used before: the new stream is behind what the old one ran, nothing else) */
    pthread_mutex_unlock(&g_mu);
    x->cus = cus; x->slot = k;
    *s = x;
    return 0;
}
int qrd_stream_create(void** s, int hp) { (void) hp; return stream_new(s, 256); }
int qrd_stream_create_cumask(void** s, int first, int count) { (void) first; return stream_new(s, count); }
int qrd_stream_destroy(void* s)
{
    if (s) { pthread_mutex_lock(&g_mu); g_slot[slot_of(s)].live = 0; pthread_mutex_unlock(&g_mu); }
    free(s);
    return 0;
}
int qrd_stream_cus(void* s) { return s ? ((stub_stream*) s)->cus : 256; }
int qrd_stream_cus_coresident(void* s) { const int c = qrd_stream_cus(s); return c >= 32 ? c / 32 * 32 : c / 2; }
int qrd_stream_sync(void* s)
{
    pthread_mutex_lock(&g_mu);
    vc_join(&t_host, &g_slot[slot_of(s)].clk);
    pthread_mutex_unlock(&g_mu);
    return 0;
}
int qrd_device_sync(void) { pthread_mutex_lock(&g_mu); join_device_locked(); pthread_mutex_unlock(&g_mu); return 0; }
/* graph capture: use_graph excludes look-ahead, so a captured schedule is single-stream and is checked as it is issued */
int qrd_capture_begin(void* s) { (void) s; return 0; }
int qrd_capture_end(void* s, void** exec) { (void) s; *exec = calloc(1, 8); return *exec ? 0 : 2; }
int qrd_graph_launch(void* exec, void* s) { (void) s; return exec ? 0 : 1; }
int qrd_graph_destroy(void* exec) { free(exec); return 0; }
typedef struct stub_event { double tick; int recorded; vclock clk; } stub_event;      /* (tick first: qrd_event_elapsed_ms) */
int qrd_event_create(void** e) { *e = calloc(1, sizeof(stub_event)); return *e ? 0 : 2; }
int qrd_event_create_notiming(void** e) { return qrd_event_create(e); }
int qrd_event_create_timing(void** e) { return qrd_event_create(e); }
int qrd_event_destroy(void* e) { free(e); return 0; }
/* a record stamps the event with a process-wide tick (0.01 "ms" apart, or QRD_STUB_GATHER_MS after a collective: the joint fall-back
 * decision of the pipelined exchange can be driven from a test), so that elapsed times are ordered like the records; for the order
 * model it holds a copy of the stream's clock */
static __thread double g_stub_tick = 0.0, g_stub_after_gather = 0.0;      /* per host thread = per rank */
int qrd_event_record(void* e, void* s)
{
    if (!e) return 1;
    g_stub_tick += 0.01 + g_stub_after_gather;
    g_stub_after_gather = 0.0;
    stub_event* ev = (stub_event*) e;
    ev->tick = g_stub_tick;
    pthread_mutex_lock(&g_mu);
    vc_join(&g_slot[slot_of(s)].clk, &t_host);        /* (a record is queued work too: what the host knows precedes it) */
    ev->clk = g_slot[slot_of(s)].clk;
    ev->recorded = 1;
    pthread_mutex_unlock(&g_mu);
    return 0;
}
int qrd_event_sync(void* e)
{
    if (!e) return 1;
    pthread_mutex_lock(&g_mu);
    if (((stub_event*) e)->recorded) vc_join(&t_host, &((stub_event*) e)->clk);
    pthread_mutex_unlock(&g_mu);
    return 0;
}
/* the waits of the process, in call order: site (function:event-expression, where the caller was built to say so) and a serial number of
 * the call site; QRD_STUB_SKIP_WAIT=k: the k-th one (from 1) returns without joining */
#define MAXW 8192
static struct { const char *func, *expr; int site; } g_wait[MAXW];
static long g_nwait, g_skip_wait = -1;
int qrd_stub_wait_at(void* s, void* e, const char* func, const char* expr, int site)
{
    if (!e) return 1;
    pthread_mutex_lock(&g_mu);
    if (g_skip_wait < 0) { const char* v = getenv("QRD_STUB_SKIP_WAIT"); g_skip_wait = v ? atol(v) : 0; }
    if (g_nwait < MAXW) { g_wait[g_nwait].func = func; g_wait[g_nwait].expr = expr; g_wait[g_nwait].site = site; }
    const long k = ++g_nwait;
    if (k != g_skip_wait && ((stub_event*) e)->recorded) vc_join(&g_slot[slot_of(s)].clk, &((stub_event*) e)->clk);
    pthread_mutex_unlock(&g_mu);
    return 0;
}
int qrd_stream_wait_event(void* s, void* e) { return qrd_stub_wait_at(s, e, NULL, NULL, -1); }
long qrd_stub_wait_count(void) { pthread_mutex_lock(&g_mu); const long n = g_nwait; pthread_mutex_unlock(&g_mu); return n; }
int qrd_stub_wait_site(long k, const char** func, const char** expr, int* site)
{
    if (k < 1 || k > g_nwait || k > MAXW) return 1;
    *func = g_wait[k - 1].func; *expr = g_wait[k - 1].expr; *site = g_wait[k - 1].site;
    return 0;
}
int qrd_event_elapsed_ms(void* a, void* b, float* ms) { if (!a || !b) return 1; *ms = (float) (*(double*) b - *(double*) a); return 0; }
int qrd_device_count(int* n) { const char* e = getenv("QRD_STUB_NDEV"); *n = e ? atoi(e) : 4; return 0; }
int qrd_set_device(int d) { t_dev = d; return 0; }
int qrd_get_device(int* d) { *d = t_dev; return 0; }
int qrd_host_register(void* p, size_t b) { (void) p; (void) b; return 0; }
int qrd_host_unregister(void* p) { (void) p; return 0; }
const char* qrd_error_string(int e) { (void) e; return "stub device layer error"; }
int qrd_device_info(char* name, int len, int* cus, int* khz, size_t* mem)
{
    if (name && len > 0) snprintf(name, (size_t) len, "stub");
    if (cus) *cus = 256;
    if (khz) *khz = 2400000;
    if (mem) *mem = (size_t) 1 << 36;
    return 0;
}
int qrd_probe_mfma_f64(double* o) { o[0] = o[1] = o[2] = 1.0; return 0; }
int qrd_probe_copy(double* g) { *g = 1.0; return 0; }

/* ---- kernel launches: operand checks only.  Tags after qr_device.h: const operands are read, outputs written, in-place operands and a
 *      GEMM's C with beta != 0 read-write, scratch a launch fills and consumes itself (slabs, ws) written ---- */
static void gemm_nn_chk(int M, int N, int K, const double* A, int lda, const double* B, int ldb, double be, double* C, int ldc)
{ chk("gemm_nn A", A, lda, M, K, RD); chk("gemm_nn B", B, ldb, K, N, RD); chk("gemm_nn C", C, ldc, M, N, BETA(be)); }
int qrd_gemm_nn(void* s, int M, int N, int K, double al, const double* A, int lda, const double* B, int ldb, double be, double* C, int ldc)
{ (void) al; op_begin(s, "gemm_nn"); gemm_nn_chk(M, N, K, A, lda, B, ldb, be, C, ldc); return 0; }
int qrd_gemm_nn_update(void* s, int M, int N, int K, double al, const double* A, int lda, const double* B, int ldb, double be, double* C, int ldc)
{ (void) al; op_begin(s, "gemm_nn_update"); gemm_nn_chk(M, N, K, A, lda, B, ldb, be, C, ldc); return 0; }
int qrd_gemm_nn_update2(void* s, int M, int N, int K, double al, const double* A, int lda, const double* B, int ldb, double be, double* C, int ldc)
{ (void) al; op_begin(s, "gemm_nn_update2"); gemm_nn_chk(M, N, K, A, lda, B, ldb, be, C, ldc); return 0; }
static void gemm_tn_chk(int M, int N, int K, const double* A, int lda, const double* B, int ldb, double be, double* C, int ldc,
                        double* slabs, size_t cap, const double* Tm, int ldt)
{
    chk("gemm_tn A", A, lda, K, M, RD); chk("gemm_tn B", B, ldb, K, N, RD); chk("gemm_tn C", C, ldc, M, N, BETA(be));
    if (slabs) chkb("gemm_tn slabs", slabs, cap * sizeof(double), WR);
    if (Tm) chk("gemm_tn T", Tm, ldt, M, M, RD);
}
int qrd_gemm_tn(void* s, int M, int N, int K, double al, const double* A, int lda, const double* B, int ldb, double be, double* C, int ldc,
                double* slabs, size_t cap, const double* Tm, int ldt)
{ (void) al; op_begin(s, "gemm_tn"); gemm_tn_chk(M, N, K, A, lda, B, ldb, be, C, ldc, slabs, cap, Tm, ldt); return 0; }
int qrd_gemm_tn_update(void* s, int M, int N, int K, double al, const double* A, int lda, const double* B, int ldb, double be, double* C, int ldc,
                       double* slabs, size_t cap)
{ (void) al; op_begin(s, "gemm_tn_update"); gemm_tn_chk(M, N, K, A, lda, B, ldb, be, C, ldc, slabs, cap, NULL, 0); return 0; }
int qrd_gemm_tn_update_wide(void* s, int M, int N, int K, double al, const double* A, int lda, const double* B, int ldb, double be, double* C, int ldc,
                            double* slabs, size_t cap)
{ (void) al; op_begin(s, "gemm_tn_update_wide"); gemm_tn_chk(M, N, K, A, lda, B, ldb, be, C, ldc, slabs, cap, NULL, 0); return 0; }
int qrd_gemm_tn_dual(void* s, int N1, int N2, int K, const double* A, int lda, const double* B1, int ldb1, const double* B2, int ldb2,
                     const double* Tm, int ldt, double* W, int ldw, double* G2, int ldg, double* slabs, size_t cap)
{
    op_begin(s, "gemm_tn_dual");
    chk("tn_dual A", A, lda, K, 32, RD);
    if (N1 > 0) { chk("tn_dual B1", B1, ldb1, K, N1, RD); chk("tn_dual W", W, ldw, 32, N1, WR); }
    if (N2 > 0) { chk("tn_dual B2", B2, ldb2, K, N2, RD); chk("tn_dual G2", G2, ldg, N2, 32, WR); }
    chk("tn_dual T", Tm, ldt, 32, 32, RD);
    chkb("tn_dual slabs", slabs, cap * sizeof(double), WR);
    return (K & 64) ? -7 : 0;          /* both outcomes of the fused launch are exercised */
}
int qrd_gemm_nt_ok(int M, int N, int K, const double* A, int lda, const double* Bt, int ldbt, const double* C, int ldc)
{ (void) A; (void) Bt; (void) C; (void) lda; (void) ldbt; (void) ldc; return M % 128 == 0 && N % 128 == 0 && K % 16 == 0; }
int qrd_gemm_nt4_ok(int M, int N, int K, const double* A, int lda, const double* Bt, int ldbt, const double* C, int ldc)
{ (void) A; (void) Bt; (void) C; (void) ldbt; (void) ldc; return M >= 128 && N >= 64 && N % 64 == 0 && K >= 32 && K % 16 == 0 && (M % 128 == 0 || (M % 2 == 0 && (M + 127) / 128 * 128 <= lda)); }
int qrd_gemm_nt(void* s, int M, int N, int K, int sign, const double* A, int lda, const double* Bt, int ldbt, double* C, int ldc, int gm,
                unsigned long long* st)
{
    (void) sign; (void) gm; (void) st;
    op_begin(s, "gemm_nt");
    chk("gemm_nt A", A, lda, M, K, RD); chk("gemm_nt Bt", Bt, ldbt, N, K, RD); chk("gemm_nt C", C, ldc, M, N, RW);      /* C += sign A Bt^T */
    return 0;
}
/* a leaf / panel factored in place: P read-write, tau, the w x w T block and V out */
static void leaf_chk(const char* w, double* P, int ld, int mk, int wd, double* tau, double* T, int ldt, double* Vw, int ldv)
{ chk(w, P, ld, mk, wd, RW); chk(w, tau, wd, wd, 1, WR); chk(w, T, ldt, wd, wd, WR); chk(w, Vw, ldv, mk, wd, WR); }
size_t qrd_panel_ws_size(int m) { return (size_t) 80 * (size_t) (m > 0 ? m : 1) + 65536; }
int qrd_panel_tsqr(void* s, double* P, int ld, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv, double* ws, int mcap)
{
    op_begin(s, "panel_tsqr");
    leaf_chk("panel_tsqr", P, ld, mk, w, tau, T, ldt, Vw, ldv); chkb("panel ws", ws, sizeof(double) * qrd_panel_ws_size(mcap), WR);
    return 0;
}
/* (slabs: gram_nslab > 0 partial Gram matrices of this leaf are read there, left by the previous leaf's qrd_leaf_update_gram) */
static void cholqr_chk(double* P, int ld, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv, double* ws, int mcap,
                       double* cws, double* slabs, size_t cap, int gn)
{
    leaf_chk("panel_cholqr", P, ld, mk, w, tau, T, ldt, Vw, ldv); chkb("panel ws", ws, sizeof(double) * qrd_panel_ws_size(mcap), WR);
    chkb("cholqr ws", cws, sizeof(double) * QRD_CHOLQR_WS, WR); chkb("cholqr slabs", slabs, cap * sizeof(double), gn > 0 ? RW : WR);
}
int qrd_panel_cholqr(void* s, double* P, int ld, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv, double* ws, int mcap,
                     double* cws, double* slabs, size_t cap, int gn)
{
    op_begin(s, "panel_cholqr");
    cholqr_chk(P, ld, mk, w, tau, T, ldt, Vw, ldv, ws, mcap, cws, slabs, cap, gn);
    return 0;
}
int qrd_panel_cholqr_ep(void* s, double* P, int ld, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv, double* ws, int mcap,
                        double* cws, double* slabs, size_t cap, int gn, int N1, const double* B1, int ldb1, int N2, const double* B2, int ldb2,
                        double* W, int ldw, double* G2, int ldg, double* eps, size_t ecap, int* did)
{
    op_begin(s, "panel_cholqr_ep");
    cholqr_chk(P, ld, mk, w, tau, T, ldt, Vw, ldv, ws, mcap, cws, slabs, cap, gn);
    if (N1 > 0) { chk("ep B1", B1, ldb1, mk, N1, RD); chk("ep W", W, ldw, 32, N1, WR); }
    if (N2 > 0) { chk("ep B2", B2, ldb2, mk, N2, RD); chk("ep G2", G2, ldg, N2, 32, WR); }
    chkb("ep slabs", eps, ecap * sizeof(double), WR);
    if (ecap < (size_t) 32 * (size_t) (N1 + N2)) { fprintf(stderr, "qrd_stub: early-product slab buffer too small\n"); abort(); }
    *did = (mk & 64) ? 0 : 1;          /* both outcomes are exercised */
    return 0;
}
/* the full-width tall panel: same shape rule as the real layer; panels whose height has bit 12 set are REFUSED by the (stub) guard, so
 * that the host's fall-back to the leaf chain on the untouched panel is exercised as well.
 * (ws keeps R and the shifted Gram matrix for restore_r / r_block / retry: written here, read there; status[1] is a sticky count) */
size_t qrd_panel_cqr_ws_doubles(void) { return 12 * 128 * 128 + 128 + 64 + 256 * 36 * 256; }
static int cqr_q_chk(const char* name, void* s, double* A, int lda, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv, double* ws,
                     int* status, double* Qb, int ldq, unsigned* hflag, unsigned seq)
{
    if (!qrd_panel_cqr_ok(mk, w)) return -7;
    op_begin(s, name);
    leaf_chk("panel_cqr", A, lda, mk, w, tau, T, ldt, Vw, ldv);
    if (Qb) chk("panel_cqr Q", Qb, ldq, mk, w, WR);
    chkb("cqr ws", ws, sizeof(double) * qrd_panel_cqr_ws_doubles(), WR); chkb("cqr status", status, 4 * sizeof(int), RW);
    status[0] = 0;
    if (mk & 4096) { status[0] = 1; if (!hflag) status[1] += 1; }
    if (hflag) __atomic_store_n(hflag, 2u * seq + (unsigned) status[0], __ATOMIC_RELEASE);
    return 0;
}
int qrd_panel_cqr_q(void* s, double* A, int lda, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv, double* ws, int* status,
                    double* Qb, int ldq, unsigned* hflag, unsigned seq)
{ return cqr_q_chk("panel_cqr_q", s, A, lda, mk, w, tau, T, ldt, Vw, ldv, ws, status, Qb, ldq, hflag, seq); }
int qrd_panel_cqr_p(void* s, double* A, int lda, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv, double* ws, int* status,
                    double* Qb, int ldq, unsigned* hflag, unsigned seq, int park)
{
    if (park && (!Qb || Qb == A)) return -7;
    return cqr_q_chk("panel_cqr_p", s, A, lda, mk, w, tau, T, ldt, Vw, ldv, ws, status, Qb, ldq, hflag, seq);
}
/* the stub's guard accepts a retried panel unless bit 7 of its height is set too (65408 = 0xFF80: refused twice; 61440 + ...: see host_sanitize.c) */
int qrd_panel_cqr_retry(void* s, double* A, int lda, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv, double* ws, int* status,
                        double* Qb, int ldq, unsigned* hflag, unsigned seq, int park)
{
    (void) park;
    if (!Qb || Qb == A || Qb == Vw) return -7;
    op_begin(s, "panel_cqr_retry");
    leaf_chk("cqr retry", A, lda, mk, w, tau, T, ldt, Vw, ldv);
    chk("cqr retry Q", Qb, ldq, mk, w, WR);
    chkb("cqr ws", ws, sizeof(double) * qrd_panel_cqr_ws_doubles(), RW); chkb("cqr status", status, 4 * sizeof(int), RW);
    status[0] = (mk & 128) ? 1 : 0;
    if (hflag) __atomic_store_n(hflag, 2u * seq + (unsigned) status[0], __ATOMIC_RELEASE);
    return 0;
}
int qrd_panel_cqr_restore_r(void* s, double* A, int lda, int w, const double* ws, const int* status)
{
    op_begin(s, "panel_cqr_restore_r");
    chk("cqr restore A", A, lda, w, w, WR); chkb("cqr ws", ws, sizeof(double) * qrd_panel_cqr_ws_doubles(), RD); chkb("cqr status", status, 4 * sizeof(int), RD);
    return 0;
}
int qrd_panel_cqr_r_block(void* s, const double* ws, int w, double* D, int ldd)
{ op_begin(s, "panel_cqr_r_block"); chk("cqr r block", D, ldd, w, w, WR); chkb("cqr ws", ws, sizeof(double) * qrd_panel_cqr_ws_doubles(), RD); return 0; }
int qrd_panel_cqr(void* s, double* A, int lda, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv, double* ws, int* status)
{
    return cqr_q_chk("panel_cqr", s, A, lda, mk, w, tau, T, ldt, Vw, ldv, ws, status, NULL, 0, NULL, 0u);
}
int qrd_host_word_alloc(unsigned** host, unsigned** dev)
{
    unsigned* w = (unsigned*) calloc(16, sizeof(unsigned));
    if (!w) return 2;
    *host = w; *dev = w;
    return 0;
}
int qrd_host_word_free(unsigned* host) { free(host); return 0; }
int qrd_trsm_gt(void* s, int kw, int nc, const double* G, int ldg, const double* T, int ldt, const double* Y, int ldy, double* W, int ldw)
{
    if (kw < 32 || kw > 256 || kw % 32 || nc < 16 || nc % 16) return -7;
    op_begin(s, "trsm_gt");
    chk("trsm G", G, ldg, kw, kw, RD); chk("trsm T", T, ldt, kw, kw, RD); chk("trsm Y", Y, ldy, kw, nc, RD); chk("trsm W", W, ldw, kw, nc, WR);
    return 0;
}
int qrd_transpose(void* s, int rows, int cols, const double* S, int lds, double* D, int ldd)
{
    op_begin(s, "transpose");
    chk("transpose S", S, lds, rows, cols, RD); chk("transpose D", D, ldd, cols, rows, WR);
    return 0;
}
int qrd_panel_cqr_init(void) { return 0; }
int qrd_panel_cqr_ok(int mk, int w) { return w >= 32 && w <= 128 && w % 32 == 0 && mk >= 2 * w; }
double* qrd_panel_cqr_g1(double* ws) { return ws; }
double* qrd_panel_cqr_g2(double* ws) { return ws + 128 * 128; }
int qrd_panel_cqr_stage1(void* s, const double* A, int lda, int mk, int w, double* Vw, int ldv, double* ws, int* status)
{
    op_begin(s, "panel_cqr_stage1");
    chk("cqr stage1 A", A, lda, mk, w, RD); chk("cqr stage1 Vw", Vw, ldv, mk, w, WR);
    chkb("cqr ws", ws, sizeof(double) * qrd_panel_cqr_ws_doubles(), RW); chkb("cqr status", status, 4 * sizeof(int), RW);
    if (mk & 4096) status[0] = 1;
    return 0;
}
int qrd_panel_cqr_stage2(void* s, double* A, int lda, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv, double* ws, int* status)
{
    op_begin(s, "panel_cqr_stage2");
    leaf_chk("cqr stage2", A, lda, mk, w, tau, T, ldt, Vw, ldv);
    chkb("cqr ws", ws, sizeof(double) * qrd_panel_cqr_ws_doubles(), RW); chkb("cqr status", status, 4 * sizeof(int), RW);
    return 0;
}
size_t qrd_panel_fused_ws_doubles(void) { return 700000; }
/* same shape rules as the real launch layer (whole leaves, <= 256 columns, <= 32 x 256 rows, rows a multiple of 4, aligned operands);
 * heights with bit 9 set are declined so that both routes of factor_panel are exercised */
int qrd_panel_fused_merges_t(int wh, int with_gram) { return wh == 64 && with_gram; }
int qrd_panel_fused_ok(void* s, const double* A, int lda, int mk, int wh, const double* Vw, int ldv)
{
    (void) s;
    if (wh < 32 || wh > 256 || wh % 32 || mk < wh || mk % 4 || mk > 8192 || (mk & 512)) return 0;
    return !(((uintptr_t) A & 15) || ((uintptr_t) Vw & 15) || lda % 2 || ldv % 2);
}
int qrd_panel_fused(void* s, double* A, int lda, int mk, int wh, double* tau, double* T, int ldt, double* Vw, int ldv, double* G, int ldg,
                    double* ws, unsigned* epoch, int* status)
{
    if (!qrd_panel_fused_ok(s, A, lda, mk, wh, Vw, ldv)) return -7;
    op_begin(s, "panel_fused");
    leaf_chk("panel_fused", A, lda, mk, wh, tau, T, ldt, Vw, ldv);
    if (G) chk("panel_fused G", G, ldg, wh, wh, WR);       /* NULL: the caller forms V^T V itself */
    chkb("panel_fused ws", ws, sizeof(double) * qrd_panel_fused_ws_doubles(), WR);
    chkb("panel_fused status", status, 4 * sizeof(int), RW);
    *epoch += 1024u;
    /* QRD_STUB_STALL_ONCE=1 (host_sanitize.c): the next one-launch panel reports a timed-out hand-off, once -- the host-pointer entry
     * points must notice (QR_E_STALL at their plan sync) and factor again with the route off */
    if (getenv("QRD_STUB_STALL_ONCE")) { status[1] = 1; unsetenv("QRD_STUB_STALL_ONCE"); ++g_stub_stalls; }
    return 0;
}
int qrd_panel_fused_rows(void* s, double* A, int lda, int mk, int wh, double* tau, double* T, int ldt, double* Vw, int ldv, double* G, int ldg,
                         double* ws, unsigned* epoch, int* status, int rows)
{ (void) rows; return qrd_panel_fused(s, A, lda, mk, wh, tau, T, ldt, Vw, ldv, G, ldg, ws, epoch, status); }
long qrd_stub_stalls(void) { return g_stub_stalls; }
int qrd_slab_reduce(void* s, int M, int N, int ns, const double* slabs, int lds, size_t stride, double* out, int ldo)
{
    (void) ns; (void) stride;
    op_begin(s, "slab_reduce");
    chk("slab_reduce in", slabs, lds, M, N, RD); chk("slab_reduce out", out, ldo, M, N, WR);
    return 0;
}
int qrd_leaf_update_gram(void* s, int mk, int N, const double* V, int ldv, const double* W, double* C, int ldc, double* gs, size_t cap, int gy,
                         int* nslab)
{
    (void) gy;
    if (mk < 1024) return -7;
    op_begin(s, "leaf_update_gram");
    chk("lug V", V, ldv, mk, 32, RD); chk("lug W", W, 32, 32, N, RD); chk("lug C", C, ldc, mk, N, RW);
    if (gs) chkb("lug slabs", gs, cap * sizeof(double), WR);
    if (nslab) *nslab = gs ? 8 : 0;
    return 0;
}
/* (T: the leaves' diagonal blocks are read, the merged triangle written; X is the tree's scratch) */
int qrd_larft(void* s, int nbp, int ib, const double* G, int ldg, const double* tau, double* T, int ldt, double* Tt, int bd, double* X, int ldx)
{
    (void) ib; (void) bd;
    op_begin(s, "larft");
    chk("larft G", G, ldg, nbp, nbp, RD); chk("larft tau", tau, nbp, nbp, 1, RD); chk("larft T", T, ldt, nbp, nbp, RW); chk("larft X", X, ldx, nbp, nbp, WR);
    if (Tt) chk("larft Tt", Tt, ldt, nbp, nbp, WR);
    return 0;
}
/* The pure DATA MOVERS move data (still no arithmetic: the factorisations above them are no-ops on the values), so that a test can
 * follow a tagged R factor through pack -> exchange -> stack -> extract (tests/test_tsqr_cplan_gloo.py: the C qr_tsqr_plan over gloo).
 * Every copy_block is also logged (source, destination, shape): the stacking order of the gathered factors is read off the log. */
#define STUB_COPYLOG 256
static __thread struct { const double* S; double* D; int lds, ldd, r, c; } t_copylog[STUB_COPYLOG];
static __thread long t_ncopy = 0;
long qrd_stub_copy_count(void) { return t_ncopy; }
int qrd_stub_copy_entry(long i, const double** S, double** D, int* lds, int* ldd, int* r, int* c)
{
    if (i < 0 || i >= t_ncopy || t_ncopy - i > STUB_COPYLOG) return 1;
    *S = t_copylog[i % STUB_COPYLOG].S; *D = t_copylog[i % STUB_COPYLOG].D; *lds = t_copylog[i % STUB_COPYLOG].lds;
    *ldd = t_copylog[i % STUB_COPYLOG].ldd; *r = t_copylog[i % STUB_COPYLOG].r; *c = t_copylog[i % STUB_COPYLOG].c;
    return 0;
}
int qrd_zero_block(void* s, double* A, int ld, int r, int c)
{
    op_begin(s, "zero_block"); chk("zero_block", A, ld, r, c, WR);
    for (int j = 0; j < c; ++j) memset(A + (size_t) j * ld, 0, sizeof(double) * (size_t) r);
    return 0;
}
int qrd_extract_v(void* s, const double* P, int ld, int mk, int w, double* V, int ldv)
{ op_begin(s, "extract_v"); chk("extract_v P", P, ld, mk, w, RD); chk("extract_v V", V, ldv, mk, w, WR); return 0; }
int qrd_extract_r(void* s, const double* A, int lda, int m, int n, double* R, int ldr, int rr)
{
    op_begin(s, "extract_r"); chk("extract_r A", A, lda, m, n, RD); chk("extract_r R", R, ldr, rr, n, WR);
    for (int c = 0; c < n; ++c)
        for (int i = 0; i < rr; ++i) R[(size_t) c * ldr + i] = (i <= c && i < m) ? A[(size_t) c * lda + i] : 0.0;
    return 0;
}
int qrd_extract_r_block(void* s, const double* A, int lda, int k, int w, double* R, int ldr, int rr)
{
    op_begin(s, "extract_r_block"); chk("extract_r_block A", A + (size_t) k * lda, lda, k + w, w, RD); chk("extract_r_block R", R, ldr, rr, w, WR);
    for (int j = 0; j < w; ++j)
        for (int i = 0; i < rr; ++i) R[(size_t) j * ldr + i] = (i <= k + j) ? A[(size_t) (k + j) * lda + i] : 0.0;
    return 0;
}
int qrd_set_identity(void* s, double* C, int ld, int r, int c, int ro)
{
    op_begin(s, "set_identity"); chk("set_identity", C, ld, r, c, WR);
    for (int j = 0; j < c; ++j)
        for (int i = 0; i < r; ++i) C[(size_t) j * ld + i] = (i + ro == j) ? 1.0 : 0.0;
    return 0;
}
int qrd_copy_blocks(void* s, const double* S, int lds, size_t ss, double* D, int ldd, size_t ds, int r, int c, int batch)
{
    op_begin(s, "copy_blocks");
    for (int q = 0; q < batch; ++q) {
        chk("copy_blocks S", S + q * ss, lds, r, c, RD); chk("copy_blocks D", D + q * ds, ldd, r, c, WR);
        for (int j = 0; j < c; ++j) memmove(D + q * ds + (size_t) j * ldd, S + q * ss + (size_t) j * lds, sizeof(double) * (size_t) r);
    }
    return 0;
}
int qrd_copy_block(void* s, const double* S, int lds, double* D, int ldd, int r, int c)
{
    op_begin(s, "copy_block"); chk("copy_block S", S, lds, r, c, RD); chk("copy_block D", D, ldd, r, c, WR);
    for (int j = 0; j < c; ++j) memmove(D + (size_t) j * ldd, S + (size_t) j * lds, sizeof(double) * (size_t) r);
    t_copylog[t_ncopy % STUB_COPYLOG].S = S; t_copylog[t_ncopy % STUB_COPYLOG].D = D; t_copylog[t_ncopy % STUB_COPYLOG].lds = lds;
    t_copylog[t_ncopy % STUB_COPYLOG].ldd = ldd; t_copylog[t_ncopy % STUB_COPYLOG].r = r; t_copylog[t_ncopy % STUB_COPYLOG].c = c;
    ++t_ncopy;
    return 0;
}
int qrd_fill_uniform(void* s, double* A, int ld, long long rows, int cols, long long ro, long long tr, unsigned long long seed)
{ (void) ro; (void) tr; (void) seed; op_begin(s, "fill_uniform"); chk("fill", A, ld, (long) rows, cols, WR); return 0; }
double qrd_hash_uniform_host(unsigned long long seed, unsigned long long idx) { (void) seed; (void) idx; return 0.5; }
int qrd_diff_norm(void* s, const double* X, int ldx, const double* Y, int ldy, long long rows, int cols, long long ro, long long tr,
                  unsigned long long seed, int si, double* out)
{
    (void) ro; (void) tr; (void) seed; (void) si;
    op_begin(s, "diff_norm");
    chk("diffnorm X", X, ldx, (long) rows, cols, RD); if (Y) chk("diffnorm Y", Y, ldy, (long) rows, cols, RD);
    out[0] = 0.0; out[1] = 1.0;
    return 0;
}

size_t qrd_legacy_ws_size(int m, int PR, int PC) { return (size_t) (1 + (m - PR) / (PR - PC)) * 2 * (size_t) PC * 64; }
int qrd_legacy_shape_ok(int m, int n, int PR, int PC)
{ return PR >= 2 && PR <= 64 && (PC == 2 || PC == 4 || PC == 8 || PC == 16) && PC < PR && m >= PR && n >= PC && n % PC == 0 && n <= m && (m - PR) % (PR - PC) == 0; }
int qrd_legacy_panel(void* s, double* A, int m, int n, int PR, int PC, int rp, int pc, int pcCount, double* tau, double* wy)
{
    (void) pc;
    if (pcCount < 0 || pcCount >= n / PC) { fprintf(stderr, "qrd_stub: legacy panel index out of range\n"); abort(); }
    op_begin(s, "legacy_panel");
    chk("legacy A", A, m, m, n, RW);
    chkb("legacy tau all", tau, sizeof(double) * (size_t) rp * (size_t) (n / PC) * PC, RW); chkb("legacy wy", wy, sizeof(double) * qrd_legacy_ws_size(m, PR, PC), WR);
    return 0;
}
int qrd_legacy_formq(void* s, const double* A, const double* tau, int m, int n, int PR, int PC, int rp, double* Q)
{
    (void) PR;
    op_begin(s, "legacy_formq");
    chk("legacy A", A, m, m, n, RD); chkb("legacy tau", tau, sizeof(double) * (size_t) rp * (size_t) (n / PC) * PC, RD); chk("legacy Q", Q, m, m, m, WR);
    return 0;
}

/* ---- "RCCL": a thread-level all-gather (one thread per device, the way qr_thin_mgpu drives it) ---- */
typedef struct stub_world { int n; pthread_barrier_t bar; const double* send[64]; int slot[64]; } stub_world;
typedef struct stub_comm { stub_world* w; int rank; } stub_comm;
int qrd_comm_init_all(void** comms, int n, const int* devs)
{
    (void) devs;
    stub_world* w = calloc(1, sizeof *w);
    if (!w) return QRD_E_RCCL;
    w->n = n;
    pthread_barrier_init(&w->bar, NULL, (unsigned) n);
    for (int i = 0; i < n; ++i) { stub_comm* c = calloc(1, sizeof *c); c->w = w; c->rank = i; comms[i] = c; }
    return 0;
}
int qrd_comm_unique_id(void* id) { memset(id, 7, QRD_UNIQUE_ID_BYTES); return 0; }
int qrd_comm_init_rank(void** comm, int n, const void* id, int rank) { (void) comm; (void) n; (void) id; (void) rank; return QRD_E_NORCCL; }
int qrd_comm_count(void* comm, int* n) { *n = ((stub_comm*) comm)->w->n; return 0; }
const char* qrd_rccl_error_string(int r) { (void) r; return "stub rccl error"; }
int qrd_comm_destroy(void* comm)
{
    stub_comm* c = (stub_comm*) comm;
    if (!c) return 0;
    if (c->rank == 0) { pthread_barrier_destroy(&c->w->bar); free(c->w); }
    free(c);
    return 0;
}
/* send is read and recv written on the rank's stream; between the two barriers (no rank issues anything there) every rank's stream joins
 * the clocks all the ranks' streams had at their collective: what follows it on any rank is ordered after what preceded it on every rank */
int qrd_allgather_f64(void* comm, void* stream, const double* send, double* recv, size_t count)
{
    stub_comm* c = (stub_comm*) comm;
    op_begin(stream, "allgather");
    chkb("allgather send", send, count * sizeof(double), RD);
    chkb("allgather recv", recv, count * sizeof(double) * (size_t) c->w->n, WR);
    c->w->send[c->rank] = send;
    c->w->slot[c->rank] = slot_of(stream);
    pthread_barrier_wait(&c->w->bar);
    for (int q = 0; q < c->w->n; ++q) memcpy(recv + (size_t) q * count, c->w->send[q], count * sizeof(double));
    {
        vclock all;
        memset(&all, 0, sizeof all);
        pthread_mutex_lock(&g_mu);
        for (int q = 0; q < c->w->n; ++q) vc_join(&all, &g_slot[c->w->slot[q]].clk);
        pthread_mutex_unlock(&g_mu);
        pthread_barrier_wait(&c->w->bar);
        pthread_mutex_lock(&g_mu);
        vc_join(&g_slot[slot_of(stream)].clk, &all);
        pthread_mutex_unlock(&g_mu);
    }
    pthread_barrier_wait(&c->w->bar);
    { const char* e = getenv("QRD_STUB_GATHER_MS"); if (e) g_stub_after_gather = atof(e); }
    return 0;
}

/* the device layer of the per-interface host units (least squares down to batched Levenberg-Marquardt): same helpers, a file of its own */
#include "qrd_stub_units.c"
