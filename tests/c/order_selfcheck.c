/* order_selfcheck.c -- TEST-ONLY proof that the stream-order model of the stub device layer (qrd_stub.c) can fail: direct qrd_* calls,
 * no host layer, exact report counts in count mode (`make -C cuda-qr_amd order`; tests/test_schedule_order.py runs it). */
#define _POSIX_C_SOURCE 200809L
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../cuda-qr_amd/csrc/qr_device.h"

long qrd_stub_order_reports(void);

enum { LD = 64, ROWS = 48, COLS = 40 };
static double *A, *D1, *D2;          /* the block under test; one destination per reading stream */
static void *s1, *s2, *s3, *e1, *e2;
static int g_bad;

static void wr(void* s, int c0, int nc) { qrd_zero_block(s, A + (size_t) c0 * LD, LD, ROWS, nc); }
static void rd(void* s, double* D, int c0, int nc) { qrd_copy_block(s, A + (size_t) c0 * LD, LD, D, LD, ROWS, nc); }

static void begin(void)
{
    qrd_malloc((void**) &A, sizeof(double) * LD * COLS);
    qrd_malloc((void**) &D1, sizeof(double) * LD * COLS);
    qrd_malloc((void**) &D2, sizeof(double) * LD * COLS);
    qrd_stream_create(&s1, 0); qrd_stream_create_cumask(&s2, 0, 32); qrd_stream_create_cumask(&s3, 32, 224);
    qrd_event_create(&e1); qrd_event_create(&e2);
}
static void end(const char* name, long before, long expect)
{
    const long got = qrd_stub_order_reports() - before;
    printf("%-72s %ld report%s (expected %ld)%s\n", name, got, got == 1 ? "" : "s", expect, got == expect ? "" : "   <-- WRONG");
    if (got != expect) g_bad = 1;
    qrd_device_sync();
    qrd_stream_destroy(s1); qrd_stream_destroy(s2); qrd_stream_destroy(s3);
    qrd_event_destroy(e1); qrd_event_destroy(e2);
    qrd_free(A); qrd_free(D1); qrd_free(D2);
}
static void* other_thread(void* arg) { (void) arg; rd(s2, D2, 0, 8); return NULL; }

int main(void)
{
    setenv("QRD_STUB_ORDER", "count", 1);
    long b;
    begin(); b = qrd_stub_order_reports();
    wr(s1, 0, 8); rd(s2, D2, 0, 8);
    end("write on s1, read of the same block on s2, no wait", b, 1);

    begin(); b = qrd_stub_order_reports();
    wr(s1, 0, 8); qrd_event_record(e1, s1); qrd_stream_wait_event(s2, e1); rd(s2, D2, 0, 8);
    end("write on s1, record, wait, read on s2", b, 0);

    begin(); b = qrd_stub_order_reports();
    rd(s1, D1, 0, 8); wr(s2, 0, 8);
    end("read on s1, write on s2, no wait", b, 1);

    begin(); b = qrd_stub_order_reports();
    wr(s1, 0, 8); wr(s2, 0, 8);
    end("write on s1, write on s2, no wait", b, 1);

    begin(); b = qrd_stub_order_reports();
    rd(s1, D1, 0, 8); rd(s2, D2, 0, 8);
    end("two reads", b, 0);

    begin(); b = qrd_stub_order_reports();
    wr(s1, 0, 8); wr(s2, 8, 8); wr(s3, 16, 24);
    end("disjoint column ranges of one allocation written concurrently", b, 0);

    begin(); b = qrd_stub_order_reports();
    wr(s1, 0, 8); wr(s2, 7, 8);
    end("the same ranges shifted to overlap by one column", b, 1);

    begin(); b = qrd_stub_order_reports();
    /* view 1: ld 10, 3 x 3 at element 0 -> {0,1,2, 10,11,12, 20,21,22};  view 2: ld 7, 2 x 2 at element 5 -> {5,6, 12,13}: element 12 only */
    qrd_zero_block(s1, A, 10, 3, 3); qrd_zero_block(s2, A + 5, 7, 2, 2);
    /* ... and moved up by one element -> {6,7, 13,14}: nothing shared, silent */
    qrd_zero_block(s3, A + 6 + 100, 7, 2, 2); qrd_zero_block(s2, A + 100, 10, 3, 3);
    end("two views of different ld that share exactly one element", b, 1);

    begin(); b = qrd_stub_order_reports();
    wr(s1, 0, 8); qrd_event_record(e1, s1); qrd_stream_wait_event(s3, e1); qrd_event_record(e2, s3); qrd_stream_wait_event(s2, e2); rd(s2, D2, 0, 8);
    end("order established transitively through a third stream", b, 0);

    begin(); b = qrd_stub_order_reports();
    wr(s1, 0, 8); qrd_event_record(e1, s1); qrd_stream_wait_event(s2, e1); wr(s1, 0, 8); qrd_event_record(e1, s1); rd(s2, D2, 0, 8);
    end("a wait issued before the event's second record orders up to the first", b, 1);

    begin(); b = qrd_stub_order_reports();
    wr(s1, 0, 8); qrd_stream_sync(s1); rd(s2, D2, 0, 8);
    end("stream_sync(s1) on the host, then a launch on s2", b, 0);

    begin(); b = qrd_stub_order_reports();
    wr(s1, 0, 8); qrd_stream_sync(s1);
    { pthread_t t; pthread_create(&t, NULL, other_thread, NULL); pthread_join(t, NULL); }
    end("the same launch from another host thread that did not sync", b, 1);

    begin(); b = qrd_stub_order_reports();
    wr(s1, 0, 8); qrd_stream_wait_event(s2, e1); rd(s2, D2, 0, 8);
    end("a wait on a never-recorded event orders nothing", b, 1);

    begin(); b = qrd_stub_order_reports();
    wr(s1, 0, 16); wr(s3, 16, 8); qrd_device_sync(); rd(s2, D2, 0, 24); qrd_device_sync(); wr(s3, 0, 24);
    end("after device_sync everything before it is ordered", b, 0);

    if (g_bad) { fprintf(stderr, "order self-check FAILED\n"); return 1; }
    printf("order self-check ok\n");
    return 0;
}
