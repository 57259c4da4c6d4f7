/* stage_sanitize.c -- TEST-ONLY driver of the staging unit of the batched host-pointer twins (cuda-qr_amd/csrc/qr_stage.c) over the stub
 * device layer (tests/c/qrd_stub.c: "device memory" is host memory, and every copy and clear aborts unless its block lies inside a live
 * allocation).  Built and run by `make asan` / `make tsan` in cuda-qr_amd.  Checks the carve (ascending, 8-byte aligned, packed, the
 * last block inside the allocation), the round trip of every kind of block, the error path, a failed open and that nothing leaks. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/mi355x_qr.h"
#include "../csrc/qr_stage.h"

long qrd_stub_launches(void);
int qrd_stub_live_allocations(void);

#define FAIL(code, ...) do { fprintf(stderr, "stage_sanitize: " __VA_ARGS__); fprintf(stderr, "\n"); return code; } while (0)

enum { NA = 5, NB = 3, NC = 4, ND = 2, NE = 6, NI = 3, NJ = 2, NK = 5, NL = 7 };
#define SENT_D (-7.5)
#define SENT_I (-77)

static double pat_d(int block, int i) { return 1000.0 * block + i + 0.25; }
static int pat_i(int block, int i) { return 1000 * block + i + 1; }

/* the table of both runs: doubles first, then ints; an odd count of ints in the middle (dI: the next block starts 4 bytes later than
 * it ends) and an odd count at the very end (dL: the allocation's tail is no multiple of 8) */
typedef struct {
    double *dA, *dB, *dC, *dD, *dE, *dZ;
    int *dI, *dJ, *dK, *dL;
    double inA[NA], inD[ND], outA[NA], outB[NB], outC[NC], outE[NE];
    int inK[NK], outI[NI], outJ[NJ], outL[NL];
    qr_stage_buf t[10];
} fixture;

static void fixture_init(fixture* f)
{
    for (int i = 0; i < NA; ++i) { f->inA[i] = pat_d(1, i); f->outA[i] = SENT_D; }
    for (int i = 0; i < ND; ++i) f->inD[i] = pat_d(4, i);
    for (int i = 0; i < NB; ++i) f->outB[i] = SENT_D;
    for (int i = 0; i < NC; ++i) f->outC[i] = SENT_D;
    for (int i = 0; i < NE; ++i) f->outE[i] = SENT_D;
    for (int i = 0; i < NK; ++i) f->inK[i] = pat_i(9, i);
    for (int i = 0; i < NI; ++i) f->outI[i] = SENT_I;
    for (int i = 0; i < NJ; ++i) f->outJ[i] = SENT_I;
    for (int i = 0; i < NL; ++i) f->outL[i] = SENT_I;
    const double* absent_in = NULL;
    double* absent_out = NULL;
    const qr_stage_buf t[10] = {
        QR_STAGE_F64(f->dA, NA, f->inA, f->outA, 0),        /* uploaded, downloaded */
        QR_STAGE_F64(f->dB, NB, NULL, f->outB, 1),          /* cleared, downloaded */
        QR_STAGE_F64(f->dC, NC, NULL, f->outC, 1),          /* cleared: one run with dB */
        QR_STAGE_F64(f->dD, ND, absent_in, NULL, 0),        /* an absent input: neither uploaded nor cleared nor downloaded */
        QR_STAGE_F64(f->dE, NE, NULL, absent_out, 1),       /* an absent output: cleared, not downloaded */
        QR_STAGE_F64(f->dZ, 0, NULL, f->outE, 1),           /* 0 bytes: never touched, outE keeps its sentinels */
        QR_STAGE_I32(f->dI, NI, NULL, f->outI, 1),          /* cleared, odd count */
        QR_STAGE_I32(f->dJ, NJ, NULL, f->outJ, 0),          /* neither uploaded nor cleared */
        QR_STAGE_I32(f->dK, NK, f->inK, NULL, 1),           /* uploaded: `zero` is ignored */
        QR_STAGE_I32(f->dL, NL, NULL, f->outL, 1),          /* cleared, odd count, the end of the allocation */
    };
    memcpy(f->t, t, sizeof t);
}

/* ascending, 8-byte aligned, each block where the one before it ended rounded up to 8 */
static int check_addresses(const qr_stage* st)
{
    size_t end = 0;
    for (int i = 0; i < st->nbufs; ++i) {
        const uintptr_t a = (uintptr_t) *st->bufs[i].dev, base = (uintptr_t) st->block;
        if (a % 8) FAIL(10, "block %d is not 8-byte aligned", i);
        if (a - base != ((end + 7) & ~(size_t) 7)) FAIL(11, "block %d at offset %zu, expected %zu", i, (size_t) (a - base), (end + 7) & ~(size_t) 7);
        if (a - base != st->bufs[i].off) FAIL(12, "block %d: address and recorded offset differ", i);
        end = (size_t) (a - base) + st->bufs[i].bytes;
    }
    return 0;
}

static int round_trip(void)
{
    fixture f;
    fixture_init(&f);
    qr_stage st;
    int rc = qr_stage_open(&st, 64, 8, f.t, 10);
    if (rc) FAIL(20, "open: %d", rc);
    if ((rc = check_addresses(&st)) != 0) return rc;
    /* what open left: the upload in dA and dK, zeros in every cleared block (the stub's allocation starts zeroed, so dD and dJ, which
     * nothing touched, read 0 as well) */
    for (int i = 0; i < NA; ++i) if (f.dA[i] != pat_d(1, i)) FAIL(21, "dA[%d] was not uploaded", i);
    for (int i = 0; i < NK; ++i) if (f.dK[i] != pat_i(9, i)) FAIL(22, "dK[%d] was not uploaded", i);
    for (int i = 0; i < NB; ++i) if (f.dB[i] != 0.0) FAIL(23, "dB[%d] was not cleared", i);
    for (int i = 0; i < NE; ++i) if (f.dE[i] != 0.0) FAIL(24, "dE[%d] was not cleared", i);
    /* "the kernel": a pattern through every device address but dC (cleared, never written) -- the last int of dL is the last word of
     * the allocation, one more would be the sanitizer's to report */
    for (int i = 0; i < NA; ++i) f.dA[i] = pat_d(11, i);
    for (int i = 0; i < NB; ++i) f.dB[i] = pat_d(12, i);
    for (int i = 0; i < ND; ++i) f.dD[i] = pat_d(14, i);
    for (int i = 0; i < NE; ++i) f.dE[i] = pat_d(15, i);
    for (int i = 0; i < NI; ++i) f.dI[i] = pat_i(16, i);
    for (int i = 0; i < NJ; ++i) f.dJ[i] = pat_i(17, i);
    for (int i = 0; i < NK; ++i) f.dK[i] = pat_i(18, i);
    for (int i = 0; i < NL; ++i) f.dL[i] = pat_i(19, i);
    /* no block disturbed a neighbour */
    for (int i = 0; i < NA; ++i) if (f.dA[i] != pat_d(11, i)) FAIL(30, "dA[%d] disturbed", i);
    for (int i = 0; i < NB; ++i) if (f.dB[i] != pat_d(12, i)) FAIL(31, "dB[%d] disturbed", i);
    for (int i = 0; i < NC; ++i) if (f.dC[i] != 0.0) FAIL(32, "dC[%d] disturbed", i);
    for (int i = 0; i < ND; ++i) if (f.dD[i] != pat_d(14, i)) FAIL(33, "dD[%d] disturbed", i);
    for (int i = 0; i < NE; ++i) if (f.dE[i] != pat_d(15, i)) FAIL(34, "dE[%d] disturbed", i);
    for (int i = 0; i < NI; ++i) if (f.dI[i] != pat_i(16, i)) FAIL(35, "dI[%d] disturbed", i);
    for (int i = 0; i < NJ; ++i) if (f.dJ[i] != pat_i(17, i)) FAIL(36, "dJ[%d] disturbed", i);
    for (int i = 0; i < NK; ++i) if (f.dK[i] != pat_i(18, i)) FAIL(37, "dK[%d] disturbed", i);
    rc = qr_stage_fetch(&st, 0);
    if (rc) FAIL(40, "fetch: %d", rc);
    for (int i = 0; i < NA; ++i) if (f.outA[i] != pat_d(11, i)) FAIL(41, "outA[%d]", i);
    for (int i = 0; i < NB; ++i) if (f.outB[i] != pat_d(12, i)) FAIL(42, "outB[%d]", i);
    for (int i = 0; i < NC; ++i) if (f.outC[i] != 0.0) FAIL(43, "outC[%d]: a cleared block that was never written must read 0", i);
    for (int i = 0; i < NE; ++i) if (f.outE[i] != SENT_D) FAIL(44, "outE[%d]: a block of 0 bytes downloads nothing", i);
    for (int i = 0; i < NI; ++i) if (f.outI[i] != pat_i(16, i)) FAIL(45, "outI[%d]", i);
    for (int i = 0; i < NJ; ++i) if (f.outJ[i] != pat_i(17, i)) FAIL(46, "outJ[%d]", i);
    for (int i = 0; i < NL; ++i) if (f.outL[i] != pat_i(19, i)) FAIL(47, "outL[%d]", i);
    for (int i = 0; i < NA; ++i) if (f.inA[i] != pat_d(1, i)) FAIL(48, "inA[%d] was written", i);
    qr_stage_close(&st);
    qr_stage_close(&st);                /* and once more: harmless */
    return 0;
}

/* a status that is already an error: nothing is downloaded, the status comes back */
static int error_path(void)
{
    fixture f;
    fixture_init(&f);
    qr_stage st;
    int rc = qr_stage_open(&st, 64, 8, f.t, 10);
    if (rc) FAIL(50, "open: %d", rc);
    for (int i = 0; i < NA; ++i) f.dA[i] = pat_d(11, i);
    for (int i = 0; i < NL; ++i) f.dL[i] = pat_i(19, i);
    rc = qr_stage_fetch(&st, QR_E_ARG);
    if (rc != QR_E_ARG) FAIL(51, "fetch after an error returned %d", rc);
    for (int i = 0; i < NA; ++i) if (f.outA[i] != SENT_D) FAIL(52, "outA[%d] was downloaded after an error", i);
    for (int i = 0; i < NB; ++i) if (f.outB[i] != SENT_D) FAIL(53, "outB[%d] was downloaded after an error", i);
    for (int i = 0; i < NI; ++i) if (f.outI[i] != SENT_I) FAIL(54, "outI[%d] was downloaded after an error", i);
    for (int i = 0; i < NL; ++i) if (f.outL[i] != SENT_I) FAIL(55, "outL[%d] was downloaded after an error", i);
    qr_stage_close(&st);
    return 0;
}

/* a total that does not fit a size_t: QR_E_ALLOC, every address NULL, fetch hands the status back, close is clean */
static int failed_open(void)
{
    double *d0 = (double*) &d0, *d1 = (double*) &d1, *d2 = (double*) &d2;
    double out[2] = { SENT_D, SENT_D };
    qr_stage_buf t[] = { QR_STAGE_F64(d0, 2, NULL, out, 1), { (void**) &d1, SIZE_MAX - 20, NULL, NULL, 0, 0 }, QR_STAGE_F64(d2, 4, NULL, NULL, 0) };
    qr_stage st;
    int rc = qr_stage_open(&st, 64, 8, t, QR_STAGE_COUNT(t));
    if (rc != QR_E_ALLOC) FAIL(60, "an overflowing total returned %d", rc);
    if (d0 || d1) FAIL(61, "a failed open left an address behind");
    if (qr_stage_fetch(&st, rc) != QR_E_ALLOC) FAIL(62, "fetch after a failed open");
    if (out[0] != SENT_D) FAIL(63, "a failed open downloaded");
    qr_stage_close(&st);
    /* the rounding itself overflows */
    qr_stage_buf u[] = { { (void**) &d0, SIZE_MAX - 3, NULL, NULL, 0, 0 }, QR_STAGE_F64(d1, 1, NULL, NULL, 0) };
    rc = qr_stage_open(&st, 64, 8, u, QR_STAGE_COUNT(u));
    if (rc != QR_E_ALLOC) FAIL(64, "an overflowing round-up returned %d", rc);
    qr_stage_close(&st);
    return 0;
}

static int any_word(void)
{
    const int w[5] = { 0, 0, 0, 0, 3 };
    if (qr_stage_any(w, 4) != 0 || qr_stage_any(w, 5) != 1 || qr_stage_any(w, 0) != 0) FAIL(70, "qr_stage_any");
    return 0;
}

int main(void)
{
    int rc;
    if ((rc = round_trip()) != 0) return rc;
    if ((rc = error_path()) != 0) return rc;
    if ((rc = failed_open()) != 0) return rc;
    if ((rc = any_word()) != 0) return rc;
    if (qrd_stub_live_allocations() != 0) FAIL(80, "device-memory leak: %d allocations still live", qrd_stub_live_allocations());
    printf("staging sanitize run ok: %ld device blocks checked\n", qrd_stub_launches());
    return 0;
}
