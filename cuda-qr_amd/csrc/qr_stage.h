/* qr_stage.h -- the staging every host-pointer twin of the batched sections (mi355x_qr.h sections 8 to 8l) does around its _dev call: a
 * plan of its own, ONE device allocation carved into the blocks of a table, uploads, clears, and after the call downloads and one
 * synchronisation.  Internal: not declared in the public header.
 *
 *   qr_stage_buf t[] = { QR_STAGE_F64(dA, nb * mn, A, NULL, 0), ..., QR_STAGE_I32(dinfo, nb, NULL, info, 0) };
 *   qr_stage st;
 *   int rc = qr_stage_open(&st, m, n, t, QR_STAGE_COUNT(t));
 *   if (!rc) rc = qr_..._batched_dev(st.plan, dA, ..., dinfo, batch);
 *   rc = qr_stage_fetch(&st, rc);
 *   if (!rc && qr_stage_any(info, nb)) rc = QR_E_SINGULAR;
 *   qr_stage_close(&st);
 *
 * Layout: the blocks lie in the allocation in table order, each at the end of the one before it rounded up to 8 bytes, the first at
 * offset 0.  The total and every address come from the one walk over the table (an overflowing total: QR_E_ALLOC).  Blocks of doubles
 * listed first are therefore packed exactly as doubles; blocks of ints follow in the same allocation and each starts on an 8-byte
 * boundary.  Nothing is padded further: a kernel that picked a wider load from a pointer's alignment must see the alignment it always saw.
 * A block of 0 bytes gets the address of its place and is never touched.  A block without `in` and `out` is scratch (or an optional
 * argument that is absent: it keeps its place, and the twin hands NULL to the _dev call instead of the address).
 *
 * Clears: a block with `zero` and no `in` is cleared before the call; a run of such blocks that are neighbours in the table is one
 * qrd_memset from the start of the first to the end of the last.
 *
 * Errors: the first failing step decides.  qr_stage_open stops at it (qr_stage_close is still safe, and is still needed).
 * qr_stage_fetch(st, rc) downloads only if rc is 0, always synchronises the stream, and uses the synchronisation's status only if
 * nothing failed before it.
 *
 * Calls nothing but qr_plan_create / qr_plan_destroy and qrd_malloc, qrd_free, qrd_h2d, qrd_d2h, qrd_memset, qrd_stream_sync, all of
 * which the stub device layer of the sanitizer builds has: tools/stage_sanitize.c runs this unit under ASan, UBSan and TSan. */
#ifndef QR_STAGE_H
#define QR_STAGE_H
#include <stddef.h>

#include "../../include/mi355x_qr.h"

typedef struct {
    void** dev;         /* receives the device address */
    size_t bytes;       /* size of the block; 0 is allowed */
    const void* in;     /* host source, uploaded before the call; NULL: no upload */
    void* out;          /* host destination, downloaded after the call; NULL: no download */
    int zero;           /* cleared before the call (ignored where `in` is given) */
    size_t off;         /* set by qr_stage_open: offset from the start of the allocation */
} qr_stage_buf;

typedef struct {
    qr_plan* plan;
    void* block;
    qr_stage_buf* bufs;
    int nbufs;
} qr_stage;

/* a block of `count` doubles / ints whose device address lands in the pointer variable `ptr` */
#define QR_STAGE_F64(ptr, count, in, out, zero) { (void**) &(ptr), sizeof(double) * (count), (in), (out), (zero), 0 }
#define QR_STAGE_I32(ptr, count, in, out, zero) { (void**) &(ptr), sizeof(int) * (count), (in), (out), (zero), 0 }
#define QR_STAGE_COUNT(t) ((int) (sizeof(t) / sizeof((t)[0])))

int qr_stage_open(qr_stage* st, int plan_m, int plan_n, qr_stage_buf* bufs, int nbufs);
int qr_stage_fetch(qr_stage* st, int rc);
void qr_stage_close(qr_stage* st);

/* 1 if any of `count` info words is non-zero */
int qr_stage_any(const int* info, size_t count);

#endif
