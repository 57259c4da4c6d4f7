/* qr_stage.c -- one plan, one device allocation, uploads, clears, downloads and one synchronisation for the host-pointer twins of the
 * batched sections; the contract is in qr_stage.h. */
#include <stdint.h>
#include <string.h>

#include "../../include/mi355x_qr.h"
#include "qr_device.h"
#include "qr_plan_internal.h"
#include "qr_stage.h"

int qr_stage_open(qr_stage* st, int plan_m, int plan_n, qr_stage_buf* bufs, int nbufs)
{
    memset(st, 0, sizeof *st);
    st->bufs = bufs; st->nbufs = nbufs;
    /* the one walk: every offset and, from the last of them, the total */
    size_t total = 0;
    for (int i = 0; i < nbufs; ++i) {
        *bufs[i].dev = NULL;
        if (total > SIZE_MAX - 7) return QR_E_ALLOC;
        bufs[i].off = (total + 7) & ~(size_t) 7;
        if (bufs[i].bytes > SIZE_MAX - bufs[i].off) return QR_E_ALLOC;
        total = bufs[i].off + bufs[i].bytes;
    }
    int rc = qr_plan_create(&st->plan, plan_m, plan_n, 0, 0);
    if (rc) return rc;
    rc = qrd_malloc(&st->block, total);
    if (rc) return rc;
    void* s = st->plan->stream;
    for (int i = 0; i < nbufs; ++i) *bufs[i].dev = (char*) st->block + bufs[i].off;
    for (int i = 0; !rc && i < nbufs; ++i)
        if (bufs[i].in && bufs[i].bytes) rc = qrd_h2d(s, *bufs[i].dev, bufs[i].in, bufs[i].bytes);
    for (int i = 0; !rc && i < nbufs; ++i) {
        if (!bufs[i].zero || bufs[i].in) continue;
        int j = i;                          /* [i, j]: a run of neighbours that are all cleared */
        while (j + 1 < nbufs && bufs[j + 1].zero && !bufs[j + 1].in) ++j;
        const size_t bytes = bufs[j].off + bufs[j].bytes - bufs[i].off;
        if (bytes) rc = qrd_memset(s, *bufs[i].dev, 0, bytes);
        i = j;
    }
    return rc;
}

int qr_stage_fetch(qr_stage* st, int rc)
{
    if (!st->plan) return rc;               /* the open failed before there was a stream */
    for (int i = 0; !rc && i < st->nbufs; ++i)
        if (st->bufs[i].out && st->bufs[i].bytes) rc = qrd_d2h(st->plan->stream, st->bufs[i].out, *st->bufs[i].dev, st->bufs[i].bytes);
    const int rs = qrd_stream_sync(st->plan->stream);
    return rc ? rc : rs;
}

void qr_stage_close(qr_stage* st)
{
    if (st->block) qrd_free(st->block);
    if (st->plan) qr_plan_destroy(st->plan);
    st->block = NULL; st->plan = NULL;
}

int qr_stage_any(const int* info, size_t count)
{
    for (size_t i = 0; i < count; ++i)
        if (info[i]) return 1;
    return 0;
}
