/* qr_batched_lmb.c -- batched Levenberg-Marquardt with box bounds on x: section 8m's loop with MPFIT's rules for lo <= x <= hi, split by
 * reverse communication into a step and an update on the device (mi355x_qr.h section 8n).
 *
 *   qr_lmb_batched_create / _destroy   the handle: one device allocation carved into the packed state arrays, jpvt and tau
 *   qr_lmb_batched_start_dev           qrd_blmb_start: the bounds checked, x <- X0, D, lo, hi, the counters
 *   qr_lmb_batched_step_dev            qrd_blmb_peg on J and f, qrd_b_geqp3 on J, qrd_b_ormqr 'T' on f, qrd_blmb_step on the triangle and all
 *                                      rows of Q^T f
 *   qr_lmb_batched_update_dev          qrd_blmb_update on f at the trial points
 *   qr_lmb_batched_running             the status and info words to the host, counted there: the one call that waits
 *   qr_lstsq_lm_bounded_batched        the whole solve on host pointers, the model a callback on host buffers
 *
 * The plan supplies the stream.  The order of the calls is kept by a phase flag of the handle, on the host.  The allocation pattern, the
 * phase flag and the stride rules are qr_batched_lm.c's; the options are qr_lm_options (qr_lm_options_default is defined there).
 *
 * A unit of its own, and not yet one of the units that run over the stub device layer of the sanitizer builds: the stub has no entry
 * for the four launch wrappers called here. */
#define _POSIX_C_SOURCE 200809L
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355x_qr.h"
#include "qr_device.h"
#include "qr_plan_internal.h"
#include "qr_stage.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

enum { LM_CREATED = 0, LM_AT_X = 1, LM_STEPPED = 2 };     /* what may come next: start; a step; an update */

struct qr_lmb_batched {
    qr_plan* p;
    int m, n, batch, phase;
    qr_lm_options o;
    void* block;                  /* the one device allocation */
    qrd_blmb_state s;
    double* tau;
    int* jpvt;
    int* hwords;                  /* host: status and info of every member, as qr_lmb_batched_running fetches them */
};

/* a block of `cols` columns of `rows` rows: columns at least `rows` apart, members at least ld * cols apart */
static int bad_block(int rows, long long cols, int ld, long long stride) { return cols < 1 || ld < rows || stride < (long long) ld * cols; }

/* `len` values per member that every member may share: a stride of 0, or at least len */
static int bad_shared(long long stride, int len) { return stride != 0 && stride < len; }

static int bad_options(const qr_lm_options* o)
{
    return !(o->ftol >= 0.0) || !(o->xtol >= 0.0) || !(o->gtol >= 0.0) || !(o->factor > 0.0 && o->factor <= DBL_MAX) ||
           !(o->par_rtol > 0.0 && o->par_rtol < 1.0) || o->maxfev < 0 || (o->mode != 1 && o->mode != 2) || o->par_maxit < 1;
}

static int bad_shape(int m, int n) { return n < 1 || n > QR_BATCHED_MAX_N - 1 || m < n || m > qrd_b_max_rows(n + 1); }

int qr_lmb_batched_create(qr_lmb_batched** out, qr_plan* p, int m, int n, int batch, const qr_lm_options* opt)
{
    qr_lm_options o;
    qr_lm_options_default(&o);
    if (opt) o = *opt;
    if (!out || !p || bad_shape(m, n) || batch < 0 || bad_options(&o)) return QR_E_ARG;
    if (o.maxfev == 0) o.maxfev = 100 * (n + 1);
    qr_lmb_batched* h = (qr_lmb_batched*) calloc(1, sizeof *h);
    if (!h) return QR_E_ALLOC;
    h->p = p; h->m = m; h->n = n; h->batch = batch; h->o = o; h->phase = LM_CREATED;
    if (batch > 0) {
        const size_t nb = (size_t) batch, nn = (size_t) n;
        const size_t doubles = nb * (6 * nn + 9), ints = nb * (2 * nn + 8);
        const size_t bytes = sizeof(double) * doubles + sizeof(int) * ints;
        h->hwords = (int*) malloc(sizeof(int) * 2 * nb);
        int rc = h->hwords ? qrd_malloc(&h->block, bytes) : QR_E_ALLOC;
        /* cleared once: a member that start refuses (info -2) has nothing else written, and its words must not read as garbage */
        if (!rc && (rc = qrd_memset(p->stream, h->block, 0, bytes)) != 0) qrd_free(h->block);
        if (rc) {
            free(h->hwords);
            free(h);
            return rc;
        }
        double* d = (double*) h->block;
        qrd_blm_state* s = &h->s.b;
        s->x = d; d += nb * nn;
        s->xtrial = d; d += nb * nn;
        s->D = d; d += nb * nn;
        h->tau = d; d += nb * nn;
        h->s.lo = d; d += nb * nn;
        h->s.hi = d; d += nb * nn;
        s->delta = d; d += nb; s->par = d; d += nb; s->fnorm = d; d += nb; s->xnorm = d; d += nb;
        s->pnorm = d; d += nb; s->gnorm = d; d += nb; s->prered = d; d += nb; s->dirder = d; d += nb;
        h->s.alpha = d; d += nb;
        int* w = (int*) d;
        s->iter = w; w += nb; s->nfev = w; w += nb; s->njev = w; w += nb; s->accepted = w; w += nb;
        s->status = w; w += nb; s->info = w; w += nb;        /* (neighbours: qr_lmb_batched_running fetches the two in one copy) */
        s->par_status = w; w += nb;
        h->s.clipped = w; w += nb;
        h->s.peg = w; w += nb * nn;
        h->jpvt = w;
    }
    *out = h;
    return 0;
}

int qr_lmb_batched_destroy(qr_lmb_batched* h)
{
    if (!h) return QR_E_ARG;
    int rc = 0;
    if (h->batch > 0) {
        rc = qrd_stream_sync(h->p->stream);
        qrd_free(h->block);
        free(h->hwords);
    }
    free(h);
    return rc;
}

int qr_lmb_batched_start_dev(qr_lmb_batched* h, const double* dX0, int ldx, long long strideX, const double* dD0, long long strideD,
                             const double* dLo, long long strideLo, const double* dHi, long long strideHi)
{
    if (!h || !dX0 || bad_block(h->n, 1, ldx, strideX) || (h->o.mode == 2 && (!dD0 || bad_shared(strideD, h->n))) ||
        (dLo && bad_shared(strideLo, h->n)) || (dHi && bad_shared(strideHi, h->n)))
        return QR_E_ARG;
    h->phase = LM_AT_X;
    if (h->batch == 0) return 0;
    return qrd_blmb_start(h->p->stream, dX0, ldx, (size_t) strideX, h->o.mode == 2 ? dD0 : NULL, (size_t) (h->o.mode == 2 ? strideD : 0), dLo,
                          (size_t) (dLo ? strideLo : 0), dHi, (size_t) (dHi ? strideHi : 0), h->n, h->batch, &h->s, h->o.mode);
}

static void fill(qrd_blmb_step_args* a, const qr_lmb_batched* h)
{
    memset(a, 0, sizeof *a);
    a->d.n = h->n; a->d.nrhs = 1; a->d.nlam = 1; a->d.batch = h->batch;
    a->s = h->s;
    a->o.ftol = h->o.ftol; a->o.xtol = h->o.xtol; a->o.gtol = h->o.gtol; a->o.factor = h->o.factor; a->o.par_rtol = h->o.par_rtol;
    a->o.maxfev = h->o.maxfev; a->o.mode = h->o.mode; a->o.par_maxit = h->o.par_maxit;
}

int qr_lmb_batched_step_dev(qr_lmb_batched* h, double* dJ, int ldj, long long strideJ, double* dF, int ldf, long long strideF)
{
    if (!h || !dJ || !dF || bad_block(h->m, h->n, ldj, strideJ) || bad_block(h->m, 1, ldf, strideF) || h->phase != LM_AT_X) return QR_E_ARG;
    h->phase = LM_STEPPED;
    if (h->batch == 0) return 0;
    const size_t sj = (size_t) strideJ, sf = (size_t) strideF, n = (size_t) h->n;
    CHECK(qrd_blmb_peg(h->p->stream, dJ, h->m, ldj, sj, dF, sf, h->n, h->batch, &h->s));
    CHECK(qrd_b_geqp3(h->p->stream, dJ, h->m, h->n, ldj, sj, h->jpvt, n, h->tau, n, NULL, 0, 0, 0, 0.0, 0, NULL, NULL, h->batch));
    CHECK(qrd_b_ormqr(h->p->stream, 1, dJ, h->m, h->n, ldj, sj, h->tau, n, dF, 1, ldf, sf, h->batch));
    qrd_blmb_step_args a;
    fill(&a, h);
    a.d.R = dJ; a.d.ldr = ldj; a.d.sR = sj;
    a.d.Z = dF; a.d.ldz = ldf; a.d.sZ = sf; a.d.zrows = h->m;       /* all rows: the tail of Q^T f is summed in the launch */
    a.d.jpvt = h->jpvt; a.d.sj = n;
    return qrd_blmb_step(h->p->stream, &a);
}

int qr_lmb_batched_update_dev(qr_lmb_batched* h, const double* dFtrial, int ldf, long long strideF)
{
    if (!h || !dFtrial || bad_block(h->m, 1, ldf, strideF) || h->phase != LM_STEPPED) return QR_E_ARG;
    h->phase = LM_AT_X;
    if (h->batch == 0) return 0;
    qrd_blmb_step_args a;
    fill(&a, h);
    return qrd_blmb_update(h->p->stream, dFtrial, h->m, ldf, (size_t) strideF, h->n, h->batch, &a.s, &a.o);
}

int qr_lmb_batched_view(qr_lmb_batched* h, qr_lmb_batched_state* v)
{
    if (!h || !v) return QR_E_ARG;
    const qrd_blm_state* s = &h->s.b;
    v->x = s->x; v->xtrial = s->xtrial; v->D = s->D; v->delta = s->delta; v->par = s->par; v->fnorm = s->fnorm; v->xnorm = s->xnorm;
    v->pnorm = s->pnorm; v->gnorm = s->gnorm; v->prered = s->prered; v->dirder = s->dirder;
    v->iter = s->iter; v->nfev = s->nfev; v->njev = s->njev; v->accepted = s->accepted; v->status = s->status; v->info = s->info;
    v->par_status = s->par_status;
    v->lo = h->s.lo; v->hi = h->s.hi; v->alpha = h->s.alpha; v->peg = h->s.peg; v->clipped = h->s.clipped;
    return 0;
}

int qr_lmb_batched_running(qr_lmb_batched* h, int* count)
{
    if (!h || !count || h->phase == LM_CREATED) return QR_E_ARG;
    *count = 0;
    if (h->batch == 0) return 0;
    const size_t nb = (size_t) h->batch;
    CHECK(qrd_d2h(h->p->stream, h->hwords, h->s.b.status, sizeof(int) * 2 * nb));
    CHECK(qrd_stream_sync(h->p->stream));
    int c = 0;
    for (size_t q = 0; q < nb; ++q) c += h->hwords[q] == 0 && h->hwords[nb + q] == 0;
    *count = c;
    return 0;
}

/* the host-pointer twin: the operands staged as qr_stage.h describes, the model called on host buffers between the device calls */
int qr_lstsq_lm_bounded_batched(qr_lm_fcn fcn, void* user, int m, int n, int batch, double* X, const double* lo, const double* hi,
                                const double* D, const qr_lm_options* opt, double* fnorm, int* nfev, int* njev, int* status, int* info)
{
    qr_lm_options o;
    qr_lm_options_default(&o);
    if (opt) o = *opt;
    if (!fcn || !X || !info || bad_shape(m, n) || batch < 0 || bad_options(&o) || (o.mode == 2 && !D)) return QR_E_ARG;
    if (batch == 0) return 0;
    const size_t nb = (size_t) batch, mn = (size_t) m * n, xn = nb * (size_t) n, xb = sizeof(double) * xn, fb = sizeof(double) * nb * (size_t) m;
    double* hX = (double*) malloc(xb);
    double* hF = (double*) malloc(fb);
    double* hJ = (double*) malloc(sizeof(double) * nb * mn);
    double *dX0, *dD, *dLo, *dHi, *dJ, *dF;
    qr_stage_buf t[] = { QR_STAGE_F64(dX0, xn, X, NULL, 0), QR_STAGE_F64(dD, xn, o.mode == 2 ? D : NULL, NULL, 0),
                         QR_STAGE_F64(dLo, xn, lo, NULL, 0), QR_STAGE_F64(dHi, xn, hi, NULL, 0),
                         QR_STAGE_F64(dJ, nb * mn, NULL, NULL, 0), QR_STAGE_F64(dF, nb * (size_t) m, NULL, NULL, 0) };
    qr_stage st;
    qr_lmb_batched* h = NULL;
    int rc = (hX && hF && hJ) ? qr_stage_open(&st, m, n, t, QR_STAGE_COUNT(t)) : QR_E_ALLOC;
    const int opened = hX && hF && hJ;
    if (!rc) rc = qr_lmb_batched_create(&h, st.plan, m, n, batch, &o);
    if (!rc) rc = qr_lmb_batched_start_dev(h, dX0, n, n, o.mode == 2 ? dD : NULL, n, lo ? dLo : NULL, n, hi ? dHi : NULL, n);
    if (!rc) {
        void* s = st.plan->stream;
        const qrd_blm_state* b = &h->s.b;
        const int rounds = h->o.maxfev + 2;                       /* (every round adds 1 to nfev of every running member) */
        for (int round = 0, count = 1; !rc && count > 0 && round < rounds; ++round) {
            /* (a member that start refused has no x in the state: the model is called on its x0, and what it returns is not used) */
            rc = round == 0 ? qrd_d2h(s, hX, dX0, xb) : qrd_d2h(s, hX, b->x, xb);
            if (!rc) rc = qrd_stream_sync(s);
            if (!rc) rc = fcn(user, 1, hX, batch, hF, NULL);
            if (!rc) rc = fcn(user, 2, hX, batch, NULL, hJ);
            if (!rc) rc = qrd_h2d(s, dF, hF, fb);
            if (!rc) rc = qrd_h2d(s, dJ, hJ, sizeof(double) * nb * mn);
            if (!rc) rc = qr_lmb_batched_step_dev(h, dJ, m, (long long) mn, dF, m, m);
            if (!rc) rc = qrd_d2h(s, hX, b->xtrial, xb);
            if (!rc) rc = qrd_stream_sync(s);
            if (!rc) rc = fcn(user, 3, hX, batch, hF, NULL);
            if (!rc) rc = qrd_h2d(s, dF, hF, fb);
            if (!rc) rc = qr_lmb_batched_update_dev(h, dF, m, m);
            if (!rc) rc = qr_lmb_batched_running(h, &count);
        }
        if (!rc) rc = qrd_d2h(s, hX, b->x, xb);
        if (!rc && fnorm) rc = qrd_d2h(s, fnorm, b->fnorm, sizeof(double) * nb);
        if (!rc && nfev) rc = qrd_d2h(s, nfev, b->nfev, sizeof(int) * nb);
        if (!rc && njev) rc = qrd_d2h(s, njev, b->njev, sizeof(int) * nb);
        if (!rc && status) rc = qrd_d2h(s, status, b->status, sizeof(int) * nb);
        if (!rc) rc = qrd_d2h(s, info, b->info, sizeof(int) * nb);
    }
    if (opened) rc = qr_stage_fetch(&st, rc);
    if (!rc)                                                      /* a member that start refused keeps the X it came with */
        for (size_t q = 0; q < nb; ++q)
            if (info[q] != -2) memcpy(X + q * (size_t) n, hX + q * (size_t) n, sizeof(double) * (size_t) n);
    if (h) qr_lmb_batched_destroy(h);
    if (!rc && qr_stage_any(info, nb)) rc = QR_E_SINGULAR;
    if (opened) qr_stage_close(&st);
    free(hJ);
    free(hF);
    free(hX);
    return rc;
}
