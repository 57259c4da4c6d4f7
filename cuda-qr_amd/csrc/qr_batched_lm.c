/* qr_batched_lm.c -- batched Levenberg-Marquardt: MINPACK lmder's outer loop per member, split by reverse communication into a step and
 * an update on the device (mi355x_qr.h section 8m), and the same loop with box bounds on x (section 8n, MPFIT's rules).
 *
 *   qr_lm_batched_create / _destroy   the handle: one device allocation carved into the packed state arrays, jpvt and tau
 *   qr_lm_batched_start_dev           qrd_blm_start: x <- X0, D, the counters
 *   qr_lm_batched_step_dev            qrd_b_geqp3 on J, qrd_b_ormqr 'T' on f, qrd_blm_step on the triangle and all rows of Q^T f
 *   qr_lm_step_batched_dev            qrd_blm_step alone on factors that exist (section 8m only: the peg reads the unfactored J)
 *   qr_lm_batched_update_dev          qrd_blm_update on f at the trial points
 *   qr_lm_batched_running             the status and info words to the host, counted there: the one call that waits
 *   qr_lstsq_lm_batched               the whole solve on host pointers, the model a callback on host buffers
 *   qr_lmb_batched_* and qr_lstsq_lm_bounded_batched: the same calls of section 8n; start is qrd_blmb_start (the bounds checked, lo, hi),
 *                                     the step has qrd_blmb_peg on J and f in front and ends in qrd_blmb_step, the update is qrd_blmb_update
 *
 * One handle struct serves both sections: it holds a qrd_blmb_state, whose .b is what the launches of section 8m get, and a `bounded`
 * flag; every call is written once below (lm_*) and the public functions of either section are its callers.  A handle of one section
 * passed to a call of the other returns QR_E_ARG.  The plan supplies the stream.  The order of the calls is kept by a phase flag of the
 * handle, on the host.
 *
 * Kept out of qr_host.c for the reason qr_solve.c is: the sanitizer and stub builds compile qr_host.c against a stub device layer that
 * has none of the launch wrappers called here. */
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

struct qr_lm_batched {
    qr_plan* p;
    int m, n, batch, phase;
    int bounded;                  /* 0: a qr_lm_batched of section 8m, 1: a qr_lmb_batched of section 8n */
    qr_lm_options o;
    void* block;                  /* the one device allocation */
    qrd_blmb_state s;             /* (lo, hi, alpha, peg and clipped stay NULL in an unbounded handle) */
    double* tau;
    int* jpvt;
    int* hwords;                  /* host: status and info of every member, as lm_running fetches them */
};

/* the handle behind a public pointer of either section; NULL where it is of the other section */
static qr_lm_batched* of_kind(void* handle, int bounded)
{
    qr_lm_batched* h = (qr_lm_batched*) handle;
    return h && h->bounded == bounded ? h : NULL;
}

/* a block of `cols` columns of `rows` rows: columns at least `rows` apart, members at least ld * cols apart */
static int bad_block(int rows, long long cols, int ld, long long stride) { return cols < 1 || ld < rows || stride < (long long) ld * cols; }

/* `len` values per member that every member may share: a stride of 0, or at least len */
static int bad_shared(long long stride, int len) { return stride != 0 && stride < len; }

void qr_lm_options_default(qr_lm_options* o)
{
    if (!o) return;
    o->ftol = o->xtol = sqrt(DBL_EPSILON);
    o->gtol = 0.0;
    o->factor = 100.0;
    o->par_rtol = 0.1;
    o->maxfev = 0;                /* 100 (n + 1), filled in where n is known */
    o->mode = 1;
    o->par_maxit = 10;
}

static int bad_options(const qr_lm_options* o)
{
    return !(o->ftol >= 0.0) || !(o->xtol >= 0.0) || !(o->gtol >= 0.0) || !(o->factor > 0.0 && o->factor <= DBL_MAX) ||
           !(o->par_rtol > 0.0 && o->par_rtol < 1.0) || o->maxfev < 0 || (o->mode != 1 && o->mode != 2) || o->par_maxit < 1;
}

static int bad_shape(int m, int n) { return n < 1 || n > QR_BATCHED_MAX_N - 1 || m < n || m > qrd_b_max_rows(n + 1); }

static int lm_create(qr_lm_batched** out, qr_plan* p, int m, int n, int batch, const qr_lm_options* opt, int bounded)
{
    qr_lm_options o;
    qr_lm_options_default(&o);
    if (opt) o = *opt;
    if (!out || !p || bad_shape(m, n) || batch < 0 || bad_options(&o)) return QR_E_ARG;
    if (o.maxfev == 0) o.maxfev = 100 * (n + 1);
    qr_lm_batched* h = (qr_lm_batched*) calloc(1, sizeof *h);
    if (!h) return QR_E_ALLOC;
    h->p = p; h->m = m; h->n = n; h->batch = batch; h->o = o; h->phase = LM_CREATED; h->bounded = bounded;
    if (batch > 0) {
        const size_t nb = (size_t) batch, nn = (size_t) n;
        /* x, xtrial, D, tau (and lo, hi): n each; eight scalars (and alpha); seven words (and clipped); jpvt (and peg): n each */
        const size_t doubles = bounded ? nb * (6 * nn + 9) : nb * (4 * nn + 8), ints = bounded ? nb * (2 * nn + 8) : nb * (nn + 7);
        const size_t bytes = sizeof(double) * doubles + sizeof(int) * ints;
        h->hwords = (int*) malloc(sizeof(int) * 2 * nb);
        int rc = h->hwords ? qrd_malloc(&h->block, bytes) : QR_E_ALLOC;
        /* bounded: cleared once: a member that start refuses (info -2) has nothing else written, and its words must not read as garbage */
        if (!rc && bounded && (rc = qrd_memset(p->stream, h->block, 0, bytes)) != 0) qrd_free(h->block);
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
        if (bounded) { h->s.lo = d; d += nb * nn; h->s.hi = d; d += nb * nn; }
        s->delta = d; d += nb; s->par = d; d += nb; s->fnorm = d; d += nb; s->xnorm = d; d += nb;
        s->pnorm = d; d += nb; s->gnorm = d; d += nb; s->prered = d; d += nb; s->dirder = d; d += nb;
        if (bounded) { h->s.alpha = d; d += nb; }
        int* w = (int*) d;
        s->iter = w; w += nb; s->nfev = w; w += nb; s->njev = w; w += nb; s->accepted = w; w += nb;
        s->status = w; w += nb; s->info = w; w += nb;        /* (neighbours: lm_running fetches the two in one copy) */
        s->par_status = w; w += nb;
        if (bounded) { h->s.clipped = w; w += nb; h->s.peg = w; w += nb * nn; }
        h->jpvt = w;
    }
    *out = h;
    return 0;
}

static int lm_destroy(qr_lm_batched* h)
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

/* dLo, dHi and their strides are looked at for a bounded handle only */
static int lm_start(qr_lm_batched* h, const double* dX0, int ldx, long long strideX, const double* dD0, long long strideD, const double* dLo,
                    long long strideLo, const double* dHi, long long strideHi)
{
    if (!h || !dX0 || bad_block(h->n, 1, ldx, strideX) || (h->o.mode == 2 && (!dD0 || bad_shared(strideD, h->n))) ||
        (h->bounded && ((dLo && bad_shared(strideLo, h->n)) || (dHi && bad_shared(strideHi, h->n)))))
        return QR_E_ARG;
    h->phase = LM_AT_X;
    if (h->batch == 0) return 0;
    const double* D0 = h->o.mode == 2 ? dD0 : NULL;
    const size_t sX = (size_t) strideX, sD = (size_t) (h->o.mode == 2 ? strideD : 0);
    if (!h->bounded) return qrd_blm_start(h->p->stream, dX0, ldx, sX, D0, sD, h->n, h->batch, &h->s.b, h->o.mode);
    return qrd_blmb_start(h->p->stream, dX0, ldx, sX, D0, sD, dLo, (size_t) (dLo ? strideLo : 0), dHi, (size_t) (dHi ? strideHi : 0), h->n,
                          h->batch, &h->s, h->o.mode);
}

static qrd_blm_opts lm_opts(const qr_lm_batched* h)
{
    qrd_blm_opts o;
    memset(&o, 0, sizeof o);
    o.ftol = h->o.ftol; o.xtol = h->o.xtol; o.gtol = h->o.gtol; o.factor = h->o.factor; o.par_rtol = h->o.par_rtol;
    o.maxfev = h->o.maxfev; o.mode = h->o.mode; o.par_maxit = h->o.par_maxit;
    return o;
}

/* the step launch of the handle's section on the factors d describes (R, Z, rss, jpvt and their strides; the rest is filled in here) */
static int lm_step_launch(const qr_lm_batched* h, qrd_bd_args d)
{
    d.n = h->n; d.nrhs = 1; d.nlam = 1; d.batch = h->batch;
    if (h->bounded) {
        qrd_blmb_step_args a;
        memset(&a, 0, sizeof a);
        a.d = d; a.s = h->s; a.o = lm_opts(h);
        return qrd_blmb_step(h->p->stream, &a);
    }
    qrd_blm_step_args a;
    memset(&a, 0, sizeof a);
    a.d = d; a.s = h->s.b; a.o = lm_opts(h);
    return qrd_blm_step(h->p->stream, &a);
}

static int lm_step(qr_lm_batched* h, double* dJ, int ldj, long long strideJ, double* dF, int ldf, long long strideF)
{
    if (!h || !dJ || !dF || bad_block(h->m, h->n, ldj, strideJ) || bad_block(h->m, 1, ldf, strideF) || h->phase != LM_AT_X) return QR_E_ARG;
    h->phase = LM_STEPPED;
    if (h->batch == 0) return 0;
    const size_t sj = (size_t) strideJ, sf = (size_t) strideF, n = (size_t) h->n;
    if (h->bounded) CHECK(qrd_blmb_peg(h->p->stream, dJ, h->m, ldj, sj, dF, sf, h->n, h->batch, &h->s));
    CHECK(qrd_b_geqp3(h->p->stream, dJ, h->m, h->n, ldj, sj, h->jpvt, n, h->tau, n, NULL, 0, 0, 0, 0.0, 0, NULL, NULL, h->batch));
    CHECK(qrd_b_ormqr(h->p->stream, 1, dJ, h->m, h->n, ldj, sj, h->tau, n, dF, 1, ldf, sf, h->batch));
    qrd_bd_args d;
    memset(&d, 0, sizeof d);
    d.R = dJ; d.ldr = ldj; d.sR = sj;
    d.Z = dF; d.ldz = ldf; d.sZ = sf; d.zrows = h->m;       /* all rows: the tail of Q^T f is summed in the launch */
    d.jpvt = h->jpvt; d.sj = n;
    return lm_step_launch(h, d);
}

static int lm_update(qr_lm_batched* h, const double* dFtrial, int ldf, long long strideF)
{
    if (!h || !dFtrial || bad_block(h->m, 1, ldf, strideF) || h->phase != LM_STEPPED) return QR_E_ARG;
    h->phase = LM_AT_X;
    if (h->batch == 0) return 0;
    const qrd_blm_opts o = lm_opts(h);
    if (h->bounded) return qrd_blmb_update(h->p->stream, dFtrial, h->m, ldf, (size_t) strideF, h->n, h->batch, &h->s, &o);
    return qrd_blm_update(h->p->stream, dFtrial, h->m, ldf, (size_t) strideF, h->n, h->batch, &h->s.b, &o);
}

static int lm_running(qr_lm_batched* h, int* count)
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

/* the fields that the public state structs of both sections begin with */
#define VIEW_8M(v, s) do { \
    (v)->x = (s)->x; (v)->xtrial = (s)->xtrial; (v)->D = (s)->D; (v)->delta = (s)->delta; (v)->par = (s)->par; (v)->fnorm = (s)->fnorm; \
    (v)->xnorm = (s)->xnorm; (v)->pnorm = (s)->pnorm; (v)->gnorm = (s)->gnorm; (v)->prered = (s)->prered; (v)->dirder = (s)->dirder; \
    (v)->iter = (s)->iter; (v)->nfev = (s)->nfev; (v)->njev = (s)->njev; (v)->accepted = (s)->accepted; (v)->status = (s)->status; \
    (v)->info = (s)->info; (v)->par_status = (s)->par_status; } while (0)

/* the host-pointer twin of either section: the operands staged as qr_stage.h describes, the model called on host buffers between the
 * device calls.  lo, hi: looked at for the bounded solve only (either may be NULL) */
static int lm_solve(int bounded, qr_lm_fcn fcn, void* user, int m, int n, int batch, double* X, const double* lo, const double* hi,
                    const double* D, const qr_lm_options* opt, double* fnorm, int* nfev, int* njev, int* status, int* info)
{
    qr_lm_options o;
    qr_lm_options_default(&o);
    if (opt) o = *opt;
    if (!fcn || !X || !info || bad_shape(m, n) || batch < 0 || bad_options(&o) || (o.mode == 2 && !D)) return QR_E_ARG;
    if (batch == 0) return 0;
    if (!bounded) lo = hi = NULL;
    const size_t nb = (size_t) batch, mn = (size_t) m * n, xn = nb * (size_t) n, xb = sizeof(double) * xn, fb = sizeof(double) * nb * (size_t) m;
    double* hX = (double*) malloc(xb);
    double* hF = (double*) malloc(fb);
    double* hJ = (double*) malloc(sizeof(double) * nb * mn);
    double *dX0, *dD, *dJ, *dF, *dLo = NULL, *dHi = NULL;
    qr_stage_buf t[] = { QR_STAGE_F64(dX0, xn, X, NULL, 0), QR_STAGE_F64(dD, xn, o.mode == 2 ? D : NULL, NULL, 0),
                         QR_STAGE_F64(dJ, nb * mn, NULL, NULL, 0), QR_STAGE_F64(dF, nb * (size_t) m, NULL, NULL, 0),
                         QR_STAGE_F64(dLo, xn, lo, NULL, 0), QR_STAGE_F64(dHi, xn, hi, NULL, 0) };      /* (the last two: 8n only) */
    qr_stage st;
    qr_lm_batched* h = NULL;
    int rc = (hX && hF && hJ) ? qr_stage_open(&st, m, n, t, QR_STAGE_COUNT(t) - (bounded ? 0 : 2)) : QR_E_ALLOC;
    const int opened = hX && hF && hJ;
    if (!rc) rc = lm_create(&h, st.plan, m, n, batch, &o, bounded);
    if (!rc) rc = lm_start(h, dX0, n, n, o.mode == 2 ? dD : NULL, n, lo ? dLo : NULL, n, hi ? dHi : NULL, n);
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
            if (!rc) rc = lm_step(h, dJ, m, (long long) mn, dF, m, m);
            if (!rc) rc = qrd_d2h(s, hX, b->xtrial, xb);
            if (!rc) rc = qrd_stream_sync(s);
            if (!rc) rc = fcn(user, 3, hX, batch, hF, NULL);
            if (!rc) rc = qrd_h2d(s, dF, hF, fb);
            if (!rc) rc = lm_update(h, dF, m, m);
            if (!rc) rc = lm_running(h, &count);
        }
        if (!rc) rc = qrd_d2h(s, hX, b->x, xb);
        if (!rc && fnorm) rc = qrd_d2h(s, fnorm, b->fnorm, sizeof(double) * nb);
        if (!rc && nfev) rc = qrd_d2h(s, nfev, b->nfev, sizeof(int) * nb);
        if (!rc && njev) rc = qrd_d2h(s, njev, b->njev, sizeof(int) * nb);
        if (!rc && status) rc = qrd_d2h(s, status, b->status, sizeof(int) * nb);
        if (!rc) rc = qrd_d2h(s, info, b->info, sizeof(int) * nb);
    }
    if (opened) rc = qr_stage_fetch(&st, rc);
    if (!rc)                                                      /* a member that start refused (8n) keeps the X it came with */
        for (size_t q = 0; q < nb; ++q)
            if (info[q] != -2) memcpy(X + q * (size_t) n, hX + q * (size_t) n, sizeof(double) * (size_t) n);
    if (h) lm_destroy(h);
    if (!rc && qr_stage_any(info, nb)) rc = QR_E_SINGULAR;
    if (opened) qr_stage_close(&st);
    free(hJ);
    free(hF);
    free(hX);
    return rc;
}

/* ---- section 8m ---- */
int qr_lm_batched_create(qr_lm_batched** out, qr_plan* p, int m, int n, int batch, const qr_lm_options* opt)
{
    return lm_create(out, p, m, n, batch, opt, 0);
}

int qr_lm_batched_destroy(qr_lm_batched* h) { return lm_destroy(of_kind(h, 0)); }

int qr_lm_batched_start_dev(qr_lm_batched* h, const double* dX0, int ldx, long long strideX, const double* dD0, long long strideD)
{
    return lm_start(of_kind(h, 0), dX0, ldx, strideX, dD0, strideD, NULL, 0, NULL, 0);
}

int qr_lm_batched_step_dev(qr_lm_batched* h, double* dJ, int ldj, long long strideJ, double* dF, int ldf, long long strideF)
{
    return lm_step(of_kind(h, 0), dJ, ldj, strideJ, dF, ldf, strideF);
}

int qr_lm_step_batched_dev(qr_lm_batched* lm, const double* dR, int ldr, long long strideR, const double* dZ, int zrows, int ldz,
                           long long strideZ, const double* drss, const int* djpvt, long long stridejpvt)
{
    qr_lm_batched* h = of_kind(lm, 0);
    if (!h || !dR || !dZ || bad_block(h->n, h->n, ldr, strideR) || zrows < h->n || bad_block(zrows, 1, ldz, strideZ) ||
        (djpvt && stridejpvt < h->n) || h->phase != LM_AT_X)
        return QR_E_ARG;
    h->phase = LM_STEPPED;
    if (h->batch == 0) return 0;
    qrd_bd_args d;
    memset(&d, 0, sizeof d);
    d.R = dR; d.ldr = ldr; d.sR = (size_t) strideR;
    d.Z = dZ; d.ldz = ldz; d.sZ = (size_t) strideZ; d.zrows = zrows;
    d.rss = drss;
    d.jpvt = djpvt; d.sj = (size_t) stridejpvt;
    return lm_step_launch(h, d);
}

int qr_lm_batched_update_dev(qr_lm_batched* h, const double* dFtrial, int ldf, long long strideF)
{
    return lm_update(of_kind(h, 0), dFtrial, ldf, strideF);
}

int qr_lm_batched_view(qr_lm_batched* lm, qr_lm_batched_state* v)
{
    const qr_lm_batched* h = of_kind(lm, 0);
    if (!h || !v) return QR_E_ARG;
    VIEW_8M(v, &h->s.b);
    return 0;
}

int qr_lm_batched_running(qr_lm_batched* h, int* count) { return lm_running(of_kind(h, 0), count); }

int qr_lstsq_lm_batched(qr_lm_fcn fcn, void* user, int m, int n, int batch, double* X, const double* D, const qr_lm_options* opt, double* fnorm,
                        int* nfev, int* njev, int* status, int* info)
{
    return lm_solve(0, fcn, user, m, n, batch, X, NULL, NULL, D, opt, fnorm, nfev, njev, status, info);
}

/* ---- section 8n: a qr_lmb_batched is the same struct with the flag set ---- */
int qr_lmb_batched_create(qr_lmb_batched** out, qr_plan* p, int m, int n, int batch, const qr_lm_options* opt)
{
    return lm_create((qr_lm_batched**) out, p, m, n, batch, opt, 1);
}

int qr_lmb_batched_destroy(qr_lmb_batched* h) { return lm_destroy(of_kind(h, 1)); }

int qr_lmb_batched_start_dev(qr_lmb_batched* h, const double* dX0, int ldx, long long strideX, const double* dD0, long long strideD,
                             const double* dLo, long long strideLo, const double* dHi, long long strideHi)
{
    return lm_start(of_kind(h, 1), dX0, ldx, strideX, dD0, strideD, dLo, strideLo, dHi, strideHi);
}

int qr_lmb_batched_step_dev(qr_lmb_batched* h, double* dJ, int ldj, long long strideJ, double* dF, int ldf, long long strideF)
{
    return lm_step(of_kind(h, 1), dJ, ldj, strideJ, dF, ldf, strideF);
}

int qr_lmb_batched_update_dev(qr_lmb_batched* h, const double* dFtrial, int ldf, long long strideF)
{
    return lm_update(of_kind(h, 1), dFtrial, ldf, strideF);
}

int qr_lmb_batched_view(qr_lmb_batched* lm, qr_lmb_batched_state* v)
{
    const qr_lm_batched* h = of_kind(lm, 1);
    if (!h || !v) return QR_E_ARG;
    VIEW_8M(v, &h->s.b);
    v->lo = h->s.lo; v->hi = h->s.hi; v->alpha = h->s.alpha; v->peg = h->s.peg; v->clipped = h->s.clipped;
    return 0;
}

int qr_lmb_batched_running(qr_lmb_batched* h, int* count) { return lm_running(of_kind(h, 1), count); }

int qr_lstsq_lm_bounded_batched(qr_lm_fcn fcn, void* user, int m, int n, int batch, double* X, const double* lo, const double* hi,
                                const double* D, const qr_lm_options* opt, double* fnorm, int* nfev, int* njev, int* status, int* info)
{
    return lm_solve(1, fcn, user, m, n, batch, X, lo, hi, D, opt, fnorm, nfev, njev, status, info);
}
