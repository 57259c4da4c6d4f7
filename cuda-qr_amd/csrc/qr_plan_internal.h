/* qr_plan_internal.h -- what the host-layer translation units share and the public header does not show: the layout of a
 * qr_plan, and the plan cache of the host-pointer entry points (qr_host.c) that qr_solve.c's qr_lstsq uses as well.
 * Internal: not installed, not part of the ABI. */
#ifndef QR_PLAN_INTERNAL_H
#define QR_PLAN_INTERNAL_H
#include <stddef.h>
#include "../../include/mi355x_qr.h"

#define QR_MAX_PAIRS 4
struct qr_plan {
    int m, n, nb, ib, ldv, ldt;
    int use_graph;              /* 1: qr_geqrf_dev is captured into a hipGraph once per argument set and replayed */
    void* graph_exec;
    double *g_dA, *g_dtau; int g_m, g_n, g_lda;
    int lookahead;              /* 1: panel k+1 is factored on `stream` while `stream_u` updates the rest */
    void* stream;               /* stream the next launch of the critical path goes to: s_main outside qr_geqrf_dev,
                                 * the current phase's panel stream inside it */
    void* stream_u;             /* wide trailing-update stream of the current phase */
    void* s_main;               /* the plan's public stream: all compute units */
    /* CU partition phases: while more than until[i] of the columns remain, the panel chain owns cus[i] compute
     * units (s_pair[i][0]) and the wide update the rest (s_pair[i][1]).  npairs = 0: no partition. */
    int npairs, pair_cur;
    void* s_pair[QR_MAX_PAIRS][2];
    int pair_shared_u[QR_MAX_PAIRS];   /* phase i's update stream is phase i-1's (not owned: never destroyed / synchronised twice) */
    double pair_until[QR_MAX_PAIRS];
    void* ev_hop[2];
    void* ev_extra[2];          /* panel-stream share of wide update s finished */
    double *We, *Ye;            /* its W buffer and raw V^T A2 */
    double *Ye2;                /* raw V^T A2 of a wide update that applies T to the small product (tall-skinny plans) */
    int m_user, n_user;         /* the shape the plan was asked for; m x n (>= it) is what it factors: see padA */
    double* pad_tau;            /* n scalars of the padded factorisation (the caller's dtau has n_user) */
    int pad_failed;             /* the lazy allocation of padA failed once: do not try again */
    double* padA;               /* (m x n, ld m) heights that are not multiples of 16: qr_geqrf_dev factors a copy with zero rows appended */
    double *Yn;                 /* raw V^T A_next of the look-ahead update */
    double bal_rp, bal_ru, bal_tc0, bal_tc1;   /* load-balance model (TFLOP/s, ms); bal_rp = 0: off */
    double bal_tail_tc;         /* chain time where the next panel is ONE launch (see chain_ms); 0: the linear model everywhere */
    double bal_tc0_base, bal_tc1_base; int bal_auto;   /* bal_auto: no MI355XQR_BALANCE override -- rates follow the phase's partition */
    void* ev_half[2];           /* W_a(s): the wide update has finished the columns of panel s+1 that N(s) left out (its second half) */
    void* ev_next[2];           /* look-ahead update N(s) of the next panel's columns finished (when it runs on the update stream) */
    int next_on_update;         /* 1: N(s) runs on the update stream's CUs, ahead of W(s); 0: on the panel stream; 2: on the panel
                                 * stream while the factorisation is update-bound, on the update stream once it is chain-bound */
    void* ev_panel[2];          /* panel set s ready (V, T, VT) */
    void* t_wait;               /* see apply_small_t */
    void* ev_v[2];              /* V of panel set s complete (its T merge still running): the long-K product of N(s) may start */
    void* v_ready;              /* event factor_panel records before the T merge of a one-level panel (NULL: none) */
    int defer_hint, t_deferred; /* defer_hint (set by the caller for ONE factor_panel call): behind a one-launch panel leave the Gram matrix and the
                                 * T merge to the caller (deferred_t_merge, on the update stream: 224 compute units instead of the panel stream's 32);
                                 * t_deferred: factor_panel did so */
    void* ev_wide[2];           /* wide update that read panel set s finished */
    void* ev_tree[2];           /* the merge tree of panel set s that ran BEHIND N(s) on the update stream has finished with G and X */
    double *Vw, *VT, *T;        /* current panel set (aliases of set[cur]) */
    double *Vw2[2], *VT2[2], *T2[2];
    int vt_formed[2];           /* VT2[e] = Vw2[e] * T2[e] of the panel NOW in set e exists (cleared when a panel is factored into the set,
                                 * set where the V*T product is issued): a slice of the wide update that needs it forms it on demand */
    double *W, *Wn, *Tt, *G, *X, *slabs, *slabs_u, *panel_ws;
    double* slabs_ep;           /* split-K slabs of the leaf's early product: written while the reconstruction still reads p->slabs */
    size_t slab_ep_cap;
    int panel_tsqr;             /* 1: Householder-TSQR leaf alone (MI355XQR_PANEL=tsqr); 3: CholeskyQR2 + Householder reconstruction, guarded by (1) */
    double* chol_ws;
    double* cq_ws; int* cq_status;   /* small-factor workspace and guard words of the full-width tall panel (qr_panel_cqr.hip); NULL: not used */
    /* "parked" full-width panels (round 5): on single-stream plans whose next update applies T to the small product (tall shapes) the panel's
     * V is written once, into the caller's array -- top block included, as the unit lower triangle -- and the update reads it from there;
     * R of the top block waits in the workspace and is put back right after that update (cq_unpark).  park_hint: set by the caller of
     * factor_panel for ONE call (it knows what follows the panel); cq_parked: the panel in cq_park_top is in that state now */
    int park_hint, cq_parked, cq_park_lda, cq_park_w;
    double* cq_park_top;
    unsigned *cq_hword, *cq_hword_dev;   /* host word (mapped into the device) that receives a tall panel's verdict as soon as it exists */
    unsigned cq_seq;            /* sequence number of the last tall panel issued */
    int guard_latch;            /* 0: a refused tall panel is handed to the leaf chain (the host reads the verdict while the panel's last pass
                                 * runs); 1: nothing is read inside qr_geqrf_dev, a refusal is reported by qr_plan_sync (QR_E_REFUSED) */
    int cq_dirty, pf_dirty;     /* tall panels in LATCH mode / one-launch panels have been issued since the status words were last read (a tall
                                 * panel in poll mode has its verdict read at once: nothing is left pending) */
    int fused_off;              /* 1: never the one-launch panel (set by the host-pointer entry points after a stalled hand-off, QR_E_STALL) */
    long long n_cqr, n_cqr_refused, n_pf_leaf_fallback, n_pf_stall;   /* qr_plan_route_stats */
    long long n_cqr_retried, n_cqr_retry_ok;                          /* qr_plan_retry_stats: refused panels retried preconditioned / accepted then */
    double* pf_ws;              /* exchange workspace of the one-launch panel (qr_panel_fused.hip); NULL: not used */
    unsigned pf_epoch;          /* its epoch counter: the workspace's epoch words never exceed it */
    int* pf_status;             /* device: [0] leaves that took the Householder route inside a one-launch panel, [1] a wait timed out */
    size_t slab_cap, w_cap;
    /* profiling */
    int prof_on, prof_mask, prof_count, prof_cap, prof_open, prof_paused;
    void** prof_ev;             /* 2 events per record */
    void* prof_stream;          /* stream of the open record */
    int* prof_cls;
    double *prof_flops, *prof_bytes;
    /* column pivoting (qr_pivot.c): allocated on the first pivoted call, freed with the plan */
    double* pv_d;               /* F, its transpose, gemv partials, partial norms, pivot candidates (qrd_pivot_ws_bind) */
    int* pv_i;                  /* flags, candidate indices, the panel-length word */
    double* pv_scatter;         /* n x nrhs: X in the caller's column order (qr_gelsp_dev) */
    size_t pv_scatter_cap;
    /* Jacobi SVD (qr_svd.c): allocated on the first call of header section 7 (sized for the plan's n), freed with the plan */
    double* sv_d;               /* R^T (n x n), the accumulated rotations (n x n), unsorted values (n), one slot per block pair, the sweep's word */
    int* sv_i;                  /* the block pairs of a sweep, the sort permutation */
    int* sv_h;                  /* host image of sv_i (the copies are asynchronous: it has to outlive the call) */
    double* sv_t;               /* 2 x (n x nrhs): Z^T c and its scaled copy (qr_gelss_dev) */
    size_t sv_t_cap;
    /* signed-row update (qr_downdate.c): allocated on the first call of header section 6b, freed with the plan */
    int* hd_status;             /* device word: 0, or the column + 1 at which a removal left no positive-definite triangle */
};

/* the least-squares accumulator (qr_update.c; qr_downdate.c removes rows from it).  One device allocation: R (n x n), Rc (n x n: a
 * chunk's triangle with explicit zeros below it), Z (n x nrhs), T (32 x n), tau (n), ssq (nrhs).  dd_buf: the workspace of pop / slide,
 * allocated on their first call: copies of R, Z and ssq, and a block of at most QRD_TP_MAXROWS stacked rows with its right-hand sides */
struct qr_lsacc {
    qr_plan* p;
    int n, nrhs;
    long long rows;
    double *buf, *R, *Rc, *Z, *T, *tau, *ssq;
    double* dd_buf;
};

/* the batched accumulator (qr_batched_update.c; qr_batched_damped.c solves from it): per member R (n x n, ld n), Z (n x nrhs, ld n), rss
 * (nrhs) and one row count, all on the device */
struct qr_lsacc_batched {
    qr_plan* p;
    int n, nrhs, batch;
    double *R, *Z, *rss;         /* one allocation */
    int* rows;
};

/* a cached plan of the host-pointer entry points and its device buffers (qr_host.c) */
typedef struct host_slot {
    int used, busy, cached, dev, m, n, nb;
    unsigned long long stamp;
    qr_plan* p;
    double *dA, *dtau, *dQ, *dR;
    size_t q_cap, r_cap;            /* doubles */
} host_slot;

/* a slot whose plan fits (m, n) exactly (cached, or `priv` filled as a one-shot slot); give it back with qr_host_slot_release */
int qr_host_slot_acquire(int m, int n, host_slot* priv, host_slot** out);
void qr_host_slot_release(host_slot* sl);
/* grows a device buffer of a slot to `elems` doubles (contents lost) */
int qr_host_slot_need(double** buf, size_t* cap, size_t elems);
/* grows the plan's W buffer to `elems` doubles: drains the plan when it allocates */
int qr_plan_ensure_w(qr_plan* p, size_t elems);

#endif
