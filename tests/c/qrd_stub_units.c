/* qrd_stub_units.c -- TEST-ONLY, included at the end of qrd_stub.c (it uses its helpers: op_begin, chk, chkb): the device layer of the
 * seventeen per-interface host units, qr_solve.c down to qr_batched_lm.c.  As everywhere in the stub a launch computes nothing.  Each entry
 *   returns -7 (or 0 for an empty launch) on exactly the conditions of the real launcher's extern "C" function,
 *   calls op_begin, and
 *   checks every operand block with the extent and the read / write tag qr_device.h documents; a batched operand is checked for its first
 *   and its last member, and its member stride against the block's extent (a stride of 0 is taken only where the contract shares it).
 * The pure sizing and route functions are restated here; tests/test_units_stub.py compares them with the product's over their whole grid.
 *
 * Scripted device words (the driver's hooks; without them every word stays as the stub's calloc left it, or at the value that ends a loop):
 *   qrd_stub_script(entry, values, n)   a queue per entry; "jsvd_fold": word[0] of the next calls; "jsvd_colnorms": the norms of the next
 *                                       call; "pivot_norms", "pivot_column": *pend after the call; "th_panel": *status (where it is still
 *                                       0); "blm_update", "blmb_update": v members keep running (status 0), the others finish (status 1;
 *                                       v < 0: |v| keep running after a rejected step); "blmb_start": the first v members are refused
 *                                       (info -2, nothing else of them written)
 *   qrd_stub_set_diag(d)                qrd_tp_panel / qrd_th_panel leave d on the diagonal of the triangle (0: untouched)
 *   qrd_stub_set_info(v)                every batched launch that owns info words writes v into them (0: untouched)
 *   qrd_stub_guard(p, bytes)            a write-tagged operand that meets [p, p + bytes) aborts (NULL: off) */
#include <limits.h>

static void misuse(const char* what, const char* why) { fprintf(stderr, "qrd_stub: %s: %s\n", what, why); abort(); }

#define NSCRIPT 12
static struct { const char* entry; double v[128]; int n, at; } g_script[NSCRIPT];
static pthread_mutex_t g_smu = PTHREAD_MUTEX_INITIALIZER;
static double g_diag;
static int g_info;
void qrd_stub_script(const char* entry, const double* v, int n)
{
    pthread_mutex_lock(&g_smu);
    int k = 0;
    while (k < NSCRIPT && g_script[k].entry && strcmp(g_script[k].entry, entry)) ++k;
    if (k == NSCRIPT || n > 128) misuse(entry, "script table full");
    g_script[k].entry = entry; g_script[k].n = n; g_script[k].at = 0;
    if (n > 0) memcpy(g_script[k].v, v, sizeof(double) * (size_t) n);
    pthread_mutex_unlock(&g_smu);
}
static int script_take(const char* entry, double* v)
{
    int got = 0;
    pthread_mutex_lock(&g_smu);
    for (int k = 0; k < NSCRIPT && g_script[k].entry; ++k)
        if (!strcmp(g_script[k].entry, entry) && g_script[k].at < g_script[k].n) { *v = g_script[k].v[g_script[k].at++]; got = 1; }
    pthread_mutex_unlock(&g_smu);
    return got;
}
void qrd_stub_set_diag(double d) { g_diag = d; }
void qrd_stub_set_info(int v) { g_info = v; }

/* `batch` column-major blocks rows x cols (leading dimension ld) at base + q * stride doubles */
static void chks(const char* what, const double* base, size_t stride, long ld, long rows, long cols, int batch, int mode, int shared_ok)
{
    if (rows <= 0 || cols <= 0 || batch <= 0) return;
    if (!base) die(what, base, 0);
    if (stride == 0 && shared_ok) { chk(what, base, ld, rows, cols, mode); return; }
    if (batch > 1 && stride < (size_t) (cols - 1) * (size_t) ld + (size_t) rows) misuse(what, "member stride shorter than the block");
    chk(what, base, ld, rows, cols, mode);
    if (batch > 1) chk(what, base + (size_t) (batch - 1) * stride, ld, rows, cols, mode);
}
/* len doubles per member */
static void chkv(const char* what, const double* base, size_t stride, long len, int batch, int mode, int shared_ok)
{ chks(what, base, stride, len, len, 1, batch, mode, shared_ok); }
/* len ints per member */
static void chki(const char* what, const int* base, size_t stride, long len, int batch, int mode)
{
    if (len <= 0 || batch <= 0) return;
    if (!base) die(what, base, 0);
    if (batch > 1 && stride < (size_t) len) misuse(what, "member stride shorter than the block");
    chkb(what, base, sizeof(int) * (size_t) len, mode);
    if (batch > 1) chkb(what, base + (size_t) (batch - 1) * stride, sizeof(int) * (size_t) len, mode);
}
/* the info words of a batched launch: `per` per member, packed */
static void info_out(int* info, int per, int batch)
{
    chkb("info", info, sizeof(int) * (size_t) per * (size_t) batch, WR);
    if (g_info) for (long i = 0; i < (long) per * batch; ++i) info[i] = g_info;
}

/* ---- qr_solve.hip ---- */
int qrd_ormqr_skinny_blocks(int mk, int* rpb)
{
    int r = (mk + 255) / 256;
    r = (r + 15) / 16 * 16;
    if (r < 64) r = 64;
    if (rpb) *rpb = r;
    return (mk + r - 1) / r;
}
size_t qrd_ormqr_skinny_ws(int m, int w, int nrhs)
{
    const int b = (m + 63) / 64;
    const size_t nblk = (size_t) (b < 256 ? b : 256);
    return (nblk + 1) * (size_t) w * (size_t) nrhs;
}
int qrd_ormqr_skinny(void* s, const double* Ak, int lda, int mk, int w, const double* T, int ldt, int trans_t, double* Cs, int ldc, int nrhs,
                     double* ws)
{
    (void) trans_t;
    if (mk < 1 || w < 1 || w > QRD_SOLVE_MAX_W || w > mk || nrhs < 1) return -7;
    op_begin(s, "ormqr_skinny");
    const int nblk = qrd_ormqr_skinny_blocks(mk, NULL);
    chk("ormqr_skinny V", Ak, lda, mk, w, RD); chk("ormqr_skinny T", T, ldt, w, w, RD); chk("ormqr_skinny C", Cs, ldc, mk, nrhs, RW);
    chkb("ormqr_skinny ws", ws, sizeof(double) * (size_t) (nblk + 1) * (size_t) w * (size_t) nrhs, WR);
    return 0;
}
int qrd_trsm_step(void* s, const double* R, int lda, double* B, int ldb, int nrhs, int row_lo, int l0, int l1, int x0, int x1)
{
    if (l1 - l0 < 1 || l1 - l0 > 64 || x1 - x0 < 0 || x1 - x0 > 64 || row_lo > l0 || nrhs < 1) return -7;
    op_begin(s, "trsm_step");
    chk("trsm_step R diag", R + (size_t) l0 * lda + l0, lda, l1 - l0, l1 - l0, RD);
    if (x1 > x0) { chk("trsm_step R off", R + (size_t) x0 * lda + row_lo, lda, l1 - row_lo, x1 - x0, RD); chk("trsm_step B x", B + x0, ldb, x1 - x0, nrhs, RD); }
    chk("trsm_step B", B + row_lo, ldb, l1 - row_lo, nrhs, RW);
    return 0;
}

/* ---- qr_minnorm.hip ---- */
int qrd_trsm_t_step(void* s, const double* R, int lda, double* B, int ldb, int nrhs, int row_hi, int l0, int l1, int x0, int x1)
{
    if (l1 - l0 < 1 || l1 - l0 > 64 || x0 < 0 || x1 - x0 < 0 || x1 - x0 > 64 || x1 > l0 || row_hi < l1 || nrhs < 1) return -7;
    op_begin(s, "trsm_t_step");
    chk("trsm_t_step R diag", R + (size_t) l0 * lda + l0, lda, l1 - l0, l1 - l0, RD);
    if (x1 > x0) { chk("trsm_t_step R off", R + (size_t) l0 * lda + x0, lda, x1 - x0, row_hi - l0, RD); chk("trsm_t_step B x", B + x0, ldb, x1 - x0, nrhs, RD); }
    chk("trsm_t_step B", B + l0, ldb, row_hi - l0, nrhs, RW);
    return 0;
}
/* (a data mover, like qrd_copy_block: the wide solve's factor array is the transpose of what the caller uploaded) */
int qrd_transpose_tiled(void* s, int rows, int cols, const double* S, int lds, double* D, int ldd)
{
    if (rows <= 0 || cols <= 0) return 0;
    if ((long long) ((rows + 63) / 64) * ((cols + 63) / 64) > 0x7fffffffLL) return -7;
    op_begin(s, "transpose_tiled");
    chk("transpose_tiled S", S, lds, rows, cols, RD); chk("transpose_tiled D", D, ldd, cols, rows, WR);
    for (int c = 0; c < cols; ++c)
        for (int r = 0; r < rows; ++r) D[(size_t) r * ldd + c] = S[(size_t) c * lds + r];
    return 0;
}

/* ---- qr_update.hip, qr_downdate.hip ---- */
static void put_diag(double* Rkk, int ldr, int w) { if (g_diag != 0.0) for (int i = 0; i < w; ++i) Rkk[(size_t) i * ldr + i] = g_diag; }
int qrd_tp_panel(void* s, double* Rkk, int ldr, double* Bk, int ldb, int p, int w, double* Tk, int ldt)
{
    if (p < 1 || p > QRD_TP_MAXROWS || w < 1 || w > QRD_TP_W || ldr < w || ldb < p || ldt < w) return -7;
    op_begin(s, "tp_panel");
    chk("tp_panel R", Rkk, ldr, w, w, RW); chk("tp_panel B", Bk, ldb, p, w, RW); chk("tp_panel T", Tk, ldt, w, w, WR);
    put_diag(Rkk, ldr, w);
    return 0;
}
int qrd_tp_apply(void* s, int trans_t, const double* Vk, int ldv, int p, int w, const double* Tk, int ldt, double* C1k, int ldc1, double* C2,
                 int ldc2, int ncols)
{
    (void) trans_t;
    if (ncols <= 0) return 0;
    if (p < 1 || p > QRD_TP_MAXROWS || w < 1 || w > QRD_TP_W || ldv < p || ldt < w || ldc1 < w || ldc2 < p) return -7;
    op_begin(s, "tp_apply");
    chk("tp_apply V", Vk, ldv, p, w, RD); chk("tp_apply T", Tk, ldt, w, w, RD); chk("tp_apply C1", C1k, ldc1, w, ncols, RW);
    chk("tp_apply C2", C2, ldc2, p, ncols, RW);
    return 0;
}
int qrd_tp_colssq_add(void* s, const double* X, int ldx, int rows, int cols, double* acc)
{
    if (rows <= 0 || cols <= 0) return 0;
    op_begin(s, "tp_colssq_add");
    chk("tp_colssq X", X, ldx, rows, cols, RD); chk("tp_colssq acc", acc, cols, cols, 1, RW);
    return 0;
}
int qrd_tp_sqrt(void* s, const double* in, double* out, int n)
{
    if (n <= 0) return 0;
    op_begin(s, "tp_sqrt");
    chk("tp_sqrt in", in, n, n, 1, RD); chk("tp_sqrt out", out, n, n, 1, WR);
    return 0;
}
/* every launch of the signed-row family reads the status word first and returns at once when it is not 0 */
static int th_failed(const int* status) { chkb("th status", status, sizeof(int), RD); return *status != 0; }
int qrd_th_panel(void* s, double* Rkk, int ldr, double* Bk, int ldb, int p, int p_add, int w, double* Tk, int ldt, int col0, int* status)
{
    if (p < 1 || p > QRD_TP_MAXROWS || p_add < 0 || p_add > p || w < 1 || w > QRD_TP_W || ldr < w || ldb < p || ldt < w || col0 < 0 || !status)
        return -7;
    op_begin(s, "th_panel");
    if (th_failed(status)) return 0;
    double v = 0.0;
    if (script_take("th_panel", &v) && v != 0.0) {      /* the column that fails: nothing is written back but the word */
        chk("th_panel R", Rkk, ldr, w, w, RD); chk("th_panel B", Bk, ldb, p, w, RD); chkb("th status", status, sizeof(int), WR);
        *status = (int) v;
        return 0;
    }
    chk("th_panel R", Rkk, ldr, w, w, RW); chk("th_panel B", Bk, ldb, p, w, RW); chk("th_panel T", Tk, ldt, w, w, WR);
    put_diag(Rkk, ldr, w);
    return 0;
}
int qrd_th_apply(void* s, const double* Vk, int ldv, int p, int p_add, int w, const double* Tk, int ldt, double* C1k, int ldc1, double* C2,
                 int ldc2, int ncols, const int* status)
{
    if (ncols <= 0) return 0;
    if (p < 1 || p > QRD_TP_MAXROWS || p_add < 0 || p_add > p || w < 1 || w > QRD_TP_W || ldv < p || ldt < w || ldc1 < w || ldc2 < p || !status)
        return -7;
    op_begin(s, "th_apply");
    if (th_failed(status)) return 0;
    chk("th_apply V", Vk, ldv, p, w, RD); chk("th_apply T", Tk, ldt, w, w, RD); chk("th_apply C1", C1k, ldc1, w, ncols, RW);
    chk("th_apply C2", C2, ldc2, p, ncols, RW);
    return 0;
}
int qrd_th_colssq(void* s, const double* X, int ldx, int p, int p_add, int cols, double* acc, const int* status)
{
    if (cols <= 0) return 0;
    if (p < 1 || p > QRD_TP_MAXROWS || p_add < 0 || p_add > p || ldx < p || !status) return -7;
    op_begin(s, "th_colssq");
    if (th_failed(status)) return 0;
    chk("th_colssq X", X, ldx, p, cols, RD); chk("th_colssq acc", acc, cols, cols, 1, RW);
    return 0;
}

/* ---- qr_svd.hip ---- */
int qrd_jsvd_round(void* s, double* G, int ldg, int r, int n, double* V, int ldv, const int* pairs, int npairs, double tol, double* slots)
{
    (void) tol;
    if (npairs <= 0) return 0;
    if (r < 1 || n < 1 || ldg < r || (V && ldv < n) || !pairs || !slots) return -7;
    op_begin(s, "jsvd_round");
    chk("jsvd_round G", G, ldg, r, n, RW);
    if (V) chk("jsvd_round V", V, ldv, n, n, RW);
    chkb("jsvd_round pairs", pairs, sizeof(int) * 2 * (size_t) npairs, RD); chk("jsvd_round slots", slots, npairs, npairs, 1, WR);
    const int nblk = (n + QRD_JSVD_BLOCK - 1) / QRD_JSVD_BLOCK;
    for (int i = 0; i < 2 * npairs; ++i) if (pairs[i] < 0 || pairs[i] >= nblk) misuse("jsvd_round", "a pair names a column block past the matrix");
    return 0;
}
int qrd_jsvd_fold(void* s, const double* slots, int count, double* word)
{
    op_begin(s, "jsvd_fold");
    chk("jsvd_fold slots", slots, count, count, 1, RD); chk("jsvd_fold word", word, 1, 1, 1, WR);
    double v = 0.0;
    word[0] = script_take("jsvd_fold", &v) ? v : 0.0;
    return 0;
}
int qrd_jsvd_colnorms(void* s, const double* G, int ldg, int r, int n, double* out)
{
    if (r <= 0 || n <= 0) return 0;
    op_begin(s, "jsvd_colnorms");
    chk("jsvd_colnorms G", G, ldg, r, n, RD); chk("jsvd_colnorms out", out, n, n, 1, WR);
    double v = 0.0;
    for (int i = 0; i < n && script_take("jsvd_colnorms", &v); ++i) out[i] = v;
    return 0;
}
int qrd_jsvd_gather(void* s, const double* sig, const int* perm, double* out, int n)
{
    if (n <= 0) return 0;
    op_begin(s, "jsvd_gather");
    chk("jsvd_gather sig", sig, n, n, 1, RD); chkb("jsvd_gather perm", perm, sizeof(int) * (size_t) n, RD); chk("jsvd_gather out", out, n, n, 1, WR);
    return 0;
}
int qrd_jsvd_permute(void* s, double* M, int ld, int rows, int n, const int* perm)
{
    if (rows <= 0 || n <= 0) return 0;
    op_begin(s, "jsvd_permute");
    chk("jsvd_permute M", M, ld, rows, n, RW); chkb("jsvd_permute perm", perm, sizeof(int) * (size_t) n, RD);
    for (int j = 0; j < n; ++j) if ((perm[j] & (QRD_JSVD_LEAD - 1)) >= n) misuse("jsvd_permute", "perm names a column past the matrix");
    return 0;
}
int qrd_jsvd_normalise(void* s, double* G, int ldg, int r, int n, const double* sig)
{
    if (r <= 0 || n <= 0) return 0;
    op_begin(s, "jsvd_normalise");
    chk("jsvd_normalise G", G, ldg, r, n, RW); chk("jsvd_normalise sig", sig, n, n, 1, RD);
    return 0;
}
int qrd_jsvd_pinv_scale(void* s, const double* T1, double* T2, int n, int nrhs, const double* sig, double rc)
{
    (void) rc;
    if (n <= 0 || nrhs <= 0) return 0;
    op_begin(s, "jsvd_pinv_scale");
    chk("jsvd_pinv T1", T1, n, n, nrhs, RD); chk("jsvd_pinv T2", T2, n, n, nrhs, WR); chk("jsvd_pinv sig", sig, n, n, 1, RD);
    return 0;
}
int qrd_jsvd_rt(void* s, const double* A, int lda, int n, double* W, int ldw)
{
    if (n <= 0) return 0;
    op_begin(s, "jsvd_rt");
    chk("jsvd_rt A", A, lda, n, n, RD); chk("jsvd_rt W", W, ldw, n, n, WR);
    return 0;
}

/* ---- qr_pivot.hip ---- */
static int pivot_ld(int n) { return (n + 1) & ~1; }
static int pivot_ncb(int n) { return (n + 255) / 256; }
size_t qrd_pivot_ws_doubles(int n)
{
    const size_t ld = (size_t) pivot_ld(n);
    return ld * (2 * QRD_PIVOT_NBP + 2 + QRD_PIVOT_MAX_SPLIT) + 256 + (size_t) pivot_ncb(n) + 2;
}
size_t qrd_pivot_ws_ints(int n) { return (size_t) n + (size_t) pivot_ncb(n) + 2; }
void qrd_pivot_ws_bind(qrd_pivot_ws* w, int n, double* d, int* i)
{
    const size_t ld = (size_t) pivot_ld(n);
    w->ldf = (int) ld;
    w->F = d; d += ld * QRD_PIVOT_NBP;
    w->FT = d; d += ld * QRD_PIVOT_NBP;
    w->P = d; d += ld * QRD_PIVOT_MAX_SPLIT;
    w->vn1 = d; d += ld;
    w->vn2 = d; d += ld;
    w->npart = d; d += 256;
    w->alpha = d; d += 2;
    w->cval = d;
    w->flag = i; i += n;
    w->cidx = i; i += pivot_ncb(n);
    w->pend = i;
}
/* the small arrays every pivot launch works on: norms, flags, candidates, the panel-length words */
static void pivot_small(const qrd_pivot_ws* w, int n)
{
    chk("pivot vn1", w->vn1, n, n, 1, RW); chk("pivot vn2", w->vn2, n, n, 1, RW); chkb("pivot flag", w->flag, sizeof(int) * (size_t) n, RW);
    chk("pivot cval", w->cval, pivot_ncb(n), pivot_ncb(n), 1, RW); chkb("pivot cidx", w->cidx, sizeof(int) * (size_t) pivot_ncb(n), RW);
    chkb("pivot pend", w->pend, 2 * sizeof(int), RW);
}
int qrd_pivot_norms(void* s, const qrd_pivot_ws* w, const double* A, int lda, int m, int n, int r0, int c0, int all, int* jpvt)
{
    if (m < 1 || n < 1 || r0 < 0 || c0 < 0 || lda < m) return -7;
    op_begin(s, "pivot_norms");
    if (r0 < m && c0 < n) chk("pivot_norms A", A + (size_t) c0 * lda + r0, lda, m - r0, n - c0, RD);
    pivot_small(w, n);
    if (all) { chkb("pivot_norms jpvt", jpvt, sizeof(int) * (size_t) n, WR); for (int j = 0; j < n; ++j) jpvt[j] = j; }
    double v = 0.0;
    *w->pend = script_take("pivot_norms", &v) ? (int) v : INT_MAX;
    return 0;
}
int qrd_pivot_column(void* s, const qrd_pivot_ws* w, double* A, int lda, int m, int n, int k0, int j, int* jpvt, double* tau)
{
    const int c = k0 + j;
    if (m < n || n < 1 || k0 < 0 || j < 0 || j >= QRD_PIVOT_NBP || c >= n || lda < m) return -7;
    op_begin(s, "pivot_column");
    chk("pivot_column A", A, lda, m, n, RW); chk("pivot_column F", w->F, w->ldf, n, QRD_PIVOT_NBP, RW);
    chk("pivot_column P", w->P, w->ldf, n, QRD_PIVOT_MAX_SPLIT, WR); chk("pivot_column npart", w->npart, 256, 256, 1, WR);
    chk("pivot_column alpha", w->alpha, 2, 2, 1, WR);
    pivot_small(w, n);
    chkb("pivot_column jpvt", jpvt, sizeof(int) * (size_t) n, RW); chk("pivot_column tau", tau + c, 1, 1, 1, WR);
    double v = 0.0;
    if (script_take("pivot_column", &v)) *w->pend = (int) v;
    return 0;
}
int qrd_pivot_scatter(void* s, const double* B, int ldb, int n, int nrhs, int r, const int* jpvt, double* S)
{
    if (n < 1 || nrhs < 1 || r < 0 || r > n || ldb < n) return -7;
    op_begin(s, "pivot_scatter");
    chk("pivot_scatter B", B, ldb, n, nrhs, RD); chkb("pivot_scatter jpvt", jpvt, sizeof(int) * (size_t) n, RD); chk("pivot_scatter S", S, n, n, nrhs, WR);
    return 0;
}
int qrd_pivot_resid(void* s, const double* B, int ldb, int r0, int m, int nrhs, double* resid)
{
    if (nrhs < 1 || r0 < 0 || r0 > m || ldb < m) return -7;
    op_begin(s, "pivot_resid");
    chk("pivot_resid B", B + r0, ldb, m - r0, nrhs, RD); chk("pivot_resid out", resid, nrhs, nrhs, 1, WR);
    return 0;
}

/* ---- qr_batched.hip, qr_batched_svd.hip ---- */
#define STUB_LDS_CAP (160 * 1024)
#define STUB_WG_SMALL 72
static int sb_ld(int m) { return ((m + 29) / 32) * 32 + 2; }
int qrd_b_max_rows(int ncols) { return (ncols < 1 || ncols > QRD_B_MAX_N) ? 0 : (ncols <= 32 ? QRD_B_MAX_ROWS : QRD_B_MAX_ROWS / 2); }
int qrd_b_fits(int m, int ncols)
{
    return ncols >= 1 && ncols <= QRD_B_MAX_N && m >= 1 && m <= QRD_B_MAX_ROWS &&
           sizeof(double) * ((size_t) ncols * (size_t) sb_ld(m) + STUB_WG_SMALL) <= STUB_LDS_CAP;
}
int qrd_b_wave_route(int m, int ncols) { return m <= 64 && ncols <= 32; }
int qrd_b_geqrf(void* s, double* A, int m, int n, int lda, size_t sA, double* tau, size_t st, double* B, int nrhs, int ldb, size_t sB, int* info,
                int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || m < n || nrhs < 0 || !qrd_b_fits(m, n + nrhs) || lda < m || (nrhs && (!B || ldb < m || !info))) return -7;
    op_begin(s, "b_geqrf");
    chks("b_geqrf A", A, sA, lda, m, n, batch, RW, 0); chkv("b_geqrf tau", tau, st, n, batch, WR, 0);
    if (nrhs) { chks("b_geqrf B", B, sB, ldb, m, nrhs, batch, RW, 0); info_out(info, 1, batch); }
    return 0;
}
int qrd_b_ormqr(void* s, int trans_t, const double* A, int m, int n, int lda, size_t sA, const double* tau, size_t st, double* Cm, int nrhs, int ldc,
                size_t sC, int batch)
{
    (void) trans_t;
    if (batch <= 0) return 0;
    if (n < 1 || m < n || !qrd_b_fits(m, n) || lda < m || ldc < m || nrhs < 1) return -7;
    op_begin(s, "b_ormqr");
    chks("b_ormqr A", A, sA, lda, m, n, batch, RD, 0); chkv("b_ormqr tau", tau, st, n, batch, RD, 0); chks("b_ormqr C", Cm, sC, ldc, m, nrhs, batch, RW, 0);
    return 0;
}
int qrd_b_eye(void* s, double* Q, int m, int n, int ldq, size_t sQ, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || m < n || ldq < m) return -7;
    op_begin(s, "b_eye");
    chks("b_eye Q", Q, sQ, ldq, m, n, batch, WR, 0);
    return 0;
}
int qrd_b_trsm(void* s, const double* A, int n, int lda, size_t sA, double* B, int nrhs, int ldb, size_t sB, int* info, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || n > QRD_B_MAX_N || lda < n || ldb < n || nrhs < 1 || !info) return -7;
    op_begin(s, "b_trsm");
    chks("b_trsm A", A, sA, lda, n, n, batch, RD, 0); chks("b_trsm B", B, sB, ldb, n, nrhs, batch, RW, 0); info_out(info, 1, batch);
    return 0;
}
/* resid (nrhs per member, packed) and rank (one per member), where given */
static void piv_out(double* resid, int* rank, int nrhs, int batch)
{
    if (resid) chk("resid", resid, (long) nrhs * batch, (long) nrhs * batch, 1, WR);
    if (rank) chkb("rank", rank, sizeof(int) * (size_t) batch, WR);
}
int qrd_b_geqp3(void* s, double* A, int m, int n, int lda, size_t sA, int* jpvt, size_t sj, double* tau, size_t st, double* B, int nrhs, int ldb,
                size_t sB, double rcond, int minnorm, double* resid, int* rank, int batch)
{
    (void) rcond; (void) minnorm;
    if (batch <= 0) return 0;
    if (n < 1 || m < n || nrhs < 0 || !qrd_b_fits(m, n + nrhs) || lda < m || !jpvt || (nrhs && (!B || ldb < m))) return -7;
    op_begin(s, "b_geqp3");
    chks("b_geqp3 A", A, sA, lda, m, n, batch, RW, 0); chki("b_geqp3 jpvt", jpvt, sj, n, batch, WR); chkv("b_geqp3 tau", tau, st, n, batch, WR, 0);
    if (nrhs) { chks("b_geqp3 B", B, sB, ldb, m, nrhs, batch, RW, 0); piv_out(resid, rank, nrhs, batch); }
    return 0;
}
int qrd_b_rank(void* s, const double* A, int n, int lda, size_t sA, double rcond, int* rank, int batch)
{
    (void) rcond;
    if (batch <= 0) return 0;
    if (n < 1 || lda < n || !rank) return -7;
    op_begin(s, "b_rank");
    chks("b_rank A", A, sA, lda, n, n, batch, RD, 0); chkb("b_rank rank", rank, sizeof(int) * (size_t) batch, WR);
    return 0;
}
int qrd_b_solve_piv(void* s, const double* A, int m, int n, int lda, size_t sA, const int* jpvt, size_t sj, double* B, int nrhs, int ldb, size_t sB,
                    double rcond, int minnorm, double* resid, int* rank, int batch)
{
    (void) rcond; (void) minnorm;
    if (batch <= 0) return 0;
    if (n < 1 || n > QRD_B_MAX_N || m < n || lda < n || ldb < m || nrhs < 1 || !jpvt) return -7;
    op_begin(s, "b_solve_piv");
    chks("b_solve_piv A", A, sA, lda, n, n, batch, RD, 0); chki("b_solve_piv jpvt", jpvt, sj, n, batch, RD);
    chks("b_solve_piv B", B, sB, ldb, m, nrhs, batch, RW, 0); piv_out(resid, rank, nrhs, batch);
    return 0;
}
int qrd_b_jsvd(void* s, const double* A, int m, int n, int lda, size_t sA, const int* jpvt, size_t sj, double* S, size_t sS, double* U, int ldu,
               size_t sU, double* V, int ldv, size_t sV, int* rank, int* sweeps, int* info, int max_sweeps, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || n > QRD_B_MAX_N || m < n || m > QRD_B_MAX_ROWS || lda < m || !A || !jpvt || !S || !info || max_sweeps < 1 || (U && ldu < m) ||
        (V && ldv < n))
        return -7;
    op_begin(s, "b_jsvd");
    chks("b_jsvd A", A, sA, lda, m, n, batch, RD, 0); chki("b_jsvd jpvt", jpvt, sj, n, batch, RD); chkv("b_jsvd S", S, sS, n, batch, WR, 0);
    if (U) chks("b_jsvd U", U, sU, ldu, m, n, batch, WR, 0);
    if (V) chks("b_jsvd V", V, sV, ldv, n, n, batch, WR, 0);
    if (rank) chkb("b_jsvd rank", rank, sizeof(int) * (size_t) batch, WR);
    if (sweeps) chkb("b_jsvd sweeps", sweeps, sizeof(int) * (size_t) batch, WR);
    info_out(info, 1, batch);
    return 0;
}

/* ---- qr_batched_update.hip ---- */
int qrd_bu_max_rows(int ncols) { return (ncols < 1 || ncols > QRD_B_MAX_N) ? 0 : (ncols <= 32 ? QRD_BU_MAXROWS : QRD_BU_MAXROWS_WIDE); }
int qrd_bu_wave_route(int ncols, int p) { return ncols <= 32 && p <= 64; }
int qrd_bu_update(void* s, const qrd_bu_args* a)
{
    if (!a || a->batch <= 0) return 0;
    const int ntot = a->n + a->nrhs, p = a->p, pd = p - a->p_add, b = a->batch;
    if (a->n < 1 || a->nrhs < 0 || ntot > QRD_B_MAX_N || p < 1 || p > qrd_bu_max_rows(ntot) || a->p_add < 0 || a->p_add > p || !a->R ||
        a->ldr < a->n || (a->nrhs && (!a->Z || a->ldz < a->n)) || (a->acc ? (!a->rows || (a->nrhs && !a->rss)) : !a->tau) ||
        (!a->info && (a->p_add < p)))
        return -7;
    if (a->p_add > 0 && (!a->A0 || a->lda0 < a->p_add || (a->nrhs && (!a->C0 || a->ldc0 < a->p_add)))) return -7;
    if (a->p_add < p && (!a->A1 || a->lda1 < pd || (a->nrhs && (!a->C1 || a->ldc1 < pd)))) return -7;
    op_begin(s, "bu_update");
    const int blk = a->acc ? RD : RW;          /* the accumulator reads its block, the primitive leaves V and the transformed rows in it */
    chks("bu_update R", a->R, a->sR, a->ldr, a->n, a->n, b, RW, 0);
    if (a->nrhs) chks("bu_update Z", a->Z, a->sZ, a->ldz, a->n, a->nrhs, b, RW, 0);
    if (a->p_add > 0) { chks("bu_update A0", a->A0, a->sA0, a->lda0, a->p_add, a->n, b, blk, 0); if (a->nrhs) chks("bu_update C0", a->C0, a->sC0, a->ldc0, a->p_add, a->nrhs, b, blk, 0); }
    if (pd > 0) { chks("bu_update A1", a->A1, a->sA1, a->lda1, pd, a->n, b, blk, 0); if (a->nrhs) chks("bu_update C1", a->C1, a->sC1, a->ldc1, pd, a->nrhs, b, blk, 0); }
    if (a->acc) {
        if (a->nrhs) chk("bu_update rss", a->rss, (long) a->nrhs * b, (long) a->nrhs * b, 1, RW);
        chkb("bu_update rows", a->rows, sizeof(int) * (size_t) b, RW);
    } else chkv("bu_update tau", a->tau, a->stau, a->n, b, WR, 0);
    if (a->info) info_out(a->info, 1, b);
    return 0;
}
int qrd_bu_apply(void* s, int trans_t, const double* V, int p, int p_add, int n, int ldv, size_t sV, const double* tau, size_t st, double* C1, int ldc1,
                 size_t sC1, double* C2, int ldc2, size_t sC2, int nrhs, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || n > QRD_B_MAX_N || p < 1 || p > qrd_bu_max_rows(n) || p_add < 0 || p_add > p || (!trans_t && p_add != p) || ldv < p || ldc1 < n ||
        ldc2 < p || nrhs < 1)
        return -7;
    op_begin(s, "bu_apply");
    chks("bu_apply V", V, sV, ldv, p, n, batch, RD, 0); chkv("bu_apply tau", tau, st, n, batch, RD, 0);
    chks("bu_apply C1", C1, sC1, ldc1, n, nrhs, batch, RW, 0); chks("bu_apply C2", C2, sC2, ldc2, p, nrhs, batch, RW, 0);
    return 0;
}
int qrd_bu_solve_prep(void* s, const double* Z, int n, int nrhs, double* X, int ldx, size_t sX, const double* rss, double* resid, size_t sres, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || nrhs < 1 || ldx < n || !Z || !X || !rss) return -7;
    op_begin(s, "bu_solve_prep");
    chks("bu_solve_prep Z", Z, (size_t) n * nrhs, n, n, nrhs, batch, RD, 0); chks("bu_solve_prep X", X, sX, ldx, n, nrhs, batch, WR, 0);
    chk("bu_solve_prep rss", rss, (long) nrhs * batch, (long) nrhs * batch, 1, RD);
    if (resid) chkv("bu_solve_prep resid", resid, sres, nrhs, batch, WR, 0);
    return 0;
}

/* ---- qr_batched_minnorm.hip ---- */
int qrd_bm_fused(void* s, int tr, const double* A, int m, int n, int lda, size_t sA, double* F, int ldf, size_t sF, double* tau, size_t st, double* B,
                 int nrhs, int ldb, size_t sB, int* info, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || m < n || nrhs < 1 || !qrd_b_fits(m, n + nrhs) || lda < (tr ? n : m) || ldf < m || ldb < m || !A || !F || !tau || !B || !info) return -7;
    op_begin(s, "bm_fused");
    if (tr) chks("bm_fused A", A, sA, lda, n, m, batch, RD, 0);
    else chks("bm_fused A", A, sA, lda, m, n, batch, RD, 0);
    chks("bm_fused F", F, sF, ldf, m, n, batch, WR, 0); chkv("bm_fused tau", tau, st, n, batch, WR, 0);
    chks("bm_fused B", B, sB, ldb, m, nrhs, batch, RW, 0); info_out(info, 1, batch);
    return 0;
}
int qrd_bm_apply(void* s, const double* A, int m, int n, int lda, size_t sA, const double* tau, size_t st, double* B, int nrhs, int ldb, size_t sB,
                 int* info, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || m < n || !qrd_b_fits(m, n) || lda < m || ldb < m || nrhs < 1 || !A || !tau || !B || !info) return -7;
    op_begin(s, "bm_apply");
    chks("bm_apply A", A, sA, lda, m, n, batch, RD, 0); chkv("bm_apply tau", tau, st, n, batch, RD, 0);
    chks("bm_apply B", B, sB, ldb, m, nrhs, batch, RW, 0); info_out(info, 1, batch);
    return 0;
}
int qrd_bm_transpose(void* s, const double* S, int rows, int cols, int lds, size_t sS, double* D, int ldd, size_t sD, int batch)
{
    if (batch <= 0) return 0;
    if (rows < 1 || cols < 1 || rows > QRD_B_MAX_ROWS || cols > QRD_B_MAX_ROWS || lds < rows || ldd < cols || !S || !D) return -7;
    op_begin(s, "bm_transpose");
    chks("bm_transpose S", S, sS, lds, rows, cols, batch, RD, 0); chks("bm_transpose D", D, sD, ldd, cols, rows, batch, WR, 0);
    return 0;
}

/* ---- qr_batched_damped.hip, qr_batched_trust.hip ---- */
int qrd_bd_wave_route(int ncols) { return ncols >= 1 && ncols <= 32; }
static int bd_bad_args(const qrd_bd_args* a)
{
    return a->n < 1 || a->nrhs < 1 || a->n + a->nrhs > QRD_B_MAX_N || a->nlam < 1 || !a->Z || !a->lam || !a->X || !a->info || a->zrows < a->n ||
           a->xrows < a->n || a->ldz < a->zrows || a->ldx < a->xrows || (a->flip && (a->D || a->jpvt));
}
/* the operands every damped / trust / Levenberg-Marquardt launch shares: the factors (where they are inputs) and the weights */
static void bd_in(const qrd_bd_args* a, int factors)
{
    const int b = a->batch;
    if (factors) {
        chks("bd R", a->R, a->sR, a->ldr, a->n, a->n, b, RD, 0); chks("bd Z", a->Z, a->sZ, a->ldz, a->zrows, a->nrhs, b, RD, 0);
        if (a->rss) chk("bd rss", a->rss, (long) a->nrhs * b, (long) a->nrhs * b, 1, RD);
        if (a->jpvt) chki("bd jpvt", a->jpvt, a->sj, a->n, b, RD);
    }
    if (a->D) chkv("bd D", a->D, a->sD, a->n, b, RD, 1);
}
static void bd_out(const qrd_bd_args* a)
{
    const int b = a->batch;
    const long cols = (long) a->nlam * a->nrhs;
    chks("bd X", a->X, a->sX, a->ldx, a->xrows, cols, b, WR, 0);
    if (a->xnorm) chk("bd xnorm", a->xnorm, cols * b, cols * b, 1, WR);
    if (a->resid) chk("bd resid", a->resid, cols * b, cols * b, 1, WR);
    info_out(a->info, a->nlam, b);
}
int qrd_bd_solve(void* s, const qrd_bd_args* a)
{
    if (!a || a->batch <= 0) return 0;
    if (bd_bad_args(a) || !a->R || a->ldr < a->n) return -7;
    op_begin(s, "bd_solve");
    bd_in(a, 1); chkv("bd lam", a->lam, a->slam, a->nlam, a->batch, RD, 1); bd_out(a);
    return 0;
}
/* the factorisation in front of the fused launches: A, tau and all m rows of B */
static void fused_front(double* A, int m, int n, int lda, size_t sA, double* tau, size_t st, double* B, int nrhs, int ldz, size_t sZ, int batch)
{
    chks("fused A", A, sA, lda, m, n, batch, RW, 0); chkv("fused tau", tau, st, n, batch, WR, 0); chks("fused B", B, sZ, ldz, m, nrhs, batch, RW, 0);
}
int qrd_bd_fused(void* s, double* A, int m, int lda, size_t sA, double* tau, size_t st, double* B, const qrd_bd_args* a)
{
    if (!a || a->batch <= 0) return 0;
    qrd_bd_args b = *a;
    b.Z = B; b.zrows = b.n;
    if (bd_bad_args(&b) || !A || !tau || !B || m < a->n || m > 64 || !qrd_bd_wave_route(a->n + a->nrhs) || lda < m || a->ldz < m || a->R || a->rss ||
        a->jpvt || a->flip)
        return -7;
    op_begin(s, "bd_fused");
    fused_front(A, m, a->n, lda, sA, tau, st, B, a->nrhs, a->ldz, a->sZ, a->batch);
    bd_in(a, 0); chkv("bd lam", a->lam, a->slam, a->nlam, a->batch, RD, 1); bd_out(a);
    return 0;
}
static int bt_bad_args(const qrd_bt_args* a)
{
    const qrd_bd_args* d = &a->d;
    return d->n < 1 || d->n + 1 > QRD_B_MAX_N || d->nrhs != 1 || d->nlam != 1 || !d->Z || !d->X || !d->info || d->zrows < d->n || d->xrows < d->n ||
           d->ldz < d->zrows || d->ldx < d->xrows || (d->flip && (d->D || d->jpvt)) || !a->delta || !a->lam || !(a->rtol > 0.0 && a->rtol < 1.0) ||
           a->maxit < 1;
}
static void bt_io(const qrd_bt_args* a)
{
    const int b = a->d.batch;
    chkv("bt delta", a->delta, a->sdelta, 1, b, RD, 1);
    if (a->lam0) chkv("bt lam0", a->lam0, a->slam0, 1, b, RD, 1);
    chk("bt lam", a->lam, b, b, 1, WR);
    if (a->iter) chkb("bt iter", a->iter, sizeof(int) * (size_t) b, WR);
    if (a->status) chkb("bt status", a->status, sizeof(int) * (size_t) b, WR);
    bd_out(&a->d);
}
int qrd_bt_solve(void* s, const qrd_bt_args* a)
{
    if (!a || a->d.batch <= 0) return 0;
    if (bt_bad_args(a) || !a->d.R || a->d.ldr < a->d.n) return -7;
    op_begin(s, "bt_solve");
    bd_in(&a->d, 1); bt_io(a);
    return 0;
}
int qrd_bt_fused(void* s, double* A, int m, int lda, size_t sA, double* tau, size_t st, double* B, const qrd_bt_args* a)
{
    if (!a || a->d.batch <= 0) return 0;
    qrd_bt_args b = *a;
    b.d.Z = B; b.d.zrows = b.d.n;
    if (bt_bad_args(&b) || !A || !tau || !B || m < a->d.n || m > 64 || !qrd_bd_wave_route(a->d.n + 1) || lda < m || a->d.ldz < m || a->d.R ||
        a->d.rss || a->d.jpvt || a->d.flip)
        return -7;
    op_begin(s, "bt_fused");
    fused_front(A, m, a->d.n, lda, sA, tau, st, B, 1, a->d.ldz, a->d.sZ, a->d.batch);
    bd_in(&a->d, 0); bt_io(a);
    return 0;
}

/* ---- qr_batched_lm.hip: sections 8m (qrd_blm_*) and 8n (qrd_blmb_*) ---- */
static int blm_bad_state(const qrd_blm_state* s)
{
    return !s->x || !s->xtrial || !s->D || !s->delta || !s->par || !s->fnorm || !s->xnorm || !s->pnorm || !s->gnorm || !s->prered || !s->dirder ||
           !s->iter || !s->nfev || !s->njev || !s->accepted || !s->status || !s->info || !s->par_status;
}
static void blm_state_chk(const qrd_blm_state* s, int n, int b)
{
    double* const vec[] = {s->x, s->xtrial, s->D};
    double* const one[] = {s->delta, s->par, s->fnorm, s->xnorm, s->pnorm, s->gnorm, s->prered, s->dirder};
    int* const word[] = {s->iter, s->nfev, s->njev, s->accepted, s->status, s->info, s->par_status};
    for (int i = 0; i < 3; ++i) chk("blm state vector", vec[i], (long) n * b, (long) n * b, 1, RW);
    for (int i = 0; i < 8; ++i) chk("blm state scalar", one[i], b, b, 1, RW);
    for (int i = 0; i < 7; ++i) chkb("blm state word", word[i], sizeof(int) * (size_t) b, RW);
}
int qrd_blm_start(void* s, const double* X0, int ldx, size_t sX, const double* D0, size_t sD, int n, int batch, const qrd_blm_state* st, int mode)
{
    if (batch <= 0) return 0;
    if (!st || blm_bad_state(st) || !X0 || n < 1 || n + 1 > QRD_B_MAX_N || ldx < n || (mode == 2 && !D0)) return -7;
    op_begin(s, "blm_start");
    chkv("blm_start X0", X0, sX, n, batch, RD, 0);
    if (mode == 2) chkv("blm_start D0", D0, sD, n, batch, RD, 1);
    blm_state_chk(st, n, batch);
    for (int q = 0; q < batch; ++q) { st->status[q] = 0; st->info[q] = 0; }
    return 0;
}
int qrd_blm_step(void* s, const qrd_blm_step_args* a)
{
    if (!a || a->d.batch <= 0) return 0;
    const qrd_bd_args* d = &a->d;
    if (d->n < 1 || d->n + 1 > QRD_B_MAX_N || d->nrhs != 1 || d->nlam != 1 || !d->R || !d->Z || d->ldr < d->n || d->zrows < d->n ||
        d->ldz < d->zrows || d->flip || d->D || blm_bad_state(&a->s) || !(a->o.par_rtol > 0.0 && a->o.par_rtol < 1.0) || a->o.par_maxit < 1)
        return -7;
    op_begin(s, "blm_step");
    bd_in(d, 1); blm_state_chk(&a->s, d->n, d->batch);
    return 0;
}
/* the words an update leaves, from the script of `entry` ("blm_update", "blmb_update") */
static void blm_update_words(const char* entry, const qrd_blm_state* st, int batch)
{
    double v = 0.0;
    const int scripted = script_take(entry, &v);
    const int running = scripted ? (int) (v < 0.0 ? -v : v) : 0;          /* unscripted: every member finishes, the host loop ends */
    for (int q = 0; q < batch; ++q) {
        st->status[q] = q < running ? 0 : 1;
        st->accepted[q] = !(scripted && v < 0.0);
        if (g_info) st->info[q] = g_info;
    }
}
int qrd_blm_update(void* s, const double* Ft, int m, int ldf, size_t sF, int n, int batch, const qrd_blm_state* st, const qrd_blm_opts* o)
{
    if (batch <= 0) return 0;
    if (!st || !o || blm_bad_state(st) || !Ft || n < 1 || n + 1 > QRD_B_MAX_N || m < 1 || ldf < m) return -7;
    op_begin(s, "blm_update");
    chks("blm_update Ft", Ft, sF, ldf, m, 1, batch, RD, 0); blm_state_chk(st, n, batch);
    blm_update_words("blm_update", st, batch);
    return 0;
}
/* section 8n: the same state, then lo, hi, alpha, peg and clipped */
static int blmb_bad_state(const qrd_blmb_state* s) { return blm_bad_state(&s->b) || !s->lo || !s->hi || !s->alpha || !s->peg || !s->clipped; }
static void blmb_state_chk(const qrd_blmb_state* s, int n, int b)
{
    blm_state_chk(&s->b, n, b);
    chk("blmb state lo", s->lo, (long) n * b, (long) n * b, 1, RW); chk("blmb state hi", s->hi, (long) n * b, (long) n * b, 1, RW);
    chk("blmb state alpha", s->alpha, b, b, 1, RW);
    chkb("blmb state peg", s->peg, sizeof(int) * (size_t) n * (size_t) b, RW); chkb("blmb state clipped", s->clipped, sizeof(int) * (size_t) b, RW);
}
int qrd_blmb_start(void* s, const double* X0, int ldx, size_t sX, const double* D0, size_t sD, const double* Lo, size_t sLo, const double* Hi,
                   size_t sHi, int n, int batch, const qrd_blmb_state* st, int mode)
{
    if (batch <= 0) return 0;
    if (!st || blmb_bad_state(st) || !X0 || n < 1 || n + 1 > QRD_B_MAX_N || ldx < n || (mode == 2 && !D0)) return -7;
    op_begin(s, "blmb_start");
    chkv("blmb_start X0", X0, sX, n, batch, RD, 0);
    if (mode == 2) chkv("blmb_start D0", D0, sD, n, batch, RD, 1);
    if (Lo) chkv("blmb_start Lo", Lo, sLo, n, batch, RD, 1);
    if (Hi) chkv("blmb_start Hi", Hi, sHi, n, batch, RD, 1);
    blmb_state_chk(st, n, batch);
    double v = 0.0;
    const int refused = script_take("blmb_start", &v) ? (int) v : 0;      /* the first v members: bounds that are no box, nothing else written */
    for (int q = 0; q < batch; ++q) {
        if (q < refused) { st->b.info[q] = -2; continue; }
        st->b.status[q] = 0; st->b.info[q] = 0;
    }
    return 0;
}
int qrd_blmb_peg(void* s, double* J, int m, int ldj, size_t sJ, const double* F, size_t sF, int n, int batch, const qrd_blmb_state* st)
{
    if (batch <= 0) return 0;
    if (!st || blmb_bad_state(st) || !J || !F || n < 1 || n + 1 > QRD_B_MAX_N || m < 1 || ldj < m || sJ < (size_t) ldj * (size_t) n || sF < (size_t) m)
        return -7;
    op_begin(s, "blmb_peg");
    chks("blmb_peg J", J, sJ, ldj, m, n, batch, RW, 0); chkv("blmb_peg F", F, sF, m, batch, RD, 0);
    blmb_state_chk(st, n, batch);
    return 0;
}
int qrd_blmb_step(void* s, const qrd_blmb_step_args* a)
{
    if (!a || a->d.batch <= 0) return 0;
    const qrd_bd_args* d = &a->d;
    if (d->n < 1 || d->n + 1 > QRD_B_MAX_N || d->nrhs != 1 || d->nlam != 1 || !d->R || !d->Z || d->ldr < d->n || d->zrows < d->n ||
        d->ldz < d->zrows || d->flip || d->D || blmb_bad_state(&a->s) || !(a->o.par_rtol > 0.0 && a->o.par_rtol < 1.0) || a->o.par_maxit < 1)
        return -7;
    op_begin(s, "blmb_step");
    bd_in(d, 1); blmb_state_chk(&a->s, d->n, d->batch);
    return 0;
}
int qrd_blmb_update(void* s, const double* Ft, int m, int ldf, size_t sF, int n, int batch, const qrd_blmb_state* st, const qrd_blm_opts* o)
{
    if (batch <= 0) return 0;
    if (!st || !o || blmb_bad_state(st) || !Ft || n < 1 || n + 1 > QRD_B_MAX_N || m < 1 || ldf < m) return -7;
    op_begin(s, "blmb_update");
    chks("blmb_update Ft", Ft, sF, ldf, m, 1, batch, RD, 0); blmb_state_chk(st, n, batch);
    blm_update_words("blmb_update", &st->b, batch);
    return 0;
}

/* ---- qr_batched_lse.hip, _bvls.hip, _irls.hip, _lsei.hip, _stats.hip: one launch each, the operands in an argument block ---- */
int qrd_bl_wave_route(int m, int n, int nrhs) { return m <= 64 && n + nrhs <= 32; }
int qrd_bl_max_rows(int n, int p, int nrhs)
{
    if (n < 1 || p < 1 || p > n || nrhs < 1 || nrhs > QRD_B_MAX_N - n) return 0;
    int m = QRD_B_MAX_ROWS;
    while (m >= 1 && sizeof(double) * ((size_t) (n + nrhs) * sb_ld(m) + (size_t) p * sb_ld(n) + (size_t) nrhs * (n + p) + STUB_WG_SMALL) > STUB_LDS_CAP) --m;
    return m >= 1 && m >= n - p ? m : 0;
}
int qrd_bl_solve(void* s, const qrd_bl_args* a)
{
    if (!a) return -7;
    if (a->batch <= 0) return 0;
    const int mr = qrd_bl_max_rows(a->n, a->p, a->nrhs), b = a->batch;
    if (!mr || a->m < 1 || a->m > mr || a->m < a->n - a->p || a->lda < a->m || a->ldc < a->p || a->ldb < a->m || a->ldd < a->p || a->ldx < a->n ||
        (a->L && a->ldl < a->p) || !a->A || !a->C || !a->B || !a->D || !a->X || !a->info)
        return -7;
    op_begin(s, "bl_solve");
    chks("bl A", a->A, a->sA, a->lda, a->m, a->n, b, RD, 0); chks("bl C", a->C, a->sC, a->ldc, a->p, a->n, b, RD, 0);
    chks("bl B", a->B, a->sB, a->ldb, a->m, a->nrhs, b, RD, 0); chks("bl D", a->D, a->sD, a->ldd, a->p, a->nrhs, b, RD, 0);
    chks("bl X", a->X, a->sX, a->ldx, a->n, a->nrhs, b, WR, 0);
    if (a->L) chks("bl L", a->L, a->sL, a->ldl, a->p, a->nrhs, b, WR, 0);
    if (a->resid) chkv("bl resid", a->resid, a->sres, a->nrhs, b, WR, 0);
    info_out(a->info, 1, b);
    return 0;
}
int qrd_bv_wave_route(int m, int n) { return m <= 64 && n + 1 <= 32; }
int qrd_bv_max_rows(int n)
{
    if (n < 1 || n > QRD_B_MAX_N - 1) return 0;
    int m = QRD_B_MAX_ROWS;
    while (m >= n && sizeof(double) * ((size_t) (n + 1) * sb_ld(m) + 6 * (size_t) n + STUB_WG_SMALL) > STUB_LDS_CAP) --m;
    return m >= n ? m : 0;
}
/* one double / one int per member, packed, where given */
static void opt_d(const char* what, double* p, int b, int mode) { if (p) chk(what, p, b, b, 1, mode); }
static void opt_i(const char* what, int* p, int b, int mode) { if (p) chkb(what, p, sizeof(int) * (size_t) b, mode); }
int qrd_bv_solve(void* s, const qrd_bv_args* a)
{
    if (!a) return -7;
    if (a->batch <= 0) return 0;
    const int mr = qrd_bv_max_rows(a->n), b = a->batch;
    if (!mr || a->m < a->n || a->m > mr || a->lda < a->m || a->maxit < 1 || !a->A || !a->B || !a->X || !a->info) return -7;
    op_begin(s, "bv_solve");
    chks("bv A", a->A, a->sA, a->lda, a->m, a->n, b, RD, 0); chkv("bv B", a->B, a->sB, a->m, b, RD, 0);
    if (a->lo) chkv("bv lo", a->lo, a->sbnd, a->n, b, RD, 1);
    if (a->hi) chkv("bv hi", a->hi, a->sbnd, a->n, b, RD, 1);
    chkv("bv X", a->X, a->sX, a->n, b, WR, 0);
    if (a->W) chkv("bv W", a->W, a->sW, a->n, b, WR, 0);
    if (a->state) chki("bv state", a->state, a->sstate, a->n, b, WR);
    opt_d("bv resid", a->resid, b, WR); opt_i("bv iter", a->iter, b, WR); info_out(a->info, 1, b);
    return 0;
}
int qrd_ir_wave_route(int m, int n) { return m <= 64 && n + 1 <= 32; }
int qrd_ir_max_rows(int n)
{
    if (n < 1 || n > QRD_B_MAX_N - 1) return 0;
    int m = QRD_B_MAX_ROWS;
    while (m >= n && sizeof(double) * ((size_t) (n + 1) * sb_ld(m) + 3 * (size_t) m + 2 * (size_t) n + STUB_WG_SMALL) > STUB_LDS_CAP) --m;
    return m >= n ? m : 0;
}
int qrd_ir_solve(void* s, const qrd_ir_args* a)
{
    if (!a) return -7;
    if (a->batch <= 0) return 0;
    const int mr = qrd_ir_max_rows(a->n), b = a->batch;
    if (!mr || a->m < a->n || a->m > mr || a->lda < a->m || a->maxit < 1 || a->loss < 0 || a->loss > 2 || !(a->tune > 0.0) || !(a->tol >= 0.0) ||
        !a->A || !a->B || !a->X || !a->info)
        return -7;
    op_begin(s, "ir_solve");
    chks("ir A", a->A, a->sA, a->lda, a->m, a->n, b, RD, 0); chkv("ir B", a->B, a->sB, a->m, b, RD, 0);
    if (a->prior) chkv("ir prior", a->prior, a->sprior, a->m, b, RD, 1);
    opt_d("ir scale_in", (double*) a->scale_in, b, RD);
    if (a->X0) chkv("ir X0", a->X0, a->sX0, a->n, b, RD, 0);
    chkv("ir X", a->X, a->sX, a->n, b, WR, 0);
    if (a->W) chkv("ir W", a->W, a->sW, a->m, b, WR, 0);
    opt_d("ir scale", a->scale, b, WR); opt_d("ir resid", a->resid, b, WR); opt_i("ir iter", a->iter, b, WR); opt_i("ir status", a->status, b, WR);
    info_out(a->info, 1, b);
    return 0;
}
int qrd_le_wave_route(int m, int n) { return m <= 64 && n + 1 <= 32; }
int qrd_le_max_rows(int n, int mg)
{
    if (n < 1 || n > QRD_B_MAX_N - 1 || mg < 1 || mg > 64) return 0;
    int m = QRD_B_MAX_ROWS;
    while (m >= 1 && sizeof(double) * ((size_t) (n + 1) * sb_ld(m) + (size_t) (n + 1) * sb_ld(n) + 5 * (size_t) mg + 4 * (size_t) n + STUB_WG_SMALL) > STUB_LDS_CAP) --m;
    return m >= 1 ? m : 0;
}
int qrd_le_solve(void* s, const qrd_le_args* a)
{
    if (!a) return -7;
    if (a->batch <= 0) return 0;
    const int mr = qrd_le_max_rows(a->n, a->mg), b = a->batch;
    if (!mr || a->m < 1 || a->m > mr || a->neq < 0 || a->neq > a->n || a->neq > a->mg || a->m + a->neq < a->n || a->lda < a->m || a->ldg < a->mg ||
        a->maxit < 1 || !(a->rcond > 0.0) || !a->A || !a->B || !a->G || !a->H || !a->X || !a->info)
        return -7;
    op_begin(s, "le_solve");
    chks("le A", a->A, a->sA, a->lda, a->m, a->n, b, RD, 0); chkv("le B", a->B, a->sB, a->m, b, RD, 0);
    chks("le G", a->G, a->sG, a->ldg, a->mg, a->n, b, RD, 1); chkv("le H", a->H, a->sH, a->mg, b, RD, 1);
    chkv("le X", a->X, a->sX, a->n, b, WR, 0);
    if (a->MU) chkv("le MU", a->MU, a->sMU, a->mg, b, WR, 0);
    if (a->S) chkv("le S", a->S, a->sS, a->mg, b, WR, 0);
    if (a->state) chki("le state", a->state, a->sstate, a->mg, b, WR);
    opt_d("le resid", a->resid, b, WR); opt_i("le iter", a->iter, b, WR); info_out(a->info, 1, b);
    return 0;
}
int qrd_bs_cov_wave_route(int n) { return n >= 1 && n <= 32; }
int qrd_bs_fit_wave_route(int m, int n) { return m <= 64 && n + 1 <= 32; }
int qrd_bs_max_rows(int n)
{
    if (n < 1 || n > QRD_B_MAX_N - 1) return 0;
    int m = QRD_B_MAX_ROWS;
    while (m >= n && sizeof(double) * ((size_t) (n + 1) * sb_ld(m) + (size_t) n + STUB_WG_SMALL) > STUB_LDS_CAP) --m;
    return m >= n ? m : 0;
}
int qrd_bs_lev_chunks(int mrows) { return mrows < 1 ? 0 : (mrows - 1) / 256 + 1; }
/* C (n x n) and se (n), where given */
static void cov_out(double* C, int ldc, size_t sC, double* se, size_t sse, int n, int b)
{
    if (C) chks("covariance", C, sC, ldc, n, n, b, WR, 0);
    if (se) chkv("standard errors", se, sse, n, b, WR, 0);
}
int qrd_bs_covar(void* s, const qrd_bs_args* a)
{
    if (!a) return -7;
    if (a->batch <= 0) return 0;
    const int b = a->batch;
    if (a->n < 1 || a->n > QRD_B_MAX_N || a->ldr < a->n || !a->R || !a->info || (!a->C && !a->se) || (a->C && a->ldc < a->n) ||
        (a->acc && (!a->rss || !a->rows || a->rhs < 0 || a->rhs >= a->nrhs)))
        return -7;
    op_begin(s, "bs_covar");
    chks("bs_covar R", a->R, a->sR, a->ldr, a->n, a->n, b, RD, 0);
    if (a->jpvt) chki("bs_covar jpvt", a->jpvt, a->sj, a->n, b, RD);
    opt_i("bs_covar rank", (int*) a->rank, b, RD);
    if (a->acc) {
        chk("bs_covar rss", a->rss, (long) a->nrhs * b, (long) a->nrhs * b, 1, RD); opt_i("bs_covar rows", (int*) a->rows, b, RD);
        opt_d("bs_covar sigma2", a->sigma2, b, WR);
    } else opt_d("bs_covar mult", (double*) a->mult, b, RD);
    cov_out(a->C, a->ldc, a->sC, a->se, a->sse, a->n, b); info_out(a->info, 1, b);
    return 0;
}
int qrd_bs_leverage(void* s, const qrd_bs_lev_args* a)
{
    if (!a) return -7;
    if (a->batch <= 0) return 0;
    const int b = a->batch;
    if (a->n < 1 || a->n > QRD_B_MAX_N || a->ldr < a->n || a->mrows < 1 || a->lda < a->mrows || a->nchunk != qrd_bs_lev_chunks(a->mrows) ||
        (size_t) a->batch * (size_t) a->nchunk > 0x7fffffffu || !a->R || !a->A || !a->H || !a->info)
        return -7;
    op_begin(s, "bs_leverage");
    chks("bs_leverage R", a->R, a->sR, a->ldr, a->n, a->n, b, RD, 0); chks("bs_leverage A", a->A, a->sA, a->lda, a->mrows, a->n, b, RD, 0);
    if (a->prior) chkv("bs_leverage prior", a->prior, a->sprior, a->mrows, b, RD, 1);
    if (a->jpvt) chki("bs_leverage jpvt", a->jpvt, a->sj, a->n, b, RD);
    opt_i("bs_leverage rank", (int*) a->rank, b, RD);
    chkv("bs_leverage H", a->H, a->sH, a->mrows, b, WR, 0); info_out(a->info, 1, b);
    return 0;
}
int qrd_bs_fit(void* s, const qrd_bs_fit_args* a)
{
    if (!a) return -7;
    if (a->batch <= 0) return 0;
    const int mr = qrd_bs_max_rows(a->n), b = a->batch;
    if (!mr || a->m < a->n || a->m > mr || a->lda < a->m || !a->A || !a->B || !a->X || !a->info || (a->C && a->ldc < a->n)) return -7;
    op_begin(s, "bs_fit");
    chks("bs_fit A", a->A, a->sA, a->lda, a->m, a->n, b, RD, 0); chkv("bs_fit B", a->B, a->sB, a->m, b, RD, 0);
    if (a->prior) chkv("bs_fit prior", a->prior, a->sprior, a->m, b, RD, 1);
    chkv("bs_fit X", a->X, a->sX, a->n, b, WR, 0);
    if (a->E) chkv("bs_fit E", a->E, a->sE, a->m, b, WR, 0);
    if (a->H) chkv("bs_fit H", a->H, a->sH, a->m, b, WR, 0);
    opt_d("bs_fit sigma2", a->sigma2, b, WR); opt_i("bs_fit dof", a->dof, b, WR);
    cov_out(a->C, a->ldc, a->sC, a->se, a->sse, a->n, b); info_out(a->info, 1, b);
    return 0;
}
