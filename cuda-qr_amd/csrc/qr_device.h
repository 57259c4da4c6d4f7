/* qr_device.h -- internal C interface between the C host layer (qr_host.c) and the HIP launch
 * layer (qr_kernels.hip).  Plain C types only: the host layer never includes a HIP header.
 * All functions return 0 on success or a hipError_t / negative library code. */
#ifndef QR_DEVICE_H
#define QR_DEVICE_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

int qrd_init(void);
int qrd_gemm_nn(void* stream, int M, int N, int K, double alpha, const double* A, int lda, const double* B,
                int ldb, double beta, double* C, int ldc);
/* C = A*B with B upper triangular (V*T): N = K <= 256, N > 32, alpha 1, beta 0 end the k loop of every column tile at the diagonal and
 * never read B below row 128 (floor(j / 128) + 1) of column j; every other call is qrd_gemm_nn.  The same bits as qrd_gemm_nn for
 * finite A (the skipped terms are a * 0, added last).  (qr_host.c holds a weak fallback for device layers without it.) */
int qrd_gemm_nn_tri(void* stream, int M, int N, int K, double alpha, const double* A, int lda, const double* B,
                    int ldb, double beta, double* C, int ldc);
/* the same with the tile forced: 44, 22 or 11 (0: the built-in rule; -1: the generic kernel); kernel tests and A/Bs only */
int qrd_gemm_nn_tri_tile(void* stream, int tile, int M, int N, int K, const double* A, int lda, const double* B, int ldb, double* C,
                         int ldc);
long long qrd_vt_tri_launches(void);        /* products that took the triangle-aware kernel so far in this process */
int qrd_gemm_tn(void* stream, int M, int N, int K, double alpha, const double* A, int lda, const double* B,
                int ldb, double beta, double* C, int ldc, double* slabs, size_t slab_cap, const double* Tm,
                int ldt);
int qrd_gemm_nn_update(void* stream, int M, int N, int K, double alpha, const double* A, int lda, const double* B,
                       int ldb, double beta, double* C, int ldc);
int qrd_gemm_nn_update2(void* stream, int M, int N, int K, double alpha, const double* A, int lda, const double* B,
                        int ldb, double beta, double* C, int ldc);
int qrd_gemm_tn_dual(void* stream, int N1, int N2, int K, const double* A, int lda, const double* B1, int ldb1, const double* B2,
                     int ldb2, const double* Tm, int ldt, double* W, int ldw, double* G2, int ldg, double* slabs, size_t slab_cap);
int qrd_gemm_tn_update(void* stream, int M, int N, int K, double alpha, const double* A, int lda, const double* B,
                       int ldb, double beta, double* C, int ldc, double* slabs, size_t slab_cap);
int qrd_gemm_tn_update_wide(void* stream, int M, int N, int K, double alpha, const double* A, int lda, const double* B,
                            int ldb, double beta, double* C, int ldc, double* slabs, size_t slab_cap);
/* the same product on the even static K split wherever the shape allows it, nwg workgroups (0: from the stream); kernel tests and A/Bs only */
int qrd_gemm_tn_update_even(void* stream, int M, int N, int K, double alpha, const double* A, int lda, const double* B,
                            int ldb, double beta, double* C, int ldc, double* slabs, size_t slab_cap, int nwg);
long long qrd_tn_even_launches(void);       /* even-split launches so far in this process */
int qrd_tn_even_last_grid(void);            /* workgroups of the last one */
/* Kernel tests only: the route the last call of qrd_gemm_nn, qrd_gemm_nn_update / _update2, qrd_gemm_tn / _tn_update (/ _wide / _even),
 * qrd_gemm_nn_batch or qrd_slab_reduce took, written by the launch functions where they decide (one record for the process; a call that
 * returns before it launches anything leaves the record cleared but for the entry and the serial).  Returns the serial.
 *   out[0] entry: 1 nn, 2 nn_update, 3 tn, 4 nn_batch, 5 slab_reduce, 6 nt (qrd_gemm_nt)      out[1] tile TI TJ as two digits (44, 41, 22, 11, 14; nt: 42, 44)
 *   out[2], out[3] the fast interior Mi, Ni (0, 0: one guarded launch over everything; MIXED: the whole M, N)
 *   out[4] ksplit (slabs summed, for slab_reduce; workgroups, for the even split)      out[5] row piece of the reduction (0: none ran)
 *   out[6] flag bits (QRD_ROUTE_*)                                            out[7] serial number of the record */
#define QRD_ROUTE_FAST 1        /* a FAST (unguarded) instantiation ran on the interior */
#define QRD_ROUTE_MIXED 2       /* gemm_tn_kernel<.., MIXED>: one launch, edge tiles guarded */
#define QRD_ROUTE_WIDE 4        /* gemm_tn_wide_kernel */
#define QRD_ROUTE_EVEN 8        /* the even static K split */
#define QRD_ROUTE_KREM 16       /* K % 16 remainder split: the record is the whole-k-tile part's */
#define QRD_ROUTE_TM 32         /* Tm folded in by the reduction */
#define QRD_ROUTE_DIRECT 64     /* no slabs: the product kernel wrote C itself */
#define QRD_ROUTE_W8 128        /* gemm_nn_w8_kernel on the interior */
#define QRD_ROUTE_KEEP 256      /* gemm_nt4_kernel<.., KEEP>: the K loop's barrier leaves the tile two ahead in flight */
int qrd_gemm_last_route(int out[8]);
/* qrd_gemm_nt's record, kept apart so that the products a factorisation runs after its last wide update do not wipe it: the same eight
 * fields, entry 6 (nt), tile 42 (gemm_nt4_kernel, 128 x 64) or 44 (gemm_nt_kernel), out[2], out[3] the M, N of the call, out[7] the
 * number of qrd_gemm_nt launches so far in this process */
#define QRD_ROUTE_ENTRY_NT 6
int qrd_gemm_nt_last_route(int out[8]);
void qrd_gemm_route_note(int entry, int tile, int Mi, int Ni, int flags);     /* qr_gemm_nt.hip -> the records of qr_kernels.hip */
/* second-generation wide update (qr_gemm_nt.hip): W kept transposed, direct-to-LDS tile loads */
int qrd_gemm2_init(void);
int qrd_gemm_nt_ok(int M, int N, int K, const double* A, int lda, const double* Bt, int ldbt, const double* C, int ldc);
/* ... to the four-workgroup kernel of the trailing update: also N = 64 (mod 128), and M = 64 (mod 128) where A is readable to the next multiple of 128 rows */
int qrd_gemm_nt4_ok(int M, int N, int K, const double* A, int lda, const double* Bt, int ldbt, const double* C, int ldc);
int qrd_gemm_nt(void* stream, int M, int N, int K, int sign, const double* A, int lda, const double* Bt, int ldbt,
                double* C, int ldc, int gm, unsigned long long* stamps);
size_t qrd_panel_ws_size(int m);
int qrd_panel_tsqr_init(void);
int qrd_panel_tsqr(void* stream, double* P, int ld, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv,
                   double* ws, int m_cap);
int qrd_slab_reduce(void* stream, int M, int N, int nslab, const double* slabs, int lds, size_t stride, double* out, int ldo);
#define QRD_CHOLQR_WS (10 * 32 * 32 + 16)      /* G1, G2, R1, M, guard words; then L1 and the four fold matrices of the early product */
/* gram_nslab > 0: `slabs` already holds that many 32 x 32 partial Gram matrices of this leaf (qrd_leaf_update_gram) */
int qrd_panel_cholqr(void* stream, double* P, int ld, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv,
                     double* ws, int m_cap, double* cws, double* slabs, size_t slab_cap, int gram_nslab);
/* the leaf and its in-panel products in one call: the long-K product runs in the same launch as the one-workgroup reconstruction */
int qrd_panel_cholqr_ep(void* stream, double* P, int ld, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv,
                        double* ws, int m_cap, double* cws, double* slabs, size_t slab_cap, int gram_nslab,
                        int N1, const double* B1, int ldb1, int N2, const double* B2, int ldb2, double* W, int ldw, double* G2, int ldg,
                        double* ep_slabs, size_t ep_slab_cap, int* did);
/* fused kernels of the leaf chain (qr_leaf_fused.hip) */
int qrd_leaf_fused_init(void);
int qrd_leaf_update_gram(void* stream, int mk, int N, const double* V, int ldv, const double* W, double* C, int ldc, double* gslabs,
                         size_t gslab_cap, int gy, int* nslab);
int qrd_gemm_nn_batch(void* stream, int M, int N, int K, double alpha, const double* A, int lda, size_t sA,
                      const double* B, int ldb, size_t sB, double beta, double* C, int ldc, size_t sC, int batch);
int qrd_larft(void* stream, int nbp, int ib, const double* G, int ldg, const double* tau, double* T, int ldt,
              double* Tt, int build_diag, double* X, int ldx);
int qrd_zero_block(void* stream, double* A, int ld, int rows, int cols);
/* W = T^T Y from the panel's Gram matrix G = V^T V and the leaves' 32 x 32 T blocks on the diagonal of T, no merged T needed (forward
 * substitution over the leaves); -7: shape not taken (kw % 32, nc % 16, kw > 256) */
int qrd_trsm_gt(void* stream, int kw, int nc, const double* G, int ldg, const double* T, int ldt, const double* Y, int ldy, double* W, int ldw);
int qrd_transpose(void* stream, int rows, int cols, const double* S, int lds, double* D, int ldd);   /* D (cols x rows) = S^T */
int qrd_extract_v(void* stream, const double* P, int ld, int mk, int w, double* V, int ldv);
int qrd_extract_r(void* stream, const double* A, int lda, int m, int n, double* R, int ldr, int rrows);
int qrd_extract_r_block(void* stream, const double* A, int lda, int k, int w, double* R, int ldr, int rrows);
int qrd_set_identity(void* stream, double* C, int ld, int rows, int cols, int row_off);
int qrd_copy_block(void* stream, const double* S, int lds, double* D, int ldd, int rows, int cols);
int qrd_copy_blocks(void* stream, const double* S, int lds, size_t sstride, double* D, int ldd, size_t dstride, int rows, int cols, int batch);
int qrd_fill_uniform(void* stream, double* A, int ld, long long rows, int cols, long long row_off,
                     long long total_rows, unsigned long long seed);
double qrd_hash_uniform_host(unsigned long long seed, unsigned long long idx);
int qrd_diff_norm(void* stream, const double* X, int ldx, const double* Y, int ldy, long long rows, int cols,
                  long long row_off, long long total_rows, unsigned long long seed, int sub_identity, double* out);

/* a TALL panel (<= 128 columns) at its full width: CholeskyQR2 + Householder reconstruction in three passes over the panel
 * (qr_panel_cqr.hip): V -> Vw and below the diagonal of A, R, T (complete), tau.  status: 4 device ints, zeroed by the call;
 * status[0] = 1 afterwards: the guard refused the panel and A is untouched.  -7: shape not taken (qrd_panel_cqr_ok).
 * stage1 / stage2 + g1 / g2: the same in two halves with the Gram matrices supplied by the caller (development checks) */
size_t qrd_panel_cqr_ws_doubles(void);
int qrd_panel_cqr_init(void);
int qrd_panel_cqr_ok(int mk, int w);
int qrd_panel_cqr(void* stream, double* A, int lda, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv, double* ws, int* status);
/* the same with Q in a buffer of its own (Qb: mk x w, ld ldq): a refused panel then leaves Vw untouched as well; status[1] counts refused
 * panels (sticky, never reset by the call); hflag (NULL: none): device address of a host word that receives 2 * seq + refused as soon as
 * the verdict exists -- two thirds into the panel, so the host can decide what comes next while the last pass is still running */
int qrd_panel_cqr_q(void* stream, double* A, int lda, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv, double* ws, int* status,
                    double* Qb, int ldq, unsigned* hflag, unsigned seq);
/* parked form (park != 0): V written once, into A (top block: unit lower, zeros above); R stays in ws until qrd_panel_cqr_restore_r;
 * qrd_panel_cqr_r_block: R (upper, zeros below) into a w x w block of its own */
int qrd_panel_cqr_p(void* stream, double* A, int lda, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv, double* ws, int* status,
                    double* Qb, int ldq, unsigned* hflag, unsigned seq, int park);
/* the retry of a panel that call has just refused, preconditioned (shifted CholeskyQR3): same arguments, Qb a buffer of its own */
int qrd_panel_cqr_retry(void* stream, double* A, int lda, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv, double* ws, int* status,
                    double* Qb, int ldq, unsigned* hflag, unsigned seq, int park);
int qrd_panel_cqr_restore_r(void* stream, double* A, int lda, int w, const double* ws, const int* status);   /* status[0] != 0 (refused panel): A stays untouched */
int qrd_panel_cqr_r_block(void* stream, const double* ws, int w, double* D, int ldd);
double* qrd_panel_cqr_g1(double* ws);
double* qrd_panel_cqr_g2(double* ws);
int qrd_panel_cqr_stage1(void* stream, const double* A, int lda, int mk, int w, double* Vw, int ldv, double* ws, int* status);
int qrd_panel_cqr_stage2(void* stream, double* A, int lda, int mk, int w, double* tau, double* T, int ldt, double* Vw, int ldv, double* ws,
                         int* status);
/* a whole outer panel (<= 256 columns, <= 8192 rows) in ONE launch (qr_panel_fused.hip) */
size_t qrd_panel_fused_ws_doubles(void);
int qrd_panel_fused_init(void);
int qrd_panel_fused_merges_t(int wh, int with_gram);   /* 1: a launch with these arguments leaves the panel's complete T (no merge tree behind it) */
int qrd_panel_fused_ok(void* stream, const double* A, int lda, int mk, int wh, const double* Vw, int ldv);
int qrd_panel_fused(void* stream, double* A, int lda, int mk, int wh, double* tau, double* T, int ldt, double* Vw, int ldv,
                    double* G, int ldg, double* ws, unsigned* epoch, int* status);
/* the same with the rows per row workgroup given (0 = the library's choice, 128, 256): kernel unit tests */
int qrd_panel_fused_rows(void* stream, double* A, int lda, int mk, int wh, double* tau, double* T, int ldt, double* Vw, int ldv,
                    double* G, int ldg, double* ws, unsigned* epoch, int* status, int want_rows);

/* the reference's sliding-window schedule on the device (qr_legacy.hip): legacy-layout shim */
size_t qrd_legacy_ws_size(int m, int PR, int PC);
int qrd_legacy_shape_ok(int m, int n, int PR, int PC);
int qrd_legacy_panel(void* stream, double* A, int m, int n, int PR, int PC, int rowPanels, int pc, int pcCount, double* tau, double* wy);
int qrd_legacy_formq(void* stream, const double* A, const double* tau, int m, int n, int PR, int PC, int rowPanels, double* Q);

/* RCCL glue (qr_comm.hip): librccl is dlopen()ed on first use, never linked */
#define QRD_E_NORCCL (-120)   /* librccl.so could not be loaded */
#define QRD_E_RCCL   (-130)   /* an RCCL call failed: -130 - ncclResult_t */
#define QRD_UNIQUE_ID_BYTES 128
int qrd_comm_init_all(void** comms, int n, const int* devs);
int qrd_comm_unique_id(void* id);
int qrd_comm_init_rank(void** comm, int nranks, const void* id, int rank);
int qrd_comm_count(void* comm, int* n);
const char* qrd_rccl_error_string(int r);
int qrd_comm_destroy(void* comm);
int qrd_allgather_f64(void* comm, void* stream, const double* send, double* recv, size_t count);

/* optional roctx ranges around the host-side issue of a step's phases (MI355XQR_ROCTX=1; rocprofv3 --marker-trace) */
void qrd_range_push(const char* name);
void qrd_range_pop(void);

int qrd_malloc(void** p, size_t bytes);
int qrd_free(void* p);
int qrd_memset(void* stream, void* p, int v, size_t bytes);
int qrd_h2d(void* stream, void* d, const void* h, size_t bytes);
int qrd_d2h(void* stream, void* h, const void* d, size_t bytes);
int qrd_d2d(void* stream, void* dst, const void* src, size_t bytes);
int qrd_h2d_2d(void* stream, void* d, size_t dpitch, const void* h, size_t hpitch, size_t width, size_t height);
int qrd_d2h_2d(void* stream, void* h, size_t hpitch, const void* d, size_t dpitch, size_t width, size_t height);
int qrd_stream_create(void** s, int high_priority);
int qrd_stream_create_cumask(void** s, int first, int count);
int qrd_stream_destroy(void* s);
int qrd_capture_begin(void* s);
int qrd_capture_end(void* s, void** exec);
int qrd_graph_launch(void* exec, void* s);
int qrd_graph_destroy(void* exec);
int qrd_stream_sync(void* s);
int qrd_device_sync(void);
int qrd_event_create(void** e);
int qrd_event_create_timing(void** e);          /* timing brackets only: recorded without a system-scope fence */
int qrd_event_create_notiming(void** e);
int qrd_event_destroy(void* e);
int qrd_event_record(void* e, void* s);
int qrd_event_sync(void* e);
int qrd_stream_wait_event(void* s, void* e);
int qrd_event_elapsed_ms(void* a, void* b, float* ms);
int qrd_device_count(int* n);
int qrd_set_device(int d);
int qrd_get_device(int* d);
int qrd_stream_cus(void* s);
int qrd_stream_cus_coresident(void* s);   /* ... that a launch of workgroups waiting for each other may count on (whole multiples of 32 of a mask) */
/* one 32-bit word of pinned host memory mapped into the device (kernels publish small verdicts into it with system scope) */
int qrd_host_word_alloc(unsigned** host, unsigned** dev);
int qrd_host_word_free(unsigned* host);
int qrd_host_register(void* p, size_t bytes);
int qrd_host_unregister(void* p);
const char* qrd_error_string(int e);
int qrd_device_info(char* name, int name_len, int* cus, int* clock_khz, size_t* mem_bytes);
int qrd_probe_mfma_f64(double* out3);
int qrd_probe_copy(double* gbps);

/* least-squares solve (qr_solve.hip, called from qr_solve.c only).
 * qrd_ormqr_skinny: Cs (mk x nrhs, ldc) <- (I - V op(T) V^T) Cs for the panel whose V is the unit lower trapezoid of Ak (mk x w, lda;
 * read in place) and whose T is upper triangular (ldt); trans_t = 1: op(T) = T^T (Q^T C), 0: T (Q C).  ws: qrd_ormqr_skinny_ws doubles.
 * Three launches, fixed-order sums.  -7: shape not taken (w > QRD_SOLVE_MAX_W).
 * qrd_trsm_step: rows [row_lo, l1) of B -= R[.., x0:x1] B[x0:x1], then R[l0:l1, l0:l1] X = B[l0:l1] solved in place (l1 - l0 <= 64,
 * x1 - x0 <= 64; x0 == x1: no update) */
#define QRD_SOLVE_MAX_W 256
int qrd_ormqr_skinny_blocks(int mk, int* rows_per_block);
size_t qrd_ormqr_skinny_ws(int m, int w, int nrhs);    /* doubles of ws for every panel of a matrix of m rows */
int qrd_ormqr_skinny(void* stream, const double* Ak, int lda, int mk, int w, const double* T, int ldt, int trans_t, double* Cs, int ldc,
                     int nrhs, double* ws);
int qrd_trsm_step(void* stream, const double* R, int lda, double* B, int ldb, int nrhs, int row_lo, int l0, int l1, int x0, int x1);

/* minimum-norm solve (qr_minnorm.hip, called from qr_minnorm.c only).
 * qrd_trsm_t_step: the mirror of qrd_trsm_step for R^T X = B: rows [l0, row_hi) of B -= R[x0:x1, rows]^T B[x0:x1], then
 * R[l0:l1, l0:l1]^T X = B[l0:l1] solved in place (l1 - l0 <= 64, x1 - x0 <= 64, x1 <= l0; x0 == x1: no update).
 * qrd_transpose_tiled: D (cols x rows, ldd) = S (rows x cols, lds)^T on 64 x 64 tiles through LDS, both sides contiguous; any sizes,
 * leading dimensions and bases (qrd_transpose above is the per-element kernel for the nb x nb blocks of T). */
int qrd_trsm_t_step(void* stream, const double* R, int lda, double* B, int ldb, int nrhs, int row_hi, int l0, int l1, int x0, int x1);
int qrd_transpose_tiled(void* stream, int rows, int cols, const double* S, int lds, double* D, int ldd);

/* row-append update (qr_update.hip, called from qr_update.c only).
 * qrd_tp_panel: [Rkk (w x w upper triangle, ldr; its strict lower triangle is neither read nor written) ; Bk (p x w, ldb)] factored in
 * place by one workgroup: R' over the triangle, V over Bk, the w x w T (zeros below its diagonal) to Tk (ldt); w <= QRD_TP_W, p <= QRD_TP_MAXROWS.
 * qrd_tp_apply: W = op(Tk) (C1k + Vk^T C2), C1k -= W, C2 -= Vk W over ncols columns (C1k: w rows; C2: p rows), one workgroup per 32
 * columns; trans_t = 1: op(T) = T^T (Q^T C), 0: T (Q C).
 * qrd_tp_colssq_add: acc[c] += |X(0:rows, c)|^2 in a fixed order;  qrd_tp_sqrt: out[i] = sqrt(in[i]).  -7: shape not taken */
#define QRD_TP_W 32
#define QRD_TP_MAXROWS 256
int qrd_tp_panel(void* stream, double* Rkk, int ldr, double* Bk, int ldb, int p, int w, double* Tk, int ldt);
int qrd_tp_apply(void* stream, int trans_t, const double* Vk, int ldv, int p, int w, const double* Tk, int ldt, double* C1k, int ldc1,
                 double* C2, int ldc2, int ncols);
int qrd_tp_colssq_add(void* stream, const double* X, int ldx, int rows, int cols, double* acc);
int qrd_tp_sqrt(void* stream, const double* in, double* out, int n);

/* signed-row update (the signed instances in qr_update.hip, called from qr_downdate.c only): the rows
 * [0, p_add) of a block count +1, the rows [p_add, p) count -1 (S = diag of those signs).  status: one device int, 0 while all is well;
 * every launch reads it first and returns at once when it is not 0.
 * qrd_th_panel: qrd_tp_panel with every inner product over the p rows weighted by S; a column whose d = R(j,j)^2 + b^T S b is <= 0 or
 * not finite writes col0 + j + 1 to *status and ends the launch (nothing is written back).
 * qrd_th_apply: W = Tk^T (C1k + Vk^T S C2), C1k -= W, C2 -= Vk W, the layout of qrd_tp_apply.
 * qrd_th_colssq: acc[c] = max(0, acc[c] + |X(0:p_add, c)|^2 - |X(p_add:p, c)|^2), fixed order.  -7: shape not taken */
int qrd_th_panel(void* stream, double* Rkk, int ldr, double* Bk, int ldb, int p, int p_add, int w, double* Tk, int ldt, int col0, int* status);
int qrd_th_apply(void* stream, const double* Vk, int ldv, int p, int p_add, int w, const double* Tk, int ldt, double* C1k, int ldc1,
                 double* C2, int ldc2, int ncols, const int* status);
int qrd_th_colssq(void* stream, const double* X, int ldx, int p, int p_add, int cols, double* acc, const int* status);

/* one-sided block Jacobi SVD (qr_svd.hip, called from qr_svd.c only).
 * qrd_jsvd_round: one round of the tournament, one workgroup per block pair: pairs = 2 npairs device ints (p, q) in units of
 * QRD_JSVD_BLOCK columns (p == q: the self-pair of a one-block matrix); G is r x n (ldg), V (n x n, ldv) receives the same rotations
 * (NULL: none accumulated); slots[i] = the measure max |s_ij| / sqrt(s_ii s_jj) pair i met BEFORE it rotated; a pair at or below tol
 * is left alone.  qrd_jsvd_fold: word[0] = the maximum of count slots.
 * qrd_jsvd_colnorms: out[c] = |G(:, c)|.  perm (n device ints): column j of the result is column perm[j] & (QRD_JSVD_LEAD - 1) of the
 * input; bit QRD_JSVD_LEAD marks the first column of each cycle (qrd_jsvd_permute walks the cycles in place; qrd_jsvd_gather: values).
 * qrd_jsvd_normalise: G(:, c) /= sig[c] where sig[c] > 0.  qrd_jsvd_pinv_scale: T2[i, :] = T1[i, :] / sig[i] where sig[i] > rc sig[0],
 * else 0 (both n x nrhs, ld n).  qrd_jsvd_rt: W (n x n, ldw) = R^T of the factored A, zeros above the diagonal.  -7: bad shape */
#define QRD_JSVD_BLOCK 32
#define QRD_JSVD_LEAD 0x40000000
int qrd_jsvd_round(void* stream, double* G, int ldg, int r, int n, double* V, int ldv, const int* pairs, int npairs, double tol, double* slots);
int qrd_jsvd_fold(void* stream, const double* slots, int count, double* word);
int qrd_jsvd_colnorms(void* stream, const double* G, int ldg, int r, int n, double* out);
int qrd_jsvd_gather(void* stream, const double* sig, const int* perm, double* out, int n);
int qrd_jsvd_permute(void* stream, double* M, int ld, int rows, int n, const int* perm);
int qrd_jsvd_normalise(void* stream, double* G, int ldg, int r, int n, const double* sig);
int qrd_jsvd_pinv_scale(void* stream, const double* T1, double* T2, int n, int nrhs, const double* sig, double rc);
int qrd_jsvd_rt(void* stream, const double* A, int lda, int n, double* W, int ldw);

/* column-pivoted factorisation (qr_pivot.hip, called from qr_pivot.c only).
 * The workspace of a plan of n columns: qrd_pivot_ws_doubles(n) doubles and qrd_pivot_ws_ints(n) ints, bound by qrd_pivot_ws_bind.
 *   F      ldf x QRD_PIVOT_NBP   LAPACK dlaqps' F of the current panel (row = column of the matrix)
 *   FT     its trailing rows transposed, for the general product when the block update cannot go to qrd_gemm_nt
 *   P      row-split partial sums of the gemv, vn1 / vn2 / flag: partial norms, their last exact values, columns to recompute
 *   cval / cidx   one pivot candidate per 256 columns; pend: how many columns of the current panel are to be factored (INT_MAX: all)
 * qrd_pivot_norms: exact norms of rows r0.. of the columns from c0 on (all != 0: every one, and jpvt = identity; else the flagged ones),
 * candidates, pend reset.  qrd_pivot_column: column j of the panel at k0, three launches; a no-op once j >= *pend. */
#define QRD_PIVOT_NBP 128
#define QRD_PIVOT_MAX_SPLIT 64
typedef struct qrd_pivot_ws {
    double *F, *FT, *P, *vn1, *vn2, *npart, *alpha, *cval;
    int *flag, *cidx, *pend;
    int ldf;
} qrd_pivot_ws;
size_t qrd_pivot_ws_doubles(int n);
size_t qrd_pivot_ws_ints(int n);
void qrd_pivot_ws_bind(qrd_pivot_ws* w, int n, double* dbuf, int* ibuf);
int qrd_pivot_norms(void* stream, const qrd_pivot_ws* w, const double* A, int lda, int m, int n, int r0, int c0, int all, int* jpvt);
int qrd_pivot_column(void* stream, const qrd_pivot_ws* w, double* A, int lda, int m, int n, int k0, int j, int* jpvt, double* tau);
/* S (n x nrhs, ld n): row jpvt[i] = row i of B for i < r, zero otherwise;  resid[j] = |B(r0:m, j)| */
int qrd_pivot_scatter(void* stream, const double* B, int ldb, int n, int nrhs, int r, const int* jpvt, double* S);
int qrd_pivot_resid(void* stream, const double* B, int ldb, int r0, int m, int nrhs, double* resid);

/* batched small matrices (qr_batched.hip, called from qr_batched.c only).  Matrix
 * q of a batch is at base + q * stride (doubles), column-major.  The route is chosen from (m, columns held) alone: one wave per matrix
 * for m <= 64 and <= 32 columns (qrd_b_wave_route), else one workgroup per matrix with the matrix in LDS.
 * qrd_b_max_rows: the rows that fit for every column count of ncols' class (<= 32: 512, <= 64: 256; 0: too many columns);
 * qrd_b_fits: whether this very shape fits (m <= QRD_B_MAX_ROWS and ncols columns at a leading dimension of 2 mod 32 within 160 KiB).
 * qrd_b_geqrf: dgeqr2 of every A; nrhs > 0 (the fused gels): B's columns ride along (B <- Q^T B; n + nrhs columns are held), info[q] = 0
 * or the smallest i + 1 with R(i,i) == 0, and where it is 0 rows 0..n-1 of B <- R^-1 of them, all in the one launch.
 * qrd_b_ormqr: C <- Q^T C (trans_t = 1) or Q C (0), one launch.  qrd_b_eye: the m x n identity.  qrd_b_trsm: info and the back
 * substitution on their own (n <= QRD_B_MAX_N, any nrhs).  batch <= 0: nothing is launched.  -7: shape not taken */
#define QRD_B_MAX_N 64
#define QRD_B_MAX_ROWS 512
int qrd_b_max_rows(int ncols);
int qrd_b_fits(int m, int ncols);
int qrd_b_wave_route(int m, int ncols);
int qrd_b_geqrf(void* stream, double* A, int m, int n, int lda, size_t strideA, double* tau, size_t stridetau, double* B, int nrhs, int ldb,
                size_t strideB, int* info, int batch);
int qrd_b_ormqr(void* stream, int trans_t, const double* A, int m, int n, int lda, size_t strideA, const double* tau, size_t stridetau,
                double* Cm, int nrhs, int ldc, size_t strideC, int batch);
int qrd_b_eye(void* stream, double* Q, int m, int n, int ldq, size_t strideQ, int batch);
int qrd_b_trsm(void* stream, const double* A, int n, int lda, size_t strideA, double* B, int nrhs, int ldb, size_t strideB, int* info, int batch);
/* the same with column pivoting (mi355x_qr.h section 8b; the same two routes, chosen the same way).
 * qrd_b_geqp3: dlaqp2 of every A, jpvt 0-based; nrhs > 0 (the fused gelsp / gelsy): B's columns ride along, then the rank r (the leading
 * run of |R(i,i)| > rcond |R(0,0)|, rcond >= 0), resid[q * nrhs + j] = |(Q^T b_j)(r..m)| and rank[q] (either may be NULL), and X in the
 * caller's column order in rows 0..n-1 of B (minnorm != 0: through [R11 R12] = [T11 0] Z), all in the one launch.
 * qrd_b_rank: rank[q] from the diagonal of R.  qrd_b_solve_piv: rank, resid and X from factors and Q^T B (the composed route). */
int qrd_b_geqp3(void* stream, double* A, int m, int n, int lda, size_t strideA, int* jpvt, size_t stridej, double* tau, size_t stridetau,
                double* B, int nrhs, int ldb, size_t strideB, double rcond, int minnorm, double* resid, int* rank, int batch);
int qrd_b_rank(void* stream, const double* A, int n, int lda, size_t strideA, double rcond, int* rank, int batch);
int qrd_b_solve_piv(void* stream, const double* A, int m, int n, int lda, size_t strideA, const int* jpvt, size_t stridej, double* B, int nrhs,
                    int ldb, size_t strideB, double rcond, int minnorm, double* resid, int* rank, int batch);
/* the batched SVD's kernel (qr_batched_svd.hip; mi355x_qr.h section 8c): from the factors and jpvt of qrd_b_geqp3, per matrix the rank cut
 * r (the leading run of |R(i,i)| > sqrt(n) eps |R(0,0)|), one-sided Jacobi on (R with rows r.. dropped)^T in LDS, S (n values, descending,
 * exact zeros past r), V (n x n, NULL: not wanted) = P times the normalised columns, completed to an orthonormal basis where r < n, and
 * U (m x n, NULL: not wanted) <- [W; 0], the accumulated rotations in sorted column order, which qrd_b_ormqr (trans_t = 0) turns into the
 * left singular vectors.  rank and sweeps may be NULL; info[q] = 0, or 1 where max_sweeps sweeps did not converge.  One launch: a wave
 * per matrix for n <= 32, a workgroup above.  A is read only. */
int qrd_b_jsvd(void* stream, const double* A, int m, int n, int lda, size_t strideA, const int* jpvt, size_t stridej, double* S,
               size_t strideS, double* U, int ldu, size_t strideU, double* V, int ldv, size_t strideV, int* rank, int* sweeps, int* info,
               int max_sweeps, int batch);

/* batched row append / removal (qr_batched_update.hip, called from qr_batched_update.c only;
 * mi355x_qr.h section 8d).  Per member the n x n triangle R (and Z, n x nrhs, riding along) stacked on a block of p rows of
 * n + nrhs columns, of which rows [0, p_add) count +1 and rows [p_add, p) count -1.  The block is described by two pairs of buffers: entry
 * (i, c) of its first n columns is A0[q sA0 + c lda0 + i] for i < p_add and A1[q sA1 + c lda1 + (i - p_add)] otherwise, and C0 / C1 hold
 * the last nrhs columns in the same way (a pair that covers no row is not referenced).
 *   acc == 0  the primitive: V and the transformed right-hand-side rows go back over the block, tau (n per member, stau apart) is written
 *   acc != 0  the accumulator: the block is read only; rss (nrhs per member, packed) <- max(0, rss + |E_add|^2 - |E_del|^2) and rows (one
 *             int per member) += p_add - p_del; a member with p_del > 0 and rows + p_add - p_del < n gets info -1 before any arithmetic
 * info (one int per member; may be NULL when p_add == p): 0, the failing column + 1, or -1; on a non-zero value nothing else is written
 * for that member.  One launch: a wave per member for n + nrhs <= 32 and p <= 64 (qrd_bu_wave_route), else a workgroup per member.
 * qrd_bu_max_rows: QRD_BU_MAXROWS for 1 .. 32 columns (one block row per thread), QRD_BU_MAXROWS_WIDE for 33 .. 64 (64 columns at a
 * leading dimension of 226 beside the 64 x 65 triangle are 149 568 of the 163 840 bytes; the next leading dimension, 258, does not fit),
 * 0 otherwise.
 * qrd_bu_apply: [C1 ; C2] <- the stored transformation (trans_t = 1) or, for p_add == p only, its inverse (0), any nrhs >= 1, one launch.
 * qrd_bu_solve_prep: X_q <- Z_q and resid (may be NULL) <- sqrt(rss), ahead of qrd_b_trsm.  batch <= 0: nothing is launched.  -7: shape not taken */
#define QRD_BU_MAXROWS 256
#define QRD_BU_MAXROWS_WIDE 226
typedef struct qrd_bu_args {
    double *R, *Z, *tau, *rss;
    int *rows, *info;
    double *A0, *A1, *C0, *C1;
    size_t sR, sZ, stau, sA0, sA1, sC0, sC1;
    int ldr, ldz, lda0, lda1, ldc0, ldc1;
    int n, nrhs, p, p_add, batch, acc;
} qrd_bu_args;
int qrd_bu_max_rows(int ncols);
int qrd_bu_wave_route(int ncols, int p);
int qrd_bu_update(void* stream, const qrd_bu_args* a);
int qrd_bu_apply(void* stream, int trans_t, const double* V, int p, int p_add, int n, int ldv, size_t strideV, const double* tau,
                 size_t stridetau, double* C1, int ldc1, size_t strideC1, double* C2, int ldc2, size_t strideC2, int nrhs, int batch);
int qrd_bu_solve_prep(void* stream, const double* Z, int n, int nrhs, double* X, int ldx, size_t strideX, const double* rss, double* resid,
                      size_t strideresid, int batch);

/* batched minimum-norm solves (qr_batched_minnorm.hip, called from qr_batched_minnorm.c only;
 * mi355x_qr.h section 8e).  (m, n) is the shape of the tall matrix F that is factored, m >= n.
 * qrd_bm_fused: factor F and solve F^T X = B for minimum norm in one launch; n + nrhs columns are held (qrd_b_fits(m, n + nrhs)), the
 * route is qrd_b_wave_route(m, n + nrhs).  tr == 0: F is A (lda >= m); tr != 0: F is the transpose of A (n x m, lda >= n), read
 * through the transposed index map.  The factors go to F (ldf >= m; A itself for the in-place call) in qrd_b_geqrf's layout, bitwise
 * qrd_b_geqrf's on the same route.  B (m x nrhs, ldb >= m): rows 0..n-1 on entry, X on return.  info[q] = 0 or the smallest i + 1 with
 * R(i,i) == 0; such a member's B is not written.
 * qrd_bm_apply: the solve alone from existing factors, any nrhs >= 1, one launch.  qrd_bm_transpose: D_q (cols x rows) = S_q^T, rows and
 * cols <= QRD_B_MAX_ROWS.  batch <= 0: nothing is launched.  -7: shape not taken */
int qrd_bm_fused(void* stream, int tr, const double* A, int m, int n, int lda, size_t strideA, double* F, int ldf, size_t strideF, double* tau,
                 size_t stridetau, double* B, int nrhs, int ldb, size_t strideB, int* info, int batch);
int qrd_bm_apply(void* stream, const double* A, int m, int n, int lda, size_t strideA, const double* tau, size_t stridetau, double* B, int nrhs,
                 int ldb, size_t strideB, int* info, int batch);
int qrd_bm_transpose(void* stream, const double* S, int rows, int cols, int lds, size_t strideS, double* D, int ldd, size_t strideD, int batch);

/* batched damped least squares (qr_batched_damped.hip, called from qr_batched_damped.c only;
 * mi355x_qr.h section 8f).  Per member and per lambda_k, k < nlam: the n rows of lambda_k diag(d) eliminated against the
 * triangle R with Z riding along, then R~ x = z~.
 *   R (n x n, ldr >= n; the upper triangle is read), Z (zrows x nrhs, ldz >= zrows >= n: rows 0 .. n-1 are the top of Q^T B, the squares
 *   of rows n .. zrows-1 are added to rss), rss (nrhs per member, packed; NULL: 0), jpvt (n per member, sj apart; NULL: the identity; S
 *   uses d[jpvt[j]] in column j and x_j goes to row jpvt[j] of X), D (n per member, sD apart, sD == 0: shared; NULL: ones), lam (nlam per
 *   member, slam apart, slam == 0: shared).  flip: the triangle is read as U(i, k) = R(n-1-k, n-1-i), Z and the rows of X reversed (D and
 *   jpvt must be NULL).
 *   X (xrows x (nlam * nrhs), ldx >= xrows >= n: the solution of (lambda_k, right-hand side r) in column k * nrhs + r, rows n .. xrows-1
 *   written as zeros), xnorm and resid (nlam * nrhs per member, packed, the same order; either may be NULL), info (nlam per member,
 *   packed): 0, or i + 1 for the smallest i with R~(i,i) == 0, and then X, xnorm and resid of that pair are not written.
 * qrd_bd_solve: one launch, a wave per member for n + nrhs <= 32 (qrd_bd_wave_route), else a workgroup per member (n + nrhs <= 64).
 * qrd_bd_fused: m <= 64 and n + nrhs <= 32 only: qrd_b_geqrf's wave factorisation of [A | B], A, tau and B <- Q^T B (all m rows)
 * stored, then the same lambda loop on the registers, one launch; B takes the place of Z (ldz >= m, sZ), rss comes from rows n .. m-1;
 * R, rss, jpvt and flip must be unset, zrows is ignored.  batch <= 0: nothing is launched.  -7: shape not taken */
typedef struct qrd_bd_args {
    const double *R, *Z, *rss, *D, *lam;
    const int* jpvt;
    double *X, *xnorm, *resid;
    int* info;
    size_t sR, sZ, sj, sD, slam, sX;
    int ldr, ldz, ldx;
    int n, nrhs, nlam, zrows, xrows, flip, batch;
} qrd_bd_args;
int qrd_bd_wave_route(int ncols);
int qrd_bd_solve(void* stream, const qrd_bd_args* a);
int qrd_bd_fused(void* stream, double* A, int m, int lda, size_t strideA, double* tau, size_t stridetau, double* B, const qrd_bd_args* a);

/* batched trust-region step (qr_batched_trust.hip, called from qr_batched_trust.c only; mi355x_qr.h section 8g).  Per member the lambda
 * >= 0 with | |D x| - delta | <= rtol delta (or lambda = 0 and |D x| <= (1 + rtol) delta) by MINPACK lmpar's iteration on lambda^2,
 * every elimination being the one qrd_bd_solve runs.
 *   d: the operands of qrd_bd_args with nrhs = 1 and nlam = 1; d.lam is not referenced; X has one column, xnorm, resid and info one
 *   entry per member.  delta (one per member, sdelta apart, 0: shared), lam0 (the starting guess, slam0 apart, 0: shared; NULL: 0), rtol in
 *   (0, 1), maxit >= 1.  lam (the lambda found), iter (the eliminations run; may be NULL), status (0 converged, 1 the Gauss-Newton step
 *   accepted, 2 left by the lower-bound clause, 3 maxit reached; may be NULL): one per member, packed.  info: 0; i + 1 for the smallest i
 *   with R~(i,i) == 0 in an elimination; -1 for a delta that is not a finite positive number; nothing else is written then.
 * qrd_bt_solve: one launch, a wave per member for n + 1 <= 32, else a workgroup per member (n <= 63).  qrd_bt_fused: m <= 64 and
 * n + 1 <= 32 only, the factorisation of qrd_bd_fused in front of the same search.  batch <= 0: nothing is launched.  -7: shape not taken */
typedef struct qrd_bt_args {
    qrd_bd_args d;
    const double *delta, *lam0;
    double* lam;
    int *iter, *status;
    size_t sdelta, slam0;
    double rtol;
    int maxit;
} qrd_bt_args;
int qrd_bt_solve(void* stream, const qrd_bt_args* a);
int qrd_bt_fused(void* stream, double* A, int m, int lda, size_t strideA, double* tau, size_t stridetau, double* B, const qrd_bt_args* a);

/* batched Levenberg-Marquardt (qr_batched_lm.hip, called from qr_batched_lm.c only; mi355x_qr.h section 8m): MINPACK lmder's outer loop
 * per member in two launches per round.
 *   qrd_blm_state: the packed per-member arrays of a solver (x, xtrial, D: n each; the others one each); the fields and their order are
 *   those of the public qr_lm_batched_state.  qrd_blm_opts: the fields of qr_lm_options.
 *   qrd_blm_start: x <- X0 (n per member, sX apart), D <- D0 (mode 2; sD apart, 0: shared) or ones, iter = nfev = 1, everything else 0.
 *   qrd_blm_step: d carries the factors as qrd_bd_args does (R, Z, rss, jpvt, their strides, n, zrows, batch; nrhs = nlam = 1; D, lam, X,
 *   xnorm, resid, info and flip unset).  Per member with status == 0 and info == 0: fnorm, acnorm, the first step's D, xnorm and delta,
 *   gnorm and the gtol test, the search of qrd_bt_solve (the same device code) on D, delta and par, xtrial, prered, dirder, njev.  One
 *   launch: a wave per member for n + 1 <= 32, else a workgroup per member (n <= 63).
 *   qrd_blm_update: Ft (m rows per member, sF apart) is f at xtrial: the gain ratio, delta, par, accept or reject, nfev, the stopping
 *   tests.  One launch, a wave per member.  batch <= 0: nothing is launched.  -7: shape not taken */
typedef struct qrd_blm_state {
    double *x, *xtrial, *D, *delta, *par, *fnorm, *xnorm, *pnorm, *gnorm, *prered, *dirder;
    int *iter, *nfev, *njev, *accepted, *status, *info, *par_status;
} qrd_blm_state;
typedef struct qrd_blm_opts {
    double ftol, xtol, gtol, factor, par_rtol;
    int maxfev, mode, par_maxit;
} qrd_blm_opts;
typedef struct qrd_blm_step_args {
    qrd_bd_args d;
    qrd_blm_state s;
    qrd_blm_opts o;
} qrd_blm_step_args;
int qrd_blm_start(void* stream, const double* X0, int ldx, size_t sX, const double* D0, size_t sD, int n, int batch, const qrd_blm_state* s,
                  int mode);
int qrd_blm_step(void* stream, const qrd_blm_step_args* a);
int qrd_blm_update(void* stream, const double* Ft, int m, int ldf, size_t sF, int n, int batch, const qrd_blm_state* s, const qrd_blm_opts* o);

/* batched Levenberg-Marquardt with box bounds on x (qr_batched_lm.hip, called from qr_batched_lm.c only; mi355x_qr.h section 8n): the
 * loop above with MPFIT's rules for lo <= x <= hi.  The step kernels are section 8m's, instantiated on qrd_blmb_step_args.
 *   qrd_blmb_state: qrd_blm_state, then lo, hi (n per member), peg (n ints per member: -1 held at lo, +1 held at hi, 0 free), alpha (the
 *   fraction of the step taken) and clipped (alpha < 1), one each.
 *   qrd_blmb_start: qrd_blm_start, and lo <- Lo (sLo apart, 0: shared; NULL: -inf), hi <- Hi likewise (NULL: +inf).  A member whose
 *   bounds are no box (lo_j > hi_j or a NaN) or whose x0 lies outside gets info -2 and nothing else of it is written.
 *   qrd_blmb_peg: before the factorisation, on the unfactored J (m x n, ldj, sJ) and f (m, sF): per running member g_j = sum_i J(i,j) f_i
 *   for the columns with x_j on a bound, peg_j from its sign, the held columns of J cleared.  One launch, a wave per member.
 *   qrd_blmb_step: qrd_blm_step, with the step cut to the box between the search and the trial point.  One launch, the routes of
 *   qrd_blm_step.  qrd_blmb_update: qrd_blm_update without the two tests on the reductions while clipped is set.
 * batch <= 0: nothing is launched.  -7: shape not taken */
typedef struct qrd_blmb_state {
    qrd_blm_state b;
    double *lo, *hi, *alpha;
    int *peg, *clipped;
} qrd_blmb_state;
typedef struct qrd_blmb_step_args {
    qrd_bd_args d;
    qrd_blmb_state s;
    qrd_blm_opts o;
} qrd_blmb_step_args;
int qrd_blmb_start(void* stream, const double* X0, int ldx, size_t sX, const double* D0, size_t sD, const double* Lo, size_t sLo,
                   const double* Hi, size_t sHi, int n, int batch, const qrd_blmb_state* s, int mode);
int qrd_blmb_peg(void* stream, double* J, int m, int ldj, size_t sJ, const double* F, size_t sF, int n, int batch, const qrd_blmb_state* s);
int qrd_blmb_step(void* stream, const qrd_blmb_step_args* a);
int qrd_blmb_update(void* stream, const double* Ft, int m, int ldf, size_t sF, int n, int batch, const qrd_blmb_state* s,
                    const qrd_blm_opts* o);

/* batched equality-constrained least squares (qr_batched_lse.hip, called from qr_batched_lse.c only; mi355x_qr.h section 8h).  Per member
 * min |A x - b| subject to C x = d by the null-space method: C^T = Q_c [R_c ; 0], R_c^T y1 = d, A~ = A Q_c, the QR of A~(:, p:n) with
 * A~(:, 0:p) and b - A~(:, 0:p) y1 riding along, R_a y2 = the top of it, x = Q_c [y1 ; y2], resid from the tail, R_c lambda = g.
 *   A: m x n (lda >= m), C: p x n (ldc >= p), B: m x nrhs, D: p x nrhs, none of them written; X: n x nrhs; L (p x nrhs) and resid (nrhs
 *   per member, sres apart) may be NULL.  1 <= p <= n, m >= 1, m + p >= n, nrhs >= 1, n + nrhs <= QRD_B_MAX_N.
 *   info[q]: 0; i + 1 for the smallest i with R_c(i,i) == 0; p + i + 1 for the smallest i with R_a(i,i) == 0; X, L and resid of such a
 *   member are not written.
 * qrd_bl_wave_route: m <= 64 and n + nrhs <= 32, one wave per member; else one workgroup per member, m <= qrd_bl_max_rows(n, p, nrhs):
 * the largest m <= QRD_B_MAX_ROWS whose images fit 160 KiB of LDS (0: the shape is not taken at all).  qrd_bl_solve: one launch.
 * batch <= 0: nothing is launched.  -7: shape not taken */
typedef struct qrd_bl_args {
    const double *A, *C, *B, *D;
    double *X, *L, *resid;
    int* info;
    size_t sA, sC, sB, sD, sX, sL, sres;
    int lda, ldc, ldb, ldd, ldx, ldl;
    int m, n, p, nrhs, batch;
} qrd_bl_args;
int qrd_bl_wave_route(int m, int n, int nrhs);
int qrd_bl_max_rows(int n, int p, int nrhs);
int qrd_bl_solve(void* stream, const qrd_bl_args* a);

/* batched bound-constrained least squares (qr_batched_bvls.hip, called from qr_batched_bvls.c only; mi355x_qr.h section 8i).  Per member
 * min |A x - b| subject to lo <= x <= hi by bounded-variable least squares: the active-set loop of every member runs inside one launch,
 * every candidate a Householder QR of the free columns (in increasing index order, refilled from the untouched A) with r = b - A_B x_B
 * riding along and one back substitution.
 *   A: m x n (lda >= m, m >= n), B: m per member, neither written; lo, hi: n per member, sbnd apart (0: one vector for all members), each
 *   may be NULL (all -inf / all +inf); X: n per member; W (n per member), state (n ints per member), resid and iter (one per member) may
 *   be NULL.  maxit >= 1: the most eliminations per member.
 *   info[q]: 0; -1 for bounds that are no box (lo > hi, a NaN, lo == +inf, hi == -inf); j + 1 for an exactly zero R(i,i) on free column j
 *   (nothing but info is written for either); n + 1 at maxit eliminations (the last iterate, feasible, is written).
 * qrd_bv_wave_route: m <= 64 and n + 1 <= 32, one wave per member; else one workgroup per member, m <= qrd_bv_max_rows(n): the largest
 * m <= QRD_B_MAX_ROWS with 8 ((n + 1) qb_ld(m) + 6 n + 72) bytes within 160 KiB of LDS (0: n is not taken, n < 1 or n > 63).
 * qrd_bv_solve: one launch.  batch <= 0: nothing is launched.  -7: shape not taken */
typedef struct qrd_bv_args {
    const double *A, *B, *lo, *hi;
    double *X, *W, *resid;
    int *state, *iter, *info;
    size_t sA, sB, sbnd, sX, sW, sstate;
    int lda, m, n, maxit, batch;
} qrd_bv_args;
int qrd_bv_wave_route(int m, int n);
int qrd_bv_max_rows(int n);
int qrd_bv_solve(void* stream, const qrd_bv_args* a);

/* batched inequality-constrained least squares (qr_batched_lsei.hip, called from qr_batched_lsei.c only; mi355x_qr.h section 8l).  Per
 * member min |A x - b| subject to G(0:neq) x = h(0:neq), G(neq:mg) x >= h(neq:mg) by a dual active-set loop inside one launch, every
 * candidate the null-space solve of qr_batched_lse.hip on the rows of the set, refilled from the untouched inputs.
 *   A: m x n (lda >= m), B: m per member, G: mg x n (ldg >= mg), H: mg per member, none of them written (sG == 0, sH == 0: shared); X: n
 *   per member; MU, S (mg per member), state (mg ints per member), resid and iter (one per member) may be NULL.  1 <= n <= 63,
 *   1 <= mg <= 64, 0 <= neq <= min(n, mg), m >= 1, m + neq >= n, maxit >= 1, rcond > 0.
 *   info[q]: 0; n + 1 at maxit candidates (the last accepted pair is written); -2 infeasible; -3 an exactly zero R_c(i,i) at the start;
 *   i + 1 an exactly zero R_a(i,i) (nothing but info is written for the last three).
 * qrd_le_wave_route: m <= 64 and n + 1 <= 32, one wave per member; else one workgroup per member, m <= qrd_le_max_rows(n, mg): the
 * largest m <= QRD_B_MAX_ROWS with 8 ((n + 1) qb_ld(m) + (n + 1) qb_ld(n) + 5 mg + 4 n + 72) bytes within 160 KiB of LDS (0: (n, mg) is
 * not taken).  qrd_le_solve: one launch.  batch <= 0: nothing is launched.  -7: shape not taken */
typedef struct qrd_le_args {
    const double *A, *B, *G, *H;
    double *X, *MU, *S, *resid;
    int *state, *iter, *info;
    size_t sA, sB, sG, sH, sX, sMU, sS, sstate;
    double rcond;
    int lda, ldg, m, n, mg, neq, maxit, batch;
} qrd_le_args;
int qrd_le_wave_route(int m, int n);
int qrd_le_max_rows(int n, int mg);
int qrd_le_solve(void* stream, const qrd_le_args* a);

/* batched robust and weighted least squares (qr_batched_irls.hip, called from qr_batched_irls.c only; mi355x_qr.h section 8j).  Per member
 * iteratively reweighted least squares: the reweighting loop of every member runs inside one launch, every solve a Householder QR of the
 * rows of [A | b] (refilled from the untouched inputs) times sqrt(prior_i w_i) and one back substitution.
 *   A: m x n (lda >= m, m >= n), B: m per member, neither written; prior: m per member, sprior apart (0: one vector for all members),
 *   NULL: ones; scale_in: one per member, NULL: the MAD scale of every iterate; X0: n per member, NULL: a cold start (not referenced for
 *   loss 0); X: n per member; W (m per member), scale, resid, iter and status (one per member) may be NULL.  loss 0 / 1 / 2 (least
 *   squares, Huber, bisquare), tune > 0 the tuning constant, tol >= 0, maxit >= 1: the most solves per member.
 *   status[q]: 0 converged (or loss 0), 2 a zero scale, 3 maxit solves.  info[q]: 0; -1 for a prior weight that is negative, NaN or inf or
 *   a scale_in that is no finite positive number; -2 for fewer than n rows of positive weight; i + 1 for an exactly zero R(i,i): nothing
 *   but info is written for such a member.
 * qrd_ir_wave_route: m <= 64 and n + 1 <= 32, one wave per member; else one workgroup per member, m <= qrd_ir_max_rows(n): the largest
 * m <= QRD_B_MAX_ROWS with 8 ((n + 1) qb_ld(m) + 3 m + 2 n + 72) bytes within 160 KiB of LDS (0: n is not taken, n < 1 or n > 63).
 * qrd_ir_solve: one launch.  batch <= 0: nothing is launched.  -7: shape not taken */
typedef struct qrd_ir_args {
    const double *A, *B, *prior, *scale_in, *X0;
    double *X, *W, *scale, *resid;
    int *iter, *status, *info;
    size_t sA, sB, sprior, sX0, sX, sW;
    double tune, tol;
    int lda, m, n, loss, maxit, batch;
} qrd_ir_args;
int qrd_ir_wave_route(int m, int n);
int qrd_ir_max_rows(int n);
int qrd_ir_solve(void* stream, const qrd_ir_args* a);

/* batched covariance, standard errors and leverages (qr_batched_stats.hip, called from qr_batched_stats.c only; mi355x_qr.h section 8k).
 * qrd_bs_covar: per member C = mult P [(R11^T R11)^-1 0; 0 0] P^T from the upper triangle of R (n x n, ldr >= n, n <= QRD_B_MAX_N; the
 *   strict lower triangle is not read), R11 its leading rank x rank block, through T = R11^-1 and T T^T.  jpvt (n per member, sj apart),
 *   rank and mult (one per member) may be NULL: the identity, n and 1.  C (n x n, ldc >= n) and se (n per member) may be NULL, not both.
 *   acc != 0 (the batched accumulator): mult is formed on the device, sigma2 = rss[q nrhs + rhs] / (rows[q] - n) (+inf when rows == n),
 *   written to sigma2 where given, and used as the multiplier where scaled != 0.
 *   info[q]: 0; -1 for a jpvt that is no permutation, a rank outside 0 .. n or a multiplier that is negative, NaN or inf; i + 1 for the
 *   smallest i < rank with R(i,i) == 0; -3 (acc) for scaled with rows == n (acc and scaled: -1 also for a sigma2 that is NaN or inf).  One launch: a wave per member for n <= 32
 *   (qrd_bs_cov_wave_route), else a workgroup per member.
 * qrd_bs_leverage: H[i] = prior_i |R11^-T (P^T a_i)(0 : rank)|^2 for the mrows rows of A (mrows x n, lda >= mrows, any mrows >= 1, not
 *   written); prior as in qrd_ir_args; info -1 also for a prior weight that is negative, NaN or inf.  One launch of batch x nchunk
 *   workgroups, nchunk = qrd_bs_lev_chunks(mrows): 256 rows each, one per thread.
 * qrd_bs_fit: the weighted least-squares fit of qrd_ir_solve at loss 0 with its statistics in one launch: X (n), E (m: b - A x, 0 on
 *   excluded rows), H (m: the leverages), sigma2 = sum p e^2 / dof, dof = (rows with p > 0) - n, C and se as qrd_bs_covar computes them
 *   from the fit's R with the multiplier 1 (scaled == 0) or sigma2 (scaled != 0); everything but X and info may be NULL.  info[q]: 0; -1
 *   a bad prior weight; -2 fewer than n rows with p > 0; -3 scaled with dof == 0; i + 1 an exactly zero R(i,i).
 *   qrd_bs_fit_wave_route: m <= 64 and n + 1 <= 32, one wave per member; else one workgroup per member, m <= qrd_bs_max_rows(n): the
 *   largest m <= QRD_B_MAX_ROWS with 8 ((n + 1) qb_ld(m) + n + 72) bytes within 160 KiB of LDS (0: n is not taken, n < 1 or n > 63).
 * On a non-zero info word nothing else is written for that member.  batch <= 0: nothing is launched.  -7: shape not taken */
typedef struct qrd_bs_args {
    const double *R, *mult, *rss;
    const int *jpvt, *rank, *rows;
    double *C, *se, *sigma2;
    int* info;
    size_t sR, sj, sC, sse;
    int ldr, ldc, n, batch, acc, scaled, nrhs, rhs;
} qrd_bs_args;
typedef struct qrd_bs_lev_args {
    const double *R, *A, *prior;
    const int *jpvt, *rank;
    double* H;
    int* info;
    size_t sR, sj, sA, sprior, sH;
    int ldr, lda, n, mrows, nchunk, batch;
} qrd_bs_lev_args;
typedef struct qrd_bs_fit_args {
    const double *A, *B, *prior;
    double *X, *E, *H, *sigma2, *C, *se;
    int *dof, *info;
    size_t sA, sB, sprior, sX, sE, sH, sC, sse;
    int lda, ldc, m, n, scaled, batch;
} qrd_bs_fit_args;
int qrd_bs_cov_wave_route(int n);
int qrd_bs_fit_wave_route(int m, int n);
int qrd_bs_max_rows(int n);
int qrd_bs_lev_chunks(int mrows);
int qrd_bs_covar(void* stream, const qrd_bs_args* a);
int qrd_bs_leverage(void* stream, const qrd_bs_lev_args* a);
int qrd_bs_fit(void* stream, const qrd_bs_fit_args* a);

#define QRD_LEAFW 32

#ifdef __cplusplus
}
#endif
#endif
